// C ABI of libwct_hip.so (see include/wct_hip.h): context, weight upload, and the
// host-side orchestration of one WCT.predict (wct.py:70-106) as a chain of HIP
// kernel launches on a single stream.  Nothing here touches the CPU oracle.
#include "common.h"
#include "../../include/wct_hip.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include <cmath>
#include <algorithm>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void wct_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* wct_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct ConvLayer {
  half_t* w = nullptr;   // [cout][9][cin]
  float* b = nullptr;
  half_t* ww = nullptr;  // the filters transformed for conv_wino.hip (ConvArgs::w_wino), or null: the direct kernel only
  int cin = 0, cout = 0;
};

struct PlanStep { char kind; int cin, cout, relu; };   // 'C' or 'U'

struct Decoder {
  bool loaded = false;
  std::vector<PlanStep> plan;
  std::vector<ConvLayer> convs;    // every conv but the last
  half_t* last_w = nullptr;        // MFMA A-fragments of the 64->3 conv (see ConvLastArgs::wfrag)
  float* last_b = nullptr;
  // training (wct_train_step): fp32 master copies (HWIO), Adam moments and the last step's gradients, one entry
  // per conv of the plan (the output conv last)
  std::vector<float*> w32, b32, mw, vw, mb, vb, gw, gb;
  std::vector<int> cin, cout;
  float* grad_arena = nullptr;     // gw / gb point into ONE contiguous buffer: a single all-reduce covers a decoder
  size_t grad_count = 0;
};

struct ProfRec { hipEvent_t a, b; int cls; double flops, bytes; };
constexpr int WCT_EIG_WORDS = 2 + 6 * 3;

// A prepared style (wct_style_prepare): the style image on the device and, per level, a small cache of STATES -- the style side
// of that level (common.h: WctStyleRef) for one key.  The bits of a state depend on the partial-sum layout of the (content,
// style) pair it serves and on the mode, so a handle cannot hold one state per level: a call that needs a key the cache does
// not hold computes it from the image in front of its content chain (style_fill) and keeps it, oldest out.
constexpr int STYLE_CACHE_KEYS = 4;                  // states per level and handle
struct StyleState {
  WctStyleKey key; int kind;                         // kind 0: wct_tf, 1: wct_np, 2: AdaIN
  float* buf;                                        // wct_style_state_floats(C)
  unsigned long long stamp;                          // the call that used it last (wct_ctx::style_clock)
};
struct wct_style {
  int Hs = 0, Ws = 0;
  unsigned level_set = 0;                            // bit l: relu<l>_1 is served
  float* img = nullptr;                              // [Hs][Ws][3] fp32 in [0,1]
  std::vector<StyleState> cache[6];
};

// A warm state (wct_warm_create): per level of its set the C x C basis the content eigensolves of a call start from -- the
// re-orthonormalised eigenvectors of the last frame of the previous call -- and whether it holds one yet
struct wct_warm {
  unsigned level_set = 0;                            // bit l: relu<l>_1 is served
  float* basis[6] = {nullptr};
  bool valid[6] = {false};
};

struct wct_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool enc_loaded = false;
  half_t* first_w = nullptr;       // folded conv1_1 as fp16 hi/lo MFMA fragments (ConvFirstArgs::wfrag)
  float* first_b = nullptr;
  ConvLayer enc[12];               // conv1_2 .. conv5_1
  float* first_w32 = nullptr;      // folded conv1_1 weights fp32 [27][64] (data gradient of the feature loss)
  float* enc_wt[12] = {nullptr};   // encoder weights transposed [(tap, cout)][cin] fp32 (B operand of the dgrad GEMM)
  DevBuf train_ws;
  Decoder dec[6];
  DevBuf act[2], feat_c, feat_s[6], img_c, img_s, img_t[2], wct_out, wct_ws, stage[4];
  DevBuf usum_c, usum_s[6], umax;     // feature statistics from the tap epilogues (ConvArgs::usum / umax); umax: [7][32][UMAX_SLOTS] words
  DevBuf mix_in, feat_mix[6];      // a style mix: the K style inputs, and their features per level (K maps back to back)
  DevBuf mask_in;                  // spatial control: the label map (wct_stylize_masked) or the row labels (wct_*_masked)
  std::vector<wct_style*> styles;  // the live prepared styles of this context (wct_style_prepare .. wct_style_free)
  unsigned long long style_clock = 0;   // one tick per call that takes prepared styles
  std::vector<wct_warm*> warms;    // the live warm states of this context (wct_warm_create .. wct_warm_free)
  std::vector<wct_warm*> warm_used;// those that took a basis from solves whose status nobody has read yet (eig_status)

  int* eig_fail = nullptr;         // pinned host memory mapped into the device: [2] eigenproblems that did not converge / had
                                   // non-finite input -- bumped by jacobi_finalize_kernel (then [6 size classes][3] solver
  int* eig_fail_dev = nullptr;     // statistics: matrices, sweeps, max sweeps)
  float ss_alpha = 0.6f;           // style-swap settings (stylize.py:34-37 defaults)
  int ss_patch = 3, ss_stride = 1;
  bool prof = false;
  bool no_wino = false;            // the training forward keeps every layer on the direct kernel (its backward assumes it)
  std::vector<ProfRec> recs;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
  double prof_ms[WCT_PROF_CLASSES] = {0};
  long long prof_n[WCT_PROF_CLASSES] = {0};
  double prof_flops[WCT_PROF_CLASSES] = {0};
  double prof_bytes[WCT_PROF_CLASSES] = {0};
};

static const int LEVEL_C[6] = {0, 64, 128, 256, 512, 512};
static const int ENC_CIN[12] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
static const int ENC_COUT[12] = {64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};

static int ensure(wct_ctx* c, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return WCT_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (b.p) HIP_TRY(hipFree(b.p));
  b.p = nullptr; b.cap = 0;
  size_t want = bytes + bytes / 8 + 4096;
  HIP_TRY(hipMalloc(&b.p, want));
  b.cap = want;
  return WCT_OK;
}

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

struct ProfScope {
  wct_ctx* c; ProfRec r; bool on;
  ProfScope(wct_ctx* ctx, int cls, double flops, double bytes) : c(ctx), on(ctx->prof) {
    if (!on) return;
    if (c->free_events.empty()) {
      hipEventCreate(&r.a); hipEventCreate(&r.b);
    } else {
      r.a = c->free_events.back().first; r.b = c->free_events.back().second;
      c->free_events.pop_back();
    }
    r.cls = cls; r.flops = flops; r.bytes = bytes;
    hipEventRecord(r.a, c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    hipEventRecord(r.b, c->stream);
    c->recs.push_back(r);
  }
};

extern "C" int wct_device_count(int* n) {
  ARG_CHECK(n != nullptr);
  HIP_TRY(hipGetDeviceCount(n));
  return WCT_OK;
}

extern "C" int wct_create(int device, wct_ctx** out) {
  ARG_CHECK(out != nullptr);
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (n <= 0 || device < 0 || device >= n) {
    wct_set_error("no such HIP device %d (count %d)", device, n);
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(device));
  wct_ctx* c = new wct_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    wct_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    delete c;
    return WCT_ERR_HIP;
  }
  const bool ok = hipHostMalloc((void**)&c->eig_fail, WCT_EIG_WORDS * sizeof(int), hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&c->eig_fail_dev, c->eig_fail, 0) == hipSuccess;
  if (!ok) {
    wct_set_error("hipHostMalloc (mapped status words) failed");
    delete c;
    return WCT_ERR_HIP;
  }
  for (int i = 0; i < WCT_EIG_WORDS; ++i) c->eig_fail[i] = 0;
  *out = c;
  return WCT_OK;
}

static void free_layer(ConvLayer& l) {
  if (l.w) hipFree(l.w);
  if (l.b) hipFree(l.b);
  if (l.ww) hipFree(l.ww);
  l = ConvLayer();
}
static void free_decoder(Decoder& d) {
  for (auto& l : d.convs) free_layer(l);
  for (auto* v : {&d.w32, &d.b32, &d.mw, &d.vw, &d.mb, &d.vb})
    for (float* p : *v) if (p) hipFree(p);
  if (d.grad_arena) hipFree(d.grad_arena);
  if (d.last_w) hipFree(d.last_w);
  if (d.last_b) hipFree(d.last_b);
  d = Decoder();
}

static void free_warm(wct_warm* wm) {
  if (!wm) return;
  for (float* b : wm->basis) if (b) hipFree(b);
  delete wm;
}

static void free_style(wct_style* st) {
  if (!st) return;
  for (auto& lv : st->cache)
    for (auto& e : lv) if (e.buf) hipFree(e.buf);
  if (st->img) hipFree(st->img);
  delete st;
}

extern "C" void wct_destroy(wct_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (wct_style* st : c->styles) free_style(st);
  c->styles.clear();
  for (wct_warm* wm : c->warms) free_warm(wm);
  c->warms.clear();
  if (c->first_w) hipFree(c->first_w);
  if (c->first_b) hipFree(c->first_b);
  if (c->first_w32) hipFree(c->first_w32);
  for (int i = 0; i < 12; ++i) if (c->enc_wt[i]) hipFree(c->enc_wt[i]);
  if (c->train_ws.p) hipFree(c->train_ws.p);
  for (auto& l : c->enc) free_layer(l);
  for (auto& d : c->dec) free_decoder(d);
  DevBuf* bufs[] = {&c->act[0], &c->act[1], &c->feat_c, &c->img_c, &c->img_s, &c->img_t[0], &c->img_t[1],
                    &c->wct_out, &c->wct_ws, &c->stage[0], &c->stage[1], &c->stage[2], &c->stage[3]};
  for (DevBuf* b : bufs) if (b->p) hipFree(b->p);
  for (auto& b : c->feat_s) if (b.p) hipFree(b.p);
  for (auto& b : c->usum_s) if (b.p) hipFree(b.p);
  for (auto& b : c->feat_mix) if (b.p) hipFree(b.p);
  if (c->mix_in.p) hipFree(c->mix_in.p);
  if (c->mask_in.p) hipFree(c->mask_in.p);
  if (c->usum_c.p) hipFree(c->usum_c.p);
  if (c->umax.p) hipFree(c->umax.p);
  for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (auto& e : c->free_events) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->eig_fail) hipHostFree(c->eig_fail);
  hipStreamDestroy(c->stream);
  delete c;
}

// After a stream sync: did any eigensolve since the last check fail?  The frames / features of the call are still
// written (best effort, like LAPACK's "did not converge" info > 0), but the status is loud: WCT_STATUS_NOCONV.
// the solves behind the bases that the warm states in c->warm_used took have been judged: a failure leaves those states cold
static void warm_settle(wct_ctx* c, bool failed) {
  if (failed)
    for (wct_warm* wm : c->warm_used)
      for (bool& v : wm->valid) v = false;
  c->warm_used.clear();
}

static int eig_status(wct_ctx* c) {
  const int n_open = c->eig_fail[0], n_nan = c->eig_fail[1];
  warm_settle(c, n_open || n_nan);
  if (!n_open && !n_nan) return WCT_OK;
  c->eig_fail[0] = c->eig_fail[1] = 0;
  wct_set_error("eigensolver: %d covariance matri%s still rotating after the sweep budget, %d with non-finite entries "
                "(NaN/Inf features?); the outputs of this call are not reliable", n_open, n_open == 1 ? "x" : "ces", n_nan);
  return WCT_ERR_NOCONV;
}

// At the START of a blocking call: failures still pending in the status words were raised by EARLIER asynchronous work
// (wct_stylize_batch_dev calls that nobody followed with wct_sync).  They are reported now -- loudly, but named for what
// they are, and before this call runs, so that its own status and sweep counts are never mixed with them.
static int eig_stale(wct_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int n_open = c->eig_fail[0], n_nan = c->eig_fail[1];
  warm_settle(c, n_open || n_nan);
  if (!n_open && !n_nan) return WCT_OK;
  c->eig_fail[0] = c->eig_fail[1] = 0;
  wct_set_error("eigensolver failures of an EARLIER asynchronous wct_stylize_batch_dev call that was not followed by wct_sync "
                "(%d matri%s still rotating after the sweep budget, %d with non-finite entries): the frames of that call are "
                "not reliable; the present call was not started", n_open, n_open == 1 ? "x" : "ces", n_nan);
  return WCT_ERR_NOCONV;
}

extern "C" int wct_sync(wct_ctx* c) {
  ARG_CHECK(c != nullptr);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return eig_status(c);
}

// Solver statistics since the last call (after a stream sync), per size class k (matrices of order 32 * 2^k, k = 0..5):
// out[3k] = matrices solved, out[3k+1] = sum of their sweeps, out[3k+2] = the largest sweep count.  Cleared on read.
extern "C" int wct_eig_stats(wct_ctx* c, long long out[18]) {
  ARG_CHECK(c && out);
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 6; ++k) {
    int* s = c->eig_fail + 2 + k * 3;
    out[3 * k] = s[0]; out[3 * k + 1] = s[1]; out[3 * k + 2] = s[2];
    s[0] = s[1] = s[2] = 0;
  }
  return WCT_OK;
}

extern "C" int wct_get_stream(wct_ctx* c, void** stream_out) {
  ARG_CHECK(c && stream_out);
  *stream_out = (void*)c->stream;
  return WCT_OK;
}

extern "C" int wct_dev_alloc(wct_ctx* c, size_t bytes, void** out) {
  ARG_CHECK(c && out && bytes > 0);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMalloc(out, bytes));
  return WCT_OK;
}
extern "C" int wct_dev_free(wct_ctx* c, void* p) {
  ARG_CHECK(c != nullptr);
  if (p) HIP_TRY(hipFree(p));
  return WCT_OK;
}
extern "C" int wct_h2d(wct_ctx* c, void* dst, const void* src, size_t bytes) {
  ARG_CHECK(c && dst && src);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}
extern "C" int wct_d2h(wct_ctx* c, void* dst, const void* src, size_t bytes) {
  ARG_CHECK(c && dst && src);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------
extern "C" int wct_prof_enable(wct_ctx* c, int on) {
  ARG_CHECK(c != nullptr);
  c->prof = on != 0;
  return WCT_OK;
}
static int prof_drain(wct_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto& r : c->recs) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    c->prof_ms[r.cls] += ms;
    c->prof_n[r.cls] += 1;
    c->prof_flops[r.cls] += r.flops;
    c->prof_bytes[r.cls] += r.bytes;
    c->free_events.push_back({r.a, r.b});
  }
  c->recs.clear();
  return WCT_OK;
}
extern "C" int wct_prof_reset(wct_ctx* c) {
  ARG_CHECK(c != nullptr);
  TRY(prof_drain(c));
  for (int i = 0; i < WCT_PROF_CLASSES; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; c->prof_flops[i] = 0; c->prof_bytes[i] = 0; }
  return WCT_OK;
}
extern "C" int wct_prof_read(wct_ctx* c, double ms[WCT_PROF_CLASSES], long long launches[WCT_PROF_CLASSES],
                             double flops[WCT_PROF_CLASSES], double bytes[WCT_PROF_CLASSES]) {
  ARG_CHECK(c != nullptr);
  TRY(prof_drain(c));
  for (int i = 0; i < WCT_PROF_CLASSES; ++i) {
    if (ms) ms[i] = c->prof_ms[i];
    if (launches) launches[i] = c->prof_n[i];
    if (flops) flops[i] = c->prof_flops[i];
    if (bytes) bytes[i] = c->prof_bytes[i];
  }
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
static int upload(wct_ctx* c, const void* host, size_t bytes, void** dev) {
  HIP_TRY(hipMalloc(dev, bytes));
  HIP_TRY(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}

// Which layers also get their filters packed for the reduced-FLOP kernel (conv_wino.hip).  Decided by the layer's channel counts
// alone -- never by the batch or the image size: a frame must not depend on the batch it is computed in.  WCT_WINOGRAD=0 is a TEST
// hook (read once per process, like WCT_FUSE_CONV1): every layer on the direct kernel, the round-5 bits.
static bool wino_layer(int cin, int cout) {
  static const int on = getenv("WCT_WINOGRAD") ? atoi(getenv("WCT_WINOGRAD")) : 1;
  constexpr int min_ch = 256;
  return on && cin >= min_ch && cout >= min_ch && cin % 64 == 0 && cout % 64 == 0;
}

// HWIO fp32 -> fp16 MFMA A-fragments [cout/32][tap][cin/16][lane][8]: lane l of a fragment holds output
// channel 32*T + (l & 31), input channels 16*k16 + 8*(l >> 5) .. +7 (the v_mfma_f32_32x32x16_f16 A layout),
// so a wave fetches a fragment with ONE fully coalesced 1-KiB load
static int pack_conv(wct_ctx* c, const float* w_hwio, const float* b, int cin, int cout, ConvLayer* out) {
  free_layer(*out);
  std::vector<half_t> packed((size_t)cout * 9 * cin);
  const int c16 = cin / 16;
  for (int tap = 0; tap < 9; ++tap)
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co) {
        const int lane = (co & 31) + 32 * ((ci >> 3) & 1);
        const size_t frag = ((size_t)(co >> 5) * 9 + tap) * c16 + (ci >> 4);
        packed[(frag * 64 + lane) * 8 + (ci & 7)] = (half_t)w_hwio[((size_t)tap * cin + ci) * cout + co];
      }
  TRY(upload(c, packed.data(), packed.size() * sizeof(half_t), (void**)&out->w));
  TRY(upload(c, b, (size_t)cout * sizeof(float), (void**)&out->b));
  out->cin = cin; out->cout = cout;
  if (wino_layer(cin, cout)) {
    // U_f[kx] = sum_ky G[f][ky] g[ky][kx] (Winograd F(2,3) along y), in double, rounded to fp16 once; fragments
    // [cout/32][f*3+kx][cin/16][lane][8] like the direct ones
    static const double G[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    std::vector<half_t> pw((size_t)cout * 12 * cin);
    for (int f = 0; f < 4; ++f)
      for (int kx = 0; kx < 3; ++kx)
        for (int ci = 0; ci < cin; ++ci)
          for (int co = 0; co < cout; ++co) {
            double u = 0;
            for (int ky = 0; ky < 3; ++ky) u += G[f][ky] * (double)w_hwio[((size_t)(ky * 3 + kx) * cin + ci) * cout + co];
            const int lane = (co & 31) + 32 * ((ci >> 3) & 1);
            const size_t frag = ((size_t)(co >> 5) * 12 + f * 3 + kx) * c16 + (ci >> 4);
            pw[(frag * 64 + lane) * 8 + (ci & 7)] = (half_t)(float)u;
          }
    TRY(upload(c, pw.data(), pw.size() * sizeof(half_t), (void**)&out->ww));
  }
  return WCT_OK;
}

extern "C" int wct_set_encoder(wct_ctx* c, const float* pre_w, const float* pre_b,
                               const float* const* w, const float* const* b, int n_layers) {
  ARG_CHECK(c && pre_w && pre_b && w && b && n_layers == 13);
  HIP_TRY(hipSetDevice(c->device));
  // fold the pointwise 'preprocess' conv (vgg_normalised.py:25-26) into conv1_1: a pointwise
  // op commutes with the reflect pad, so  conv1_1(pad(P x + pb)) = conv1_1'(pad(x)) exactly.
  std::vector<float> fw(27 * 64), fb(64);
  const float* w1 = w[0];   // [3][3][3][64]
  for (int co = 0; co < 64; ++co) {
    double acc = b[0][co];
    for (int tap = 0; tap < 9; ++tap)
      for (int cp = 0; cp < 3; ++cp) acc += (double)pre_b[cp] * w1[(tap * 3 + cp) * 64 + co];
    fb[co] = (float)acc;
  }
  for (int tap = 0; tap < 9; ++tap)
    for (int ci = 0; ci < 3; ++ci)
      for (int co = 0; co < 64; ++co) {
        double acc = 0;
        for (int cp = 0; cp < 3; ++cp) acc += (double)pre_w[ci * 3 + cp] * w1[(tap * 3 + cp) * 64 + co];
        fw[(tap * 3 + ci) * 64 + co] = (float)acc;
      }
  if (c->first_w) { hipFree(c->first_w); c->first_w = nullptr; }
  if (c->first_b) { hipFree(c->first_b); c->first_b = nullptr; }
  // hi/lo split fragments: lane l of fragment (t, ks) holds channel 32t + (l&31), k = 16ks + 8(l>>5) .. +7
  std::vector<half_t> frag(2 * 2 * 2 * 64 * 8);
  for (int t = 0; t < 2; ++t)
    for (int ks = 0; ks < 2; ++ks)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
          const int co = t * 32 + (l & 31), k = ks * 16 + (l >> 5) * 8 + j;
          const float wv = k < 27 ? fw[k * 64 + co] : 0.f;
          const half_t hi = (half_t)wv;
          const half_t lo = (half_t)(wv - (float)hi);
          frag[((((t * 2 + ks) * 2 + 0) * 64) + l) * 8 + j] = hi;
          frag[((((t * 2 + ks) * 2 + 1) * 64) + l) * 8 + j] = lo;
        }
  TRY(upload(c, frag.data(), frag.size() * sizeof(half_t), (void**)&c->first_w));
  TRY(upload(c, fb.data(), fb.size() * sizeof(float), (void**)&c->first_b));
  if (c->first_w32) { hipFree(c->first_w32); c->first_w32 = nullptr; }
  TRY(upload(c, fw.data(), fw.size() * sizeof(float), (void**)&c->first_w32));
  for (int i = 0; i < 12; ++i) {
    TRY(pack_conv(c, w[i + 1], b[i + 1], ENC_CIN[i], ENC_COUT[i], &c->enc[i]));
    const int cin = ENC_CIN[i], cout = ENC_COUT[i];
    std::vector<float> wt((size_t)9 * cin * cout);
    for (int tap = 0; tap < 9; ++tap)
      for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co) wt[((size_t)tap * cout + co) * cin + ci] = w[i + 1][((size_t)tap * cin + ci) * cout + co];
    if (c->enc_wt[i]) { hipFree(c->enc_wt[i]); c->enc_wt[i] = nullptr; }
    TRY(upload(c, wt.data(), wt.size() * sizeof(float), (void**)&c->enc_wt[i]));
  }
  c->enc_loaded = true;
  return WCT_OK;
}

static std::vector<PlanStep> decoder_plan(int level) {
  // model.py:255-277 walked from `level` down to 1, then the 3-filter output conv (model.py:298)
  static const int arch5[] = {512, -1, 512, 512, 512, 0};
  static const int arch4[] = {256, -1, 256, 256, 256, 0};
  static const int arch3[] = {128, -1, 128, 0};
  static const int arch2[] = {64, -1, 0};
  static const int arch1[] = {64, 0};
  static const int* archs[6] = {nullptr, arch1, arch2, arch3, arch4, arch5};
  std::vector<PlanStep> plan;
  int cin = LEVEL_C[level];
  for (int d = level; d >= 1; --d)
    for (const int* a = archs[d]; *a != 0; ++a) {
      if (*a < 0) plan.push_back({'U', cin, cin, 0});
      else { plan.push_back({'C', cin, *a, 1}); cin = *a; }
    }
  plan.push_back({'C', cin, 3, 0});
  return plan;
}

extern "C" int wct_set_decoder(wct_ctx* c, int level, const float* const* w, const float* const* b, int n_layers) {
  ARG_CHECK(c && w && b && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  Decoder& d = c->dec[level];
  free_decoder(d);
  d.plan = decoder_plan(level);
  int nconv = 0;
  for (auto& s : d.plan) nconv += s.kind == 'C';
  if (n_layers != nconv) {
    wct_set_error("decoder relu%d_1 needs %d conv layers, got %d", level, nconv, n_layers);
    return WCT_ERR_ARG;
  }
  int i = 0;
  for (auto& s : d.plan) {
    if (s.kind != 'C') continue;
    if (s.cout == 3) {
      // HWIO [3][3][64][3] = [(tap*64+cin)][3] -> A fragments of the 32 x 64 matrix with row tap*3+cout:
      // lane l of k-step ks holds row l&31, cin = 16 ks + 8 (l>>5) .. +7
      std::vector<half_t> w16((size_t)4 * 64 * 8);
      for (int ks = 0; ks < 4; ++ks)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int row = l & 31, cin = ks * 16 + (l >> 5) * 8 + j;
            const int tap = row / 3, co = row % 3;
            w16[((size_t)ks * 64 + l) * 8 + j] = row < 27 ? (half_t)w[i][((size_t)tap * 64 + cin) * 3 + co] : (half_t)0.f;
          }
      TRY(upload(c, w16.data(), w16.size() * sizeof(half_t), (void**)&d.last_w));
      TRY(upload(c, b[i], 3 * sizeof(float), (void**)&d.last_b));
    } else {
      d.convs.emplace_back();
      TRY(pack_conv(c, w[i], b[i], s.cin, s.cout, &d.convs.back()));
    }
    {
      float *w32 = nullptr, *b32 = nullptr;
      TRY(upload(c, w[i], (size_t)9 * s.cin * s.cout * sizeof(float), (void**)&w32));
      TRY(upload(c, b[i], (size_t)s.cout * sizeof(float), (void**)&b32));
      d.w32.push_back(w32); d.b32.push_back(b32); d.cin.push_back(s.cin); d.cout.push_back(s.cout);
    }
    ++i;
  }
  d.loaded = true;
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// encoder / decoder drivers (device pointers, batch B)
// ---------------------------------------------------------------------------
static void level_dims(int H, int W, int level, int* h, int* w) {
  for (int l = 1; l < level; ++l) { H = (H + 1) / 2; W = (W + 1) / 2; }   // 'same' pooling = ceil
  *h = H; *w = W;
}

// every 3x3 conv reflect-pads its input by one pixel, which needs a map of at least 2x2 (tf.pad REFLECT refuses a
// padding >= the dimension just the same): the feature map of the deepest level must still be 2x2
static int check_min_size(const char* what, int H, int W, int level) {
  int h, w;
  level_dims(H, W, level, &h, &w);
  if (h < 2 || w < 2) {
    wct_set_error("%s %dx%d is too small for relu%d_1: its %dx%d feature map cannot be reflect-padded (need >= %dx%d pixels)",
                  what, H, W, level, h, w, (1 << (level - 1)) + 1, (1 << (level - 1)) + 1);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}


static int run_conv(wct_ctx* c, const ConvLayer& l, const half_t* x, half_t* y16, float* y32,
                    int B, int H, int W, int upsample, int relu, int pool = 0, float* usum = nullptr, unsigned* umax = nullptr,
                    bool tap_layer = false) {
  ConvArgs a;
  a.x = x; a.w = l.w; a.bias = l.b; a.y16 = y16; a.y32 = y32; a.usum = usum; a.umax = umax;
  // a layer whose output CAN be tapped (conv2_1 .. conv5_1) stays on the direct kernel in every pass, tapped or not: the kernel
  // of a layer must not depend on which levels the caller asked for (fused == chained, bit for bit)
  a.w_wino = c->no_wino || tap_layer ? nullptr : l.ww;
  a.B = B; a.H = H; a.W = W; a.Cin = l.cin; a.Cout = l.cout; a.upsample = upsample; a.relu = relu; a.pool = pool;
  const double px = (double)B * H * W;
  const double in_px = upsample ? px / 4 : px;
  const double out_px = pool ? (double)B * ((H + 1) / 2) * ((W + 1) / 2) : px;
  // class 9: the launches the reduced-FLOP kernel takes; flops = the DIRECT convolution's (the kernel executes 2/3 of them)
  ProfScope ps(c, conv3x3_wino_takes(a) ? 9 : 0, 2.0 * px * 9 * l.cin * l.cout,
               in_px * l.cin * 2 + out_px * l.cout * ((y16 ? 2 : 0) + (y32 ? 4 : 0)) + 9.0 * l.cin * l.cout * 2);
  return launch_conv3x3(a, c->stream);
}

// img: [B][H][W][3] fp32 device.  taps32[l] (l=1..5): fp32 feature output for relu<l>_1 or null.
// usum / umax (optional, per level like taps32): statistics of the tap, taken by the epilogue that writes it
static int run_encoder(wct_ctx* c, const float* img, int B, int H, int W, int clamp01, int deepest,
                       float* const taps32[6], float* const* usum = nullptr, unsigned* const* umax = nullptr) {
  if (!c->enc_loaded) { wct_set_error("encoder weights not set (wct_set_encoder)"); return WCT_ERR_STATE; }
  ARG_CHECK(deepest >= 1 && deepest <= 5 && H >= 2 && W >= 2);
  const size_t act_bytes = (size_t)B * H * W * 64 * sizeof(half_t);
  TRY(ensure(c, c->act[0], act_bytes));
  TRY(ensure(c, c->act[1], act_bytes));
  half_t* cur = (half_t*)c->act[0].p;
  half_t* nxt = (half_t*)c->act[1].p;
  // relu1_1 is read by conv1_2 only (no tap on it: every content pass of a level >= 2): conv1_1 moves into conv1_2's patch
  // loader (ConvArgs::img1) -- the 64-channel full-resolution map is neither written nor read, and the bits are the same.
  // (WCT_FUSE_CONV1=0: the two launches; test hook, read once per process)
  static const int fuse_conv1_env = getenv("WCT_FUSE_CONV1") ? atoi(getenv("WCT_FUSE_CONV1")) : 1;
  const bool fuse_conv1 = fuse_conv1_env && deepest > 1 && !taps32[1];
  if (!fuse_conv1) {
    ConvFirstArgs a;
    a.x = img; a.wfrag = c->first_w; a.bias = c->first_b;
    a.y16 = deepest > 1 ? cur : nullptr; a.y32 = taps32[1];
    a.B = B; a.H = H; a.W = W; a.clamp01 = clamp01;
    a.usum = usum && taps32[1] ? usum[1] : nullptr; a.umax = a.usum ? umax[1] : nullptr;
    const double px = (double)B * H * W;
    ProfScope ps(c, 1, 2.0 * px * 27 * 64, px * (12 + 64 * ((a.y16 ? 2 : 0) + (a.y32 ? 4 : 0))));
    TRY(launch_conv_first(a, c->stream));
  }
  if (deepest == 1) return WCT_OK;
  // enc[i]: level whose relu*_1 it produces (0 = none), and whether a 'same' max-pool follows it
  // (conv1_2, conv2_2, conv3_4, conv4_4 -- their outputs feed nothing but the pool, so it is fused
  // into their epilogue)
  static const int seq_tap[12] = {0, 2, 0, 3, 0, 0, 0, 4, 0, 0, 0, 5};
  static const int pool_after[12] = {1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0};
  int h = H, w = W;
  for (int i = 0; i < 12; ++i) {
    const ConvLayer& l = c->enc[i];
    const int tap = seq_tap[i];
    const bool last = tap == deepest;
    const bool fuse = pool_after[i];
    float* const us = tap && taps32[tap] && usum ? usum[tap] : nullptr;
    if (i == 0 && fuse_conv1) {
      ConvArgs a;
      a.x = nullptr; a.w = l.w; a.bias = l.b; a.y16 = nxt; a.y32 = nullptr; a.usum = nullptr; a.umax = nullptr;
      a.B = B; a.H = h; a.W = w; a.Cin = 64; a.Cout = 64; a.upsample = 0; a.relu = 1; a.pool = fuse;
      a.img1 = img; a.w1frag = c->first_w; a.bias1 = c->first_b; a.clamp01 = clamp01;
      const double px = (double)B * h * w, out_px = fuse ? (double)B * ((h + 1) / 2) * ((w + 1) / 2) : px;
      ProfScope ps(c, 8, 2.0 * px * (27 * 64 + 9 * 64 * 64), px * 12 + out_px * 64 * 2 + 9.0 * 64 * 64 * 2);
      TRY(launch_conv3x3(a, c->stream));
    } else
    TRY(run_conv(c, l, cur, last ? nullptr : nxt, tap ? taps32[tap] : nullptr, B, h, w, 0, 1, fuse, us, us ? umax[tap] : nullptr, tap != 0));
    half_t* t = cur; cur = nxt; nxt = t;
    if (last) break;
    if (fuse) { h = (h + 1) / 2; w = (w + 1) / 2; }
  }
  return WCT_OK;
}

// feat16: [B][h][w][C] fp16 device (may alias neither act buffer). img_out: [B][h*2^(l-1)][..][3] fp32
static int run_decoder(wct_ctx* c, int level, const half_t* feat16, int B, int h, int w, float* img_out) {
  Decoder& d = c->dec[level];
  if (!d.loaded) { wct_set_error("decoder weights for relu%d_1 not set (wct_set_decoder)", level); return WCT_ERR_STATE; }
  const int scale = 1 << (level - 1);
  const size_t act_bytes = (size_t)B * h * scale * w * scale * 64 * sizeof(half_t);
  const size_t deep_bytes = (size_t)B * h * w * LEVEL_C[level] * sizeof(half_t) * 4;   // after the first upsample, <= 4x
  TRY(ensure(c, c->act[0], act_bytes > deep_bytes ? act_bytes : deep_bytes));
  TRY(ensure(c, c->act[1], act_bytes > deep_bytes ? act_bytes : deep_bytes));
  const half_t* cur = feat16;
  half_t* bufs[2] = {(half_t*)c->act[0].p, (half_t*)c->act[1].p};
  int which = 0, ci = 0, up = 0;
  const size_t nsteps = d.plan.size();
  for (size_t si = 0; si < nsteps; ++si) {
    const PlanStep& s = d.plan[si];
    if (s.kind == 'U') { up = 1; h *= 2; w *= 2; continue; }
    if (s.cout == 3) {
      ARG_CHECK(up == 0);
      ConvLastArgs a;
      a.x = cur; a.wfrag = d.last_w; a.bias = d.last_b; a.y = img_out; a.B = B; a.H = h; a.W = w;
      const double px = (double)B * h * w;
      ProfScope ps(c, 2, 2.0 * px * 576 * 3, px * (128 + 12));
      TRY(launch_conv_last(a, c->stream));
    } else {
      half_t* out = bufs[which];
      TRY(run_conv(c, d.convs[ci++], cur, out, nullptr, B, h, w, up, 1));
      cur = out; which ^= 1; up = 0;
    }
  }
  return WCT_OK;
}

// what the stages of a transform are charged in their profile classes: covariance (4), apply (6), or the one AdaIN launch (7)
struct StageCost { double cov_flops, cov_bytes, apply_flops, apply_bytes, adain_bytes; };

// One transform by a variant's launcher, launch(mode, stages): AdaIN (stages = 0) in one launch, or the covariance, eigensolve
// and apply stages, each timed in its class
template <typename Launch>
static int run_stages(wct_ctx* c, size_t ws_bytes, unsigned flags, const StageCost& cost, Launch&& launch) {
  TRY(ensure(c, c->wct_ws, ws_bytes));
  if (flags & WCT_FLAG_ADAIN) {
    ProfScope ps(c, 7, 0, cost.adain_bytes);
    return launch(0, 0);
  }
  const int mode = (flags & WCT_FLAG_MODE_NP) ? WCT_MODE_NP : WCT_MODE_TF;
  {
    ProfScope ps(c, 4, cost.cov_flops, cost.cov_bytes);
    TRY(launch(mode, WCT_STAGE_COV));
  }
  {
    ProfScope ps(c, 5, 0, 0);
    TRY(launch(mode, WCT_STAGE_EIG));
  }
  ProfScope ps(c, 6, cost.apply_flops, cost.apply_bytes);
  return launch(mode, WCT_STAGE_APPLY);
}

static int run_transform(wct_ctx* c, const float* fc, int Nc, const float* fs, int Ns, int C, int P,
                         float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev,
                         const WctFeatStats* st = nullptr, const WctStyleRef* prep = nullptr /* a prepared style: fs may be null */,
                         const WctWarmRef* warm = nullptr /* a warm state's basis for this level */) {
  const int shared = (flags & WCT_FLAG_STYLE_SHARED) ? 1 : 0;
  const StageCost cost = {(double)P * 2.0 * C * C * ((double)Nc + Ns), (double)P * 2.0 * ((double)Nc + Ns) * C * 4,
                          (double)P * (2.0 * C * C * Nc + 6.0 * C * C * C), (double)P * Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)),
                          (double)P * (2.0 * Nc + 2.0 * Ns) * C * 4 + (double)P * Nc * C * 6};
  return run_stages(c, wct_workspace_bytes(C, Nc, Ns, P), flags, cost, [&](int mode, int stages) {
    if (!stages) return launch_adain(fc, Nc, fs, Ns, C, P, alpha, 1e-5f, out16, out32, c->wct_ws.p, c->wct_ws.cap, c->stream, shared, st, prep);
    return launch_wct(fc, Nc, fs, Ns, C, P, alpha, mode, eps, out16, out32, c->wct_ws.p, c->wct_ws.cap, sweeps_dev, stages, c->stream,
                      shared, c->eig_fail_dev, st, prep, warm);
  });
}

// lambda[k] = weights[k] / sum(weights) (Li et al. 2017, sec. 4.2); refuses K outside 1 .. WCT_MIX_MAX and weights that are
// negative, not finite or sum to zero
static int mix_weights(const float* weights, int K, float* lambda) {
  if (K < 1 || K > WCT_MIX_MAX) { wct_set_error("style mix: K = %d styles, must be 1 .. %d", K, (int)WCT_MIX_MAX); return WCT_ERR_ARG; }
  if (!weights) { wct_set_error("style mix: no weights"); return WCT_ERR_ARG; }
  double sum = 0.0;
  for (int k = 0; k < K; ++k) {
    if (!(weights[k] >= 0.f) || !std::isfinite(weights[k])) {
      wct_set_error("style mix: weight %d is %g; weights must be finite and >= 0", k, (double)weights[k]);
      return WCT_ERR_ARG;
    }
    sum += weights[k];
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) { wct_set_error("style mix: the weights sum to %g, must be > 0", sum); return WCT_ERR_ARG; }
  for (int k = 0; k < K; ++k) lambda[k] = (float)(weights[k] / sum);
  return WCT_OK;
}

// the style-mix counterpart of run_transform (device pointers; one content, K styles); sweeps_dev [2K] or null
static int run_transform_mix(wct_ctx* c, const float* fc, int Nc, const float* const* fs, const int* Ns, int K, const float* lambda,
                             int C, float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev,
                             const WctFeatStats* st = nullptr, const WctStyleRef* prep = nullptr /* K prepared styles: fs may be null */) {
  double ns = 0;
  for (int k = 0; k < K; ++k) ns += Ns[k];
  // (the mix of the K colouring matrices is timed with the tail it belongs to)
  const StageCost cost = {2.0 * C * C * (Nc + ns), 2.0 * (Nc + ns) * C * 4, 2.0 * C * C * Nc + 6.0 * C * C * C * (K + 1) + 2.0 * C * C * K,
                          (double)Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)), (2.0 * Nc + 2.0 * ns) * C * 4 + (double)Nc * C * 6};
  return run_stages(c, wct_mix_workspace_bytes(C, Nc, Ns, K, lambda), flags, cost, [&](int mode, int stages) {
    if (!stages) return launch_adain_mix(fc, Nc, fs, Ns, K, lambda, C, alpha, 1e-5f, out16, out32, c->wct_ws.p, c->wct_ws.cap, c->stream, st, prep);
    return launch_wct_mix(fc, Nc, fs, Ns, K, lambda, C, alpha, mode, eps, out16, out32, c->wct_ws.p, c->wct_ws.cap, sweeps_dev, stages,
                          c->stream, c->eig_fail_dev, st, prep);
  });
}

// Spatial control: refuses K outside 1 .. WCT_MIX_MAX and any label >= K in the n labels
static int mask_check(const uint8_t* labels, size_t n, int K) {
  if (K < 1 || K > WCT_MIX_MAX) { wct_set_error("mask: K = %d styles, must be 1 .. %d", K, (int)WCT_MIX_MAX); return WCT_ERR_ARG; }
  uint8_t top = 0;
  for (size_t i = 0; i < n; ++i) top = labels[i] > top ? labels[i] : top;
  if (top >= K) { wct_set_error("mask: label %d with K = %d styles (labels must be 0 .. K - 1)", (int)top, K); return WCT_ERR_ARG; }
  return WCT_OK;
}

// nk[k] = the rows of label k in an h x w feature map (MaskGeom's rule), on the host: it sizes the launches, and nothing is read back
static void mask_counts(const uint8_t* mask, int Hm, int Wm, int h, int w, int stride, int K, int* nk) {
  for (int k = 0; k < K; ++k) nk[k] = 0;
  for (int i = 0; i < h; ++i) {
    const uint8_t* row = mask + (size_t)std::min(i * stride, Hm - 1) * Wm;
    for (int j = 0; j < w; ++j) ++nk[row[std::min(j * stride, Wm - 1)]];
  }
}

// the masked counterpart of run_transform (device pointers; one content of Nc rows labelled by g, K styles); sweeps_dev [2P] or null
static int run_transform_masked(wct_ctx* c, const float* fc, int Nc, const MaskGeom& g, const int* nk, const float* const* fs,
                                const int* Ns, int K, int C, float alpha, unsigned flags, float eps, half_t* out16, float* out32,
                                int* sweeps_dev) {
  double ns = 0;
  int P = 0;
  for (int k = 0; k < K; ++k) { ns += nk[k] >= 2 ? Ns[k] : 0; P += nk[k] >= 2; }
  // (the covariance stage is charged the compaction and gather as well)
  const StageCost cost = {2.0 * C * C * (Nc + ns), (4.0 * Nc + 2.0 * (Nc + ns)) * C * 4, 2.0 * C * C * Nc + 6.0 * C * C * C * P,
                          (double)Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)), (4.0 * Nc + 2.0 * ns) * C * 4 + (double)Nc * C * 6};
  return run_stages(c, wct_masked_workspace_bytes(C, Nc, nk, Ns, K), flags, cost, [&](int mode, int stages) {
    if (!stages) return launch_adain_masked(fc, Nc, g, nk, fs, Ns, K, C, alpha, 1e-5f, out16, out32, c->wct_ws.p, c->wct_ws.cap, c->stream);
    return launch_wct_masked(fc, Nc, g, nk, fs, Ns, K, C, alpha, mode, eps, out16, out32, c->wct_ws.p, c->wct_ws.cap, sweeps_dev, stages,
                             c->stream, c->eig_fail_dev);
  });
}

// ---------------------------------------------------------------------------
// op-level host entry points
// ---------------------------------------------------------------------------
static int stage_in(wct_ctx* c, int slot, const void* host, size_t bytes, void** dev) {
  TRY(ensure(c, c->stage[slot], bytes));
  HIP_TRY(hipMemcpyAsync(c->stage[slot].p, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = c->stage[slot].p;
  return WCT_OK;
}
static int fetch(wct_ctx* c, void* host, const void* dev, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}

extern "C" int wct_transform(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C,
                             float alpha, int mode, float eps, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out && (mode == WCT_NP || mode == WCT_TF));
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->stage[3], 256));
  TRY(run_transform(c, (float*)dc, Nc, (float*)ds, Ns, C, 1, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps,
                    nullptr, (float*)c->stage[2].p, (int*)c->stage[3].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) TRY(fetch(c, sweeps_out, c->stage[3].p, 2 * sizeof(int)));
  return eig_status(c);
}

extern "C" int wct_adain(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C,
                         float alpha, float epsilon, float* out) {
  ARG_CHECK(c && content && style && out);
  HIP_TRY(hipSetDevice(c->device));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->wct_ws, wct_workspace_bytes(C, Nc, Ns, 1)));
  TRY(launch_adain((float*)dc, Nc, (float*)ds, Ns, C, 1, alpha, epsilon, nullptr, (float*)c->stage[2].p,
                   c->wct_ws.p, c->wct_ws.cap, c->stream, 0));
  return fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4);
}

// the inputs of a one-content, K-style op: the content [Nc][C] in stage 0 (*dc), the K host feature maps [Ns[k]][C] back to back
// in c->mix_in (ds[k] points at map k); room for the output in stage 2 and the sweeps in stage 3
static int stage_in_multi(wct_ctx* c, const float* content, int Nc, const float* const* styles, const int* Ns, int K, int C,
                          void** dc, const float* ds[]) {
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, dc));
  size_t total = 0;
  for (int k = 0; k < K; ++k) { ARG_CHECK(styles[k] && Ns[k] >= 1); total += (size_t)Ns[k] * C * 4; }
  TRY(ensure(c, c->mix_in, total));
  size_t off = 0;
  for (int k = 0; k < K; ++k) {
    char* d = (char*)c->mix_in.p + off;
    HIP_TRY(hipMemcpyAsync(d, styles[k], (size_t)Ns[k] * C * 4, hipMemcpyHostToDevice, c->stream));
    ds[k] = (const float*)d;
    off += (size_t)Ns[k] * C * 4;
  }
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  return ensure(c, c->stage[3], 2 * WCT_MIX_MAX * sizeof(int));
}

extern "C" int wct_transform_mix(wct_ctx* c, const float* content, int Nc, const float* const* styles, const int* Ns, int K,
                                 const float* weights, int C, float alpha, int mode, float eps, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && styles && Ns && out && (mode == WCT_NP || mode == WCT_TF));
  float lambda[WCT_MIX_MAX];
  TRY(mix_weights(weights, K, lambda));
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void* dc;
  const float* ds[WCT_MIX_MAX];
  TRY(stage_in_multi(c, content, Nc, styles, Ns, K, C, &dc, ds));
  TRY(run_transform_mix(c, (float*)dc, Nc, ds, Ns, K, lambda, C, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps,
                        nullptr, (float*)c->stage[2].p, (int*)c->stage[3].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) {
    int sw[2 * WCT_MIX_MAX];
    TRY(fetch(c, sw, c->stage[3].p, 2 * K * sizeof(int)));
    sweeps_out[0] = sw[0];                                     // the content, then style k at slot 2k + 1
    for (int k = 0; k < K; ++k) sweeps_out[1 + k] = sw[2 * k + 1];
  }
  return eig_status(c);
}

extern "C" int wct_adain_mix(wct_ctx* c, const float* content, int Nc, const float* const* styles, const int* Ns, int K,
                             const float* weights, int C, float alpha, float epsilon, float* out) {
  ARG_CHECK(c && content && styles && Ns && out);
  float lambda[WCT_MIX_MAX];
  TRY(mix_weights(weights, K, lambda));
  HIP_TRY(hipSetDevice(c->device));
  void* dc;
  const float* ds[WCT_MIX_MAX];
  TRY(stage_in_multi(c, content, Nc, styles, Ns, K, C, &dc, ds));
  TRY(ensure(c, c->wct_ws, wct_mix_workspace_bytes(C, Nc, Ns, K, lambda)));
  TRY(launch_adain_mix((float*)dc, Nc, ds, Ns, K, lambda, C, alpha, epsilon, nullptr, (float*)c->stage[2].p,
                       c->wct_ws.p, c->wct_ws.cap, c->stream));
  return fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4);
}

// the row labels of a masked transform in c->mask_in, and their counts; g: one row of Nc labels
static int stage_labels(wct_ctx* c, const uint8_t* labels, int Nc, int K, int* nk, MaskGeom* g) {
  TRY(mask_check(labels, (size_t)Nc, K));
  mask_counts(labels, 1, Nc, 1, Nc, 1, K, nk);
  TRY(ensure(c, c->mask_in, (size_t)Nc));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, labels, (size_t)Nc, hipMemcpyHostToDevice, c->stream));
  *g = MaskGeom{(const uint8_t*)c->mask_in.p, 1, Nc, Nc, 1};
  return WCT_OK;
}

extern "C" int wct_transform_masked(wct_ctx* c, const float* content, int Nc, const uint8_t* labels, const float* const* styles,
                                    const int* Ns, int K, int C, float alpha, int mode, float eps, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && labels && styles && Ns && out && Nc >= 1 && (mode == WCT_NP || mode == WCT_TF));
  HIP_TRY(hipSetDevice(c->device));
  int nk[WCT_MIX_MAX];
  MaskGeom g;
  TRY(stage_labels(c, labels, Nc, K, nk, &g));
  TRY(eig_stale(c));
  void* dc;
  const float* ds[WCT_MIX_MAX];
  TRY(stage_in_multi(c, content, Nc, styles, Ns, K, C, &dc, ds));
  TRY(run_transform_masked(c, (float*)dc, Nc, g, nk, ds, Ns, K, C, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps,
                           nullptr, (float*)c->stage[2].p, (int*)c->stage[3].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) {
    int sw[2 * WCT_MIX_MAX];
    TRY(fetch(c, sw, c->stage[3].p, 2 * WCT_MIX_MAX * sizeof(int)));
    for (int k = 0, p = 0; k < K; ++k) {               // pair p = the p-th label with >= 2 rows
      sweeps_out[2 * k] = nk[k] >= 2 ? sw[2 * p] : 0;
      sweeps_out[2 * k + 1] = nk[k] >= 2 ? sw[2 * p + 1] : 0;
      p += nk[k] >= 2;
    }
  }
  return eig_status(c);
}

extern "C" int wct_adain_masked(wct_ctx* c, const float* content, int Nc, const uint8_t* labels, const float* const* styles,
                                const int* Ns, int K, int C, float alpha, float epsilon, float* out) {
  ARG_CHECK(c && content && labels && styles && Ns && out && Nc >= 1);
  HIP_TRY(hipSetDevice(c->device));
  int nk[WCT_MIX_MAX];
  MaskGeom g;
  TRY(stage_labels(c, labels, Nc, K, nk, &g));
  void* dc;
  const float* ds[WCT_MIX_MAX];
  TRY(stage_in_multi(c, content, Nc, styles, Ns, K, C, &dc, ds));
  TRY(ensure(c, c->wct_ws, wct_masked_workspace_bytes(C, Nc, nk, Ns, K)));
  TRY(launch_adain_masked((float*)dc, Nc, g, nk, ds, Ns, K, C, alpha, epsilon, nullptr, (float*)c->stage[2].p,
                          c->wct_ws.p, c->wct_ws.cap, c->stream));
  return fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4);
}

extern "C" int wct_mask_compact(wct_ctx* c, const uint8_t* mask, int Hm, int Wm, int h, int w, int stride, int K, int* perm_out,
                                int* seg_off_out) {
  ARG_CHECK(c && mask && perm_out && seg_off_out && Hm >= 1 && Wm >= 1 && h >= 1 && w >= 1 && stride >= 1);
  TRY(mask_check(mask, (size_t)Hm * Wm, K));
  HIP_TRY(hipSetDevice(c->device));
  const int N = h * w;
  TRY(ensure(c, c->mask_in, (size_t)Hm * Wm));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, mask, (size_t)Hm * Wm, hipMemcpyHostToDevice, c->stream));
  const size_t perm_bytes = ((size_t)N * sizeof(int) + 255) & ~(size_t)255;
  TRY(ensure(c, c->stage[2], perm_bytes + 256 + mask_compact_workspace_bytes(N)));
  int* perm = (int*)c->stage[2].p;
  int* seg_off = (int*)((char*)c->stage[2].p + perm_bytes);
  TRY(launch_mask_compact(MaskGeom{(const uint8_t*)c->mask_in.p, Hm, Wm, w, stride}, N, K, perm, seg_off, (char*)seg_off + 256, c->stream));
  TRY(fetch(c, seg_off_out, seg_off, (K + 1) * sizeof(int)));
  return fetch(c, perm_out, perm, (size_t)N * sizeof(int));
}

extern "C" int wct_mask_compact_batch(wct_ctx* c, const uint8_t* masks, int B, int Hm, int Wm, int h, int w, int stride, int K,
                                      int* perm_out, int* seg_off_out) {
  ARG_CHECK(c && masks && perm_out && seg_off_out && B >= 1 && B <= 32 && Hm >= 1 && Wm >= 1 && h >= 1 && w >= 1 && stride >= 1);
  TRY(mask_check(masks, (size_t)B * Hm * Wm, K));
  HIP_TRY(hipSetDevice(c->device));
  const int N = h * w;
  TRY(ensure(c, c->mask_in, (size_t)B * Hm * Wm));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, masks, (size_t)B * Hm * Wm, hipMemcpyHostToDevice, c->stream));
  const size_t perm_bytes = ((size_t)B * N * sizeof(int) + 255) & ~(size_t)255;
  const size_t seg_bytes = ((size_t)B * (WCT_MIX_MAX + 1) * sizeof(int) + 255) & ~(size_t)255;
  TRY(ensure(c, c->stage[2], perm_bytes + seg_bytes + mask_compact_workspace_bytes(N, B)));
  int* perm = (int*)c->stage[2].p;
  int* seg_off = (int*)((char*)c->stage[2].p + perm_bytes);
  TRY(launch_mask_compact_batch(MaskGeom{(const uint8_t*)c->mask_in.p, Hm, Wm, w, stride}, N, K, B, perm, seg_off, (char*)seg_off + seg_bytes,
                                c->stream));
  std::vector<int> seg((size_t)B * (WCT_MIX_MAX + 1));
  TRY(fetch(c, seg.data(), seg_off, seg.size() * sizeof(int)));
  for (int f = 0; f < B; ++f)
    for (int k = 0; k <= K; ++k) seg_off_out[f * (K + 1) + k] = seg[(size_t)f * (WCT_MIX_MAX + 1) + k];
  return fetch(c, perm_out, perm, (size_t)B * N * sizeof(int));
}

extern "C" int wct_set_style_swap(wct_ctx* c, float ss_alpha, int patch_size, int stride) {
  ARG_CHECK(c && patch_size >= 1 && stride >= 1);
  c->ss_alpha = ss_alpha; c->ss_patch = patch_size; c->ss_stride = stride;
  return WCT_OK;
}

extern "C" int wct_style_swap(wct_ctx* c, const float* content, int hc, int wc, const float* style, int hs, int ws,
                              int C, float alpha, int patch_size, int stride, float eps, float* out) {
  ARG_CHECK(c && content && style && out && hc > 0 && wc > 0 && hs > 0 && ws > 0);
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)hc * wc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)hs * ws * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)hc * wc * C * 4));
  ARG_CHECK(patch_size >= 1 && stride >= 1 && hc >= patch_size && wc >= patch_size && hs >= patch_size && ws >= patch_size);
  TRY(ensure(c, c->wct_ws, style_swap_workspace_bytes(C, hc, wc, hs, ws, patch_size, stride)));
  TRY(launch_style_swap((float*)dc, hc, wc, (float*)ds, hs, ws, C, alpha, patch_size, stride, eps, nullptr,
                        (float*)c->stage[2].p, c->wct_ws.p, c->wct_ws.cap, c->stream, c->eig_fail_dev));
  TRY(fetch(c, out, c->stage[2].p, (size_t)hc * wc * C * 4));
  return eig_status(c);
}

__global__ void extract_diag_kernel(const float* A, float* d, int C) {
  const int m = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < C) d[m * C + k] = A[(size_t)m * C * C + (size_t)k * C + k];
}

// wct_eigh's input contract: the UPPER triangle is authoritative.  The solver reads an element from whichever triangle is
// contiguous for the kernel at hand, so the staged copy is mirrored first (a C caller may pass upper-only data or a matrix
// that is symmetric only to round-off -- ADVICE r4).  In tiles: coalesced rows in, transposed through LDS out.
__global__ __launch_bounds__(256) void mirror_upper_kernel(float* A, int C) {
  __shared__ float t[32][33];
  const int bi = blockIdx.x, bj = blockIdx.y;
  if (bj < bi) return;                                     // tile (bi, bj) of the upper triangle -> tile (bj, bi)
  float* Am = A + (size_t)blockIdx.z * C * C;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, j = bj * 32 + tx;
    t[r][tx] = (i < C && j < C) ? Am[(size_t)i * C + j] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i = bj * 32 + r, j = bi * 32 + tx;           // element (i, j) of the lower side = upper (j, i)
    if (i < C && j < C && i > j) Am[(size_t)i * C + j] = t[tx][r];
  }
}

extern "C" int wct_eigh(wct_ctx* c, const float* A, int C, int nmat, float* evals, float* evecs, int* sweeps_out) {
  ARG_CHECK(c && A && evals && evecs && nmat >= 1 && nmat <= 64);
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  const size_t mb = (size_t)nmat * C * C * 4;
  void* dA;
  TRY(stage_in(c, 0, A, mb, &dA));
  hipLaunchKernelGGL(mirror_upper_kernel, dim3(cdiv(C, 32), cdiv(C, 32), nmat), dim3(256), 0, c->stream, (float*)dA, C);
  TRY(ensure(c, c->stage[1], mb));
  TRY(ensure(c, c->stage[2], (size_t)nmat * C * 4 + 1024));
  TRY(ensure(c, c->wct_ws, jacobi_workspace_bytes(C, nmat)));
  int* sw = (int*)((char*)c->stage[2].p + (size_t)nmat * C * 4);
  {
    ProfScope ps(c, 5, 0, 0);
    TRY(launch_jacobi_eigh((float*)dA, (float*)c->stage[1].p, C, nmat, c->wct_ws.p, c->wct_ws.cap, sw, c->eig_fail_dev, c->stream));
  }
  hipLaunchKernelGGL(extract_diag_kernel, dim3(cdiv(C, 256), nmat), dim3(256), 0, c->stream, (float*)dA, (float*)c->stage[2].p, C);
  TRY(fetch(c, evals, c->stage[2].p, (size_t)nmat * C * 4));
  TRY(fetch(c, evecs, c->stage[1].p, mb));
  if (sweeps_out) TRY(fetch(c, sweeps_out, sw, nmat * sizeof(int)));
  return eig_status(c);
}

extern "C" int wct_conv3x3(wct_ctx* c, const float* x, int H, int W, int Cin, const float* w_hwio, const float* bias,
                           int Cout, int relu, int upsample, float* y) {
  ARG_CHECK(c && x && w_hwio && bias && y);
  HIP_TRY(hipSetDevice(c->device));
  const int Ho = upsample ? 2 * H : H, Wo = upsample ? 2 * W : W;
  ConvLayer l;
  TRY(pack_conv(c, w_hwio, bias, Cin, Cout, &l));
  void* dx;
  int rc = stage_in(c, 0, x, (size_t)H * W * Cin * 4, &dx);
  if (!rc) rc = ensure(c, c->stage[1], (size_t)H * W * Cin * 2);
  if (!rc) rc = ensure(c, c->stage[2], (size_t)Ho * Wo * Cout * 4);
  if (!rc) rc = launch_f32_to_f16((float*)dx, (half_t*)c->stage[1].p, (size_t)H * W * Cin, c->stream);
  if (!rc) rc = run_conv(c, l, (half_t*)c->stage[1].p, nullptr, (float*)c->stage[2].p, 1, Ho, Wo, upsample, relu);
  if (!rc) rc = fetch(c, y, c->stage[2].p, (size_t)Ho * Wo * Cout * 4);
  hipStreamSynchronize(c->stream);
  free_layer(l);
  return rc;
}

// One layer as the PIPELINE runs it: fp16 activations in, fp16 out (returned as fp32), optionally with the fused 2x2 'same'
// max-pool.  algo 0: the pipeline's choice for this layer shape, 1: the direct kernel, 2: the reduced-FLOP kernel (conv_wino.hip;
// an error if the shape is not one it takes).  x: [B][H][W][Cin] fp32 (rounded to fp16 on the device like wct_conv3x3).
extern "C" int wct_conv3x3_f16(wct_ctx* c, const float* x, int B, int H, int W, int Cin, const float* w_hwio, const float* bias,
                               int Cout, int relu, int upsample, int pool, int algo, float* y) {
  ARG_CHECK(c && x && w_hwio && bias && y && B >= 1 && algo >= 0 && algo <= 2);
  HIP_TRY(hipSetDevice(c->device));
  const int Hc = upsample ? 2 * H : H, Wc = upsample ? 2 * W : W;
  const int Ho = pool ? (Hc + 1) / 2 : Hc, Wo = pool ? (Wc + 1) / 2 : Wc;
  ConvLayer l;
  TRY(pack_conv(c, w_hwio, bias, Cin, Cout, &l));
  int rc = WCT_OK;
  if (algo == 2 && !l.ww) {
    // a shape the policy leaves on the direct kernel: pack its Winograd fragments on the device for this call
    float* w32 = nullptr;
    rc = upload(c, w_hwio, (size_t)9 * Cin * Cout * sizeof(float), (void**)&w32);
    if (!rc && hipMalloc((void**)&l.ww, (size_t)Cout * 12 * Cin * sizeof(half_t)) != hipSuccess) { wct_set_error("hipMalloc failed"); rc = WCT_ERR_NOMEM; }
    if (!rc) rc = launch_pack_conv_wino_frag(w32, l.ww, Cin, Cout, c->stream);
    hipStreamSynchronize(c->stream);
    if (w32) hipFree(w32);
  }
  const bool keep = c->no_wino;
  c->no_wino = algo == 1;
  void* dx;
  const size_t nin = (size_t)B * H * W * Cin, nout = (size_t)B * Ho * Wo * Cout;
  if (!rc) rc = stage_in(c, 0, x, nin * 4, &dx);
  if (!rc) rc = ensure(c, c->stage[1], nin * 2);
  if (!rc) rc = ensure(c, c->stage[2], nout * 2);
  if (!rc) rc = ensure(c, c->stage[3], nout * 4);
  if (!rc) rc = launch_f32_to_f16((float*)dx, (half_t*)c->stage[1].p, nin, c->stream);
  if (!rc) {
    ConvArgs a;
    a.x = (half_t*)c->stage[1].p; a.w = l.w; a.bias = l.b; a.y16 = (half_t*)c->stage[2].p; a.y32 = nullptr; a.usum = nullptr; a.umax = nullptr;
    a.B = B; a.H = Hc; a.W = Wc; a.Cin = Cin; a.Cout = Cout; a.upsample = upsample; a.relu = relu; a.pool = pool;
    a.w_wino = c->no_wino ? nullptr : l.ww;
    if (algo == 2 && !conv3x3_wino_takes(a)) { wct_set_error("wct_conv3x3_f16: algo 2 does not take this layer"); rc = WCT_ERR_ARG; }
    if (!rc) {
      const double px = (double)B * Hc * Wc;
      ProfScope ps(c, 0, 2.0 * px * 9 * Cin * Cout, (double)nin * 2 + (double)nout * 2 + 9.0 * Cin * Cout * 2);
      rc = launch_conv3x3(a, c->stream);
    }
  }
  c->no_wino = keep;
  if (!rc) rc = launch_f16_to_f32((half_t*)c->stage[2].p, (float*)c->stage[3].p, nout, c->stream);
  if (!rc) rc = fetch(c, y, c->stage[3].p, nout * 4);
  hipStreamSynchronize(c->stream);
  free_layer(l);
  return rc;
}

extern "C" int wct_maxpool(wct_ctx* c, const float* x, int H, int W, int C, float* y) {
  ARG_CHECK(c && x && y && C % 8 == 0);
  HIP_TRY(hipSetDevice(c->device));
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  void* dx;
  TRY(stage_in(c, 0, x, (size_t)H * W * C * 4, &dx));
  TRY(ensure(c, c->stage[1], (size_t)H * W * C * 2));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * C * 2));
  TRY(ensure(c, c->stage[3], (size_t)Ho * Wo * C * 4));
  TRY(launch_f32_to_f16((float*)dx, (half_t*)c->stage[1].p, (size_t)H * W * C, c->stream));
  TRY(launch_maxpool2x2((half_t*)c->stage[1].p, (half_t*)c->stage[2].p, 1, H, W, C, c->stream));
  TRY(launch_f16_to_f32((half_t*)c->stage[2].p, (float*)c->stage[3].p, (size_t)Ho * Wo * C, c->stream));
  return fetch(c, y, c->stage[3].p, (size_t)Ho * Wo * C * 4);
}

extern "C" int wct_encode(wct_ctx* c, const float* img01, int H, int W, int level, float* feat) {
  ARG_CHECK(c && img01 && feat && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  TRY(check_min_size("image", H, W, level));
  int h, w;
  level_dims(H, W, level, &h, &w);
  void* dimg;
  TRY(stage_in(c, 0, img01, (size_t)H * W * 3 * 4, &dimg));
  const size_t fb = (size_t)h * w * LEVEL_C[level] * 4;
  TRY(ensure(c, c->feat_c, fb));
  float* taps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  taps[level] = (float*)c->feat_c.p;
  TRY(run_encoder(c, (float*)dimg, 1, H, W, 0, level, taps));
  return fetch(c, feat, c->feat_c.p, fb);
}

extern "C" int wct_decode(wct_ctx* c, const float* feat, int h, int w, int level, float* img) {
  ARG_CHECK(c && feat && img && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  const int C = LEVEL_C[level], scale = 1 << (level - 1);
  void* df;
  TRY(stage_in(c, 0, feat, (size_t)h * w * C * 4, &df));
  TRY(ensure(c, c->wct_out, (size_t)h * w * C * 2));
  TRY(launch_f32_to_f16((float*)df, (half_t*)c->wct_out.p, (size_t)h * w * C, c->stream));
  const size_t ib = (size_t)h * scale * w * scale * 3 * 4;
  TRY(ensure(c, c->img_t[0], ib));
  TRY(run_decoder(c, level, (half_t*)c->wct_out.p, 1, h, w, (float*)c->img_t[0].p));
  return fetch(c, img, c->img_t[0].p, ib);
}

extern "C" int wct_coral_stats(wct_ctx* c, const uint8_t* img, int H, int W, double sums[9]) {
  ARG_CHECK(c && img && sums && H > 0 && W > 0);
  HIP_TRY(hipSetDevice(c->device));
  const size_t npix = (size_t)H * W;
  void* dimg;
  TRY(stage_in(c, 0, img, npix * 3, &dimg));
  int nblocks = (int)((npix + 255) / 256);
  if (nblocks > 1024) nblocks = 1024;
  TRY(ensure(c, c->stage[1], (size_t)(nblocks + 1) * 9 * sizeof(unsigned long long)));
  unsigned long long* partial = (unsigned long long*)c->stage[1].p;
  unsigned long long* out9 = partial + (size_t)nblocks * 9;
  TRY(launch_coral_stats((uint8_t*)dimg, npix, partial, nblocks, out9, c->stream));
  unsigned long long host9[9];
  TRY(fetch(c, host9, out9, sizeof(host9)));
  for (int k = 0; k < 9; ++k) sums[k] = (double)host9[k];     // exact: < 2^53
  return WCT_OK;
}

extern "C" int wct_coral_apply(wct_ctx* c, const uint8_t* src, int H, int W, const double M[9],
                               const double src_mean[3], const double src_std[3], const double tgt_mean[3],
                               const double tgt_std[3], uint8_t* out_u8, double* out_f64) {
  ARG_CHECK(c && src && M && src_mean && src_std && tgt_mean && tgt_std && (out_u8 || out_f64) && H > 0 && W > 0);
  HIP_TRY(hipSetDevice(c->device));
  const size_t npix = (size_t)H * W;
  CoralApplyArgs a;
  for (int i = 0; i < 9; ++i) a.M[i] = M[i];
  for (int i = 0; i < 3; ++i) { a.src_mean[i] = src_mean[i]; a.src_std[i] = src_std[i]; a.tgt_mean[i] = tgt_mean[i]; a.tgt_std[i] = tgt_std[i]; }
  void* dsrc;
  TRY(stage_in(c, 0, src, npix * 3, &dsrc));
  if (out_u8) TRY(ensure(c, c->stage[1], npix * 3));
  if (out_f64) TRY(ensure(c, c->stage[2], npix * 3 * sizeof(double)));
  TRY(launch_coral_apply((uint8_t*)dsrc, npix, a, out_u8 ? (uint8_t*)c->stage[1].p : nullptr,
                         out_f64 ? (double*)c->stage[2].p : nullptr, c->stream));
  if (out_u8) TRY(fetch(c, out_u8, c->stage[1].p, npix * 3));
  if (out_f64) TRY(fetch(c, out_f64, c->stage[2].p, npix * 3 * sizeof(double)));
  return WCT_OK;
}

// Luminance-only colour preservation, op level (csrc/colors.hip): the refusals both calls share
static int content_colors_checks(const void* stylized, int Ho, int Wo, const void* content, int Hc, int Wc, int B, const void* out) {
  if (!stylized || !content || !out) { wct_set_error("content colours: null image pointer"); return WCT_ERR_ARG; }
  if (B < 1 || B > 32) { wct_set_error("content colours: B = %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (Hc < 1 || Wc < 1 || Ho < Hc || Wo < Wc) {
    wct_set_error("content colours: a %dx%d stylized frame for a %dx%d content (the frame is never the smaller one)", Ho, Wo, Hc, Wc);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

extern "C" int wct_content_colors_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc,
                                            int Wc, int B, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(content_colors_checks(stylized, Ho, Wo, content, Hc, Wc, B, out));
  HIP_TRY(hipSetDevice(c->device));
  ProfScope ps(c, 7, 0, (double)B * Ho * Wo * 3 * 2 + (double)B * Hc * Wc * 3);
  return launch_content_colors_u8(stylized, content, B, Ho, Wo, Hc, Wc, out, c->stream);
}

extern "C" int wct_content_colors(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc,
                                  uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(content_colors_checks(stylized, Ho, Wo, content, Hc, Wc, 1, out));
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc;
  TRY(stage_in(c, 0, stylized, (size_t)Ho * Wo * 3, &ds));
  TRY(stage_in(c, 1, content, (size_t)Hc * Wc * 3, &dc));
  TRY(wct_content_colors_batch_dev(c, (uint8_t*)ds, Ho, Wo, (uint8_t*)dc, Hc, Wc, 1, (uint8_t*)ds));    // (in place)
  return fetch(c, out, ds, (size_t)Ho * Wo * 3);
}

// ---------------------------------------------------------------------------
// the hot path
// ---------------------------------------------------------------------------
extern "C" int wct_output_size(int Hc, int Wc, const int* levels, int n_levels, int* Ho, int* Wo) {
  ARG_CHECK(levels && Ho && Wo && n_levels >= 1 && Hc >= 2 && Wc >= 2);
  int H = Hc, W = Wc;
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    TRY(check_min_size("content", H, W, levels[i]));
    int h, w;
    level_dims(H, W, levels[i], &h, &w);
    H = h << (levels[i] - 1); W = w << (levels[i] - 1);     // ceil pooling then x2 upsampling
  }
  *Ho = H; *Wo = W;
  return WCT_OK;
}

// The checks of a stylize call before any launch: the levels and their decoders, the output size (*Ho, *Wo), K styles
// large enough for the deepest level (*deepest)
static int stylize_checks(wct_ctx* c, int Hc, int Wc, const uint8_t* const* styles, const int* Hs, const int* Ws, int K,
                          const int* levels, int n_levels, int* deepest, int* Ho, int* Wo) {
  *deepest = 0;
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    if (levels[i] > *deepest) *deepest = levels[i];
    if (!c->dec[levels[i]].loaded) { wct_set_error("decoder weights for relu%d_1 not set", levels[i]); return WCT_ERR_STATE; }
  }
  TRY(wct_output_size(Hc, Wc, levels, n_levels, Ho, Wo));
  for (int k = 0; k < K; ++k) { ARG_CHECK(styles[k]); TRY(check_min_size("style", Hs[k], Ws[k], *deepest)); }
  return WCT_OK;
}

// the content (nc samples) and style (ns) images as fp32 in [0,1] (wct.py:60-64): uint8 ones converted into img_c / img_s
static int images_f32(wct_ctx* c, unsigned flags, const void* content, size_t nc, const void* style, size_t ns, const float** img_c,
                      const float** img_s) {
  *img_c = (const float*)content; *img_s = (const float*)style;
  if (flags & WCT_FLAG_IMAGES_F32) return WCT_OK;
  TRY(ensure(c, c->img_c, nc * 4));
  TRY(ensure(c, c->img_s, ns * 4));
  ProfScope ps(c, 7, 0, (double)(nc + ns) * 5);
  TRY(launch_u8_to_f32((const uint8_t*)content, (float*)c->img_c.p, nc, c->stream));
  TRY(launch_u8_to_f32((const uint8_t*)style, (float*)c->img_s.p, ns, c->stream));
  *img_c = (const float*)c->img_c.p; *img_s = (const float*)c->img_s.p;
  return WCT_OK;
}

// The per-channel sums and the largest value of every tap come out of the epilogue that writes it (16-pixel unit sums,
// ConvArgs::usum): the transform's statistics pass then reads 1/16 of the feature bytes.  Needs a feature width that is
// a multiple of 16; other widths (and WCT_FUSE_STATS=0) take the sums from the stored features -- the same bits.
static bool fuse_stats() {
  static const int on = getenv("WCT_FUSE_STATS") ? atoi(getenv("WCT_FUSE_STATS")) : 1;
  return on != 0;
}

// The content chain of a stylize call (model.py:77-101) on B contents img_c [B][Hc][Wc][3] fp32: per level the encoder pass with
// a tap (and its unit sums, umax row 0 -- its first umax_clear bytes cleared from level clear_from on), the transform, and the
// decoder into the ping-pong images; then the uint8 frames into out (wct.py:66-68).
// style_at(l, b, &hs, &ws): pair b's style features of relu<l>_1, hs x ws.  transform(i, l, C, h, w, st): level i (relu<l>_1,
// C channels) of the h x w contents in c->feat_c -> c->wct_out (fp16), st the content's unit sums.  WCT_FLAG_SWAP5 runs the
// style-swap at relu5_1 instead.  WCT_FLAG_CONTENT_COLORS: the last launch puts the frames' luminance on the colours of
// content_raw, the contents as the caller gave them ([B][Hc][Wc][3] on the device: uint8, or fp32 with WCT_FLAG_IMAGES_F32).
template <typename StyleAt, typename Transform>
static int stylize_levels(wct_ctx* c, const float* img_c, const void* content_raw, int B, int Hc, int Wc, const int* levels,
                          int n_levels, unsigned flags, size_t umax_clear, int clear_from, StyleAt&& style_at,
                          Transform&& transform, uint8_t* out) {
  unsigned* const umax_c = (unsigned*)c->umax.p;
  const float* cur = img_c;
  int H = Hc, W = Wc;
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i], C = LEVEL_C[l];
    int h, w;
    level_dims(H, W, l, &h, &w);
    TRY(ensure(c, c->feat_c, (size_t)B * h * w * C * 4));
    float* ctaps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ctaps[l] = (float*)c->feat_c.p;
    float* us_c[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned* um_c[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (fuse_stats() && w % 16 == 0) {
      TRY(ensure(c, c->usum_c, (size_t)B * h * (w / 16) * C * 4));
      us_c[l] = (float*)c->usum_c.p; um_c[l] = umax_c;
      if (i >= clear_from) HIP_TRY(hipMemsetAsync(umax_c, 0, umax_clear, c->stream));
    }
    WctFeatStats st = {};
    st.u[0] = us_c[l]; st.umax[0] = um_c[l];
    // level i>0 encodes clip(previous decoded, 0, 1) (model.py:86): the clamp is in the conv1_1 loader
    TRY(run_encoder(c, cur, B, H, W, i > 0, l, ctaps, us_c, um_c));
    TRY(ensure(c, c->wct_out, (size_t)B * h * w * C * 2));
    if (l == 5 && (flags & WCT_FLAG_SWAP5)) {
      // tf.case priority at relu5_1: swap5 > adain > wct (model.py:148-154); pairs one at a time
      int hs, ws;
      style_at(l, 0, &hs, &ws);
      ARG_CHECK(h >= c->ss_patch && w >= c->ss_patch && hs >= c->ss_patch && ws >= c->ss_patch);
      TRY(ensure(c, c->wct_ws, style_swap_workspace_bytes(C, h, w, hs, ws, c->ss_patch, c->ss_stride)));
      ProfScope ps(c, 7, 0, 0);
      for (int b = 0; b < B; ++b)
        TRY(launch_style_swap((float*)c->feat_c.p + (size_t)b * h * w * C, h, w, style_at(l, b, &hs, &ws), hs, ws, C, c->ss_alpha,
                              c->ss_patch, c->ss_stride, -1.f, (half_t*)c->wct_out.p + (size_t)b * h * w * C, nullptr,
                              c->wct_ws.p, c->wct_ws.cap, c->stream, c->eig_fail_dev));
    } else
      TRY(transform(i, l, C, h, w, st));
    const int scale = 1 << (l - 1);
    const int H2 = h * scale, W2 = w * scale;
    DevBuf& dst = c->img_t[i & 1];
    TRY(ensure(c, dst, (size_t)B * H2 * W2 * 3 * 4));
    TRY(run_decoder(c, l, (half_t*)c->wct_out.p, B, h, w, (float*)dst.p));
    cur = (float*)dst.p; H = H2; W = W2;
  }
  if (flags & WCT_FLAG_CONTENT_COLORS) {
    const int f32 = (flags & WCT_FLAG_IMAGES_F32) ? 1 : 0;
    ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 5 + (double)B * Hc * Wc * 3 * (f32 ? 4 : 1));
    return launch_content_colors_f32(cur, content_raw, f32, B, H, W, Hc, Wc, out, c->stream);
  }
  ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 5);
  return launch_f32_to_u8(cur, out, (size_t)B * H * W * 3, c->stream);
}

extern "C" int wct_stylize_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* style,
                                     int Hs, int Ws, int B, const int* levels, int n_levels, float alpha,
                                     unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && style && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32);
  HIP_TRY(hipSetDevice(c->device));
  int deepest, Ho, Wo;
  TRY(stylize_checks(c, Hc, Wc, &style, &Hs, &Ws, 1, levels, n_levels, &deepest, &Ho, &Wo));

  // WCT_FLAG_STYLE_SHARED: `style` is ONE image for all B pairs (a video with a fixed style); its encoder pass,
  // statistics and eigensystems are computed once per call instead of once per pair
  const int shared = (flags & WCT_FLAG_STYLE_SHARED) ? 1 : 0;
  const int Bs = shared ? 1 : B;
  const float *img_c, *img_s;
  TRY(images_f32(c, flags, content, (size_t)B * Hc * Wc * 3, style, (size_t)Bs * Hs * Ws * 3, &img_c, &img_s));
  const bool want_stats = fuse_stats();
  constexpr size_t UROW = 32 * UMAX_SLOTS;                           // words per row: 32 images
  TRY(ensure(c, c->umax, 7 * UROW * sizeof(unsigned)));
  unsigned* const umax_c = (unsigned*)c->umax.p;                    // row 0: content (per level), rows 1..5: style levels
  if (want_stats) HIP_TRY(hipMemsetAsync(c->umax.p, 0, 7 * UROW * sizeof(unsigned), c->stream));
  // ONE style pass with a tap per requested level (model.py:69-75)
  float* taps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float* us_s[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  unsigned* um_s[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i];
    int h, w;
    level_dims(Hs, Ws, l, &h, &w);
    TRY(ensure(c, c->feat_s[l], (size_t)Bs * h * w * LEVEL_C[l] * 4));
    taps[l] = (float*)c->feat_s[l].p;
    if (want_stats && w % 16 == 0) {
      TRY(ensure(c, c->usum_s[l], (size_t)Bs * h * (w / 16) * LEVEL_C[l] * 4));
      us_s[l] = (float*)c->usum_s[l].p; um_s[l] = umax_c + UROW * l;
    }
  }
  TRY(run_encoder(c, img_s, Bs, Hs, Ws, 0, deepest, taps, us_s, um_s));

  // the content chain; its umax row was cleared with the others for level 0
  auto style_at = [&](int l, int b, int* hs, int* ws) {
    level_dims(Hs, Ws, l, hs, ws);
    return (const float*)c->feat_s[l].p + (size_t)(shared ? 0 : b) * *hs * *ws * LEVEL_C[l];
  };
  return stylize_levels(c, img_c, content, B, Hc, Wc, levels, n_levels, flags, UROW * sizeof(unsigned), 1, style_at,
                        [&](int, int l, int C, int h, int w, WctFeatStats st) {
                          int hs, ws;
                          const float* fs = style_at(l, 0, &hs, &ws);
                          st.u[1] = us_s[l]; st.umax[1] = um_s[l];
                          return run_transform(c, (float*)c->feat_c.p, h * w, fs, hs * ws, C, B, alpha, flags, -1.f,
                                               (half_t*)c->wct_out.p, nullptr, nullptr, &st);
                        }, out);
}

extern "C" int wct_stylize(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* style, int Hs, int Ws,
                           const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && style && out);
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));
  void *dc, *ds;
  const size_t px = (flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1;       // bytes per colour sample of the inputs
  TRY(stage_in(c, 0, content, (size_t)Hc * Wc * 3 * px, &dc));
  TRY(stage_in(c, 1, style, (size_t)Hs * Ws * 3 * px, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  TRY(wct_stylize_batch_dev(c, (uint8_t*)dc, Hc, Wc, (uint8_t*)ds, Hs, Ws, 1, levels, n_levels, alpha, flags,
                            (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

// The body of wct_stylize_mix / wct_stylize_masked (their checks done): the style encoder runs once per style (sizes may differ),
// then the content chain with B = 1, `level_transform` in the place of the single-style transform.
// level_transform(i, l, C, h, w, fs, Ns, st): stylize_levels' transform, fs[k] / Ns[k] style k's features of the level.
// WCT_FLAG_SWAP5 (K = 1) runs wct_stylize's style-swap at relu5_1 instead.
template <typename LevelTransform>
static int stylize_multi(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* const* styles, const int* Hs,
                         const int* Ws, int K, const int* levels, int n_levels, unsigned flags, uint8_t* out,
                         LevelTransform&& level_transform) {
  HIP_TRY(hipSetDevice(c->device));
  int deepest, Ho, Wo;
  TRY(stylize_checks(c, Hc, Wc, styles, Hs, Ws, K, levels, n_levels, &deepest, &Ho, &Wo));
  TRY(eig_stale(c));
  // inputs: the content in stage 0, the K styles back to back in mix_in
  const size_t px = (flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1;
  size_t ns_tot = 0, soff[WCT_MIX_MAX];
  for (int k = 0; k < K; ++k) { soff[k] = ns_tot; ns_tot += (size_t)Hs[k] * Ws[k] * 3; }
  const size_t nc = (size_t)Hc * Wc * 3;
  void* dc;
  TRY(stage_in(c, 0, content, nc * px, &dc));
  TRY(ensure(c, c->mix_in, ns_tot * px));
  for (int k = 0; k < K; ++k)
    HIP_TRY(hipMemcpyAsync((char*)c->mix_in.p + soff[k] * px, styles[k], (size_t)Hs[k] * Ws[k] * 3 * px, hipMemcpyHostToDevice, c->stream));
  const float *img_c, *img_s;
  TRY(images_f32(c, flags, dc, nc, c->mix_in.p, ns_tot, &img_c, &img_s));

  // one style pass per style, a tap per requested level (model.py:69-75); style k's map of level l at feat_mix[l] + foff[l][k]
  // (statistics from the stored features: the same bits as the epilogue's unit sums, colsum_kernel)
  size_t foff[6][WCT_MIX_MAX];
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i];
    size_t tot = 0;
    for (int k = 0; k < K; ++k) {
      int h, w;
      level_dims(Hs[k], Ws[k], l, &h, &w);
      foff[l][k] = tot;
      tot += (size_t)h * w * LEVEL_C[l];
    }
    TRY(ensure(c, c->feat_mix[l], tot * 4));
  }
  for (int k = 0; k < K; ++k) {
    float* taps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < n_levels; ++i) taps[levels[i]] = (float*)c->feat_mix[levels[i]].p + foff[levels[i]][k];
    TRY(run_encoder(c, img_s + soff[k], 1, Hs[k], Ws[k], 0, deepest, taps));
  }

  // the content chain, B = 1: pair k is style k (the style-swap takes K = 1); its umax row is cleared at every level
  TRY(ensure(c, c->umax, 32 * UMAX_SLOTS * sizeof(unsigned)));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  auto style_at = [&](int l, int k, int* hs, int* ws) {
    level_dims(Hs[k], Ws[k], l, hs, ws);
    return (const float*)c->feat_mix[l].p + foff[l][k];
  };
  TRY(stylize_levels(c, img_c, dc, 1, Hc, Wc, levels, n_levels, flags, UMAX_SLOTS * sizeof(unsigned), 0, style_at,
                     [&](int i, int l, int C, int h, int w, const WctFeatStats& st) {
                       const float* fs[WCT_MIX_MAX];
                       int Ns[WCT_MIX_MAX];
                       for (int k = 0; k < K; ++k) {
                         int hs, ws;
                         fs[k] = style_at(l, k, &hs, &ws);
                         Ns[k] = hs * ws;
                       }
                       return level_transform(i, l, C, h, w, fs, Ns, &st);
                     }, (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

// One predict() with a style mix at every level (Li et al. 2017, sec. 4.2): stylize_multi with the mix in the place of the
// single-style transform.
extern "C" int wct_stylize_mix(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* const* styles, const int* Hs,
                               const int* Ws, int K, const float* weights, const int* levels, int n_levels, float alpha,
                               unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && styles && Hs && Ws && out && levels && n_levels >= 1 && n_levels <= 16);
  float lambda[WCT_MIX_MAX];
  TRY(mix_weights(weights, K, lambda));
  if ((flags & WCT_FLAG_SWAP5) && K > 1) {
    wct_set_error("style mix: WCT_FLAG_SWAP5 needs K = 1 (style-swap is not linear in the style; got K = %d)", K);
    return WCT_ERR_ARG;
  }
  if (flags & WCT_FLAG_STYLE_SHARED) { wct_set_error("style mix: WCT_FLAG_STYLE_SHARED is for wct_stylize_batch_dev"); return WCT_ERR_ARG; }
  return stylize_multi(c, content, Hc, Wc, styles, Hs, Ws, K, levels, n_levels, flags, out,
                       [&](int, int, int C, int h, int w, const float* const* fs, const int* Ns, const WctFeatStats* st) {
                         return run_transform_mix(c, (float*)c->feat_c.p, h * w, fs, Ns, K, lambda, C, alpha, flags, -1.f,
                                                  (half_t*)c->wct_out.p, nullptr, nullptr, st);
                       });
}

// One predict() with spatial control at every level (Li et al. 2017, sec. 4.2, Fig. 7): stylize_multi with the masked transform
// in the place of the single-style transform.  The labels of every level are counted here, once, before any launch.
extern "C" int wct_stylize_masked(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* mask, const uint8_t* const* styles,
                                  const int* Hs, const int* Ws, int K, const int* levels, int n_levels, float alpha, unsigned flags,
                                  uint8_t* out) {
  ARG_CHECK(c && content && mask && styles && Hs && Ws && out && levels && n_levels >= 1 && n_levels <= 16 && Hc >= 2 && Wc >= 2);
  TRY(mask_check(mask, (size_t)Hc * Wc, K));
  if ((flags & WCT_FLAG_SWAP5) && K > 1) {
    wct_set_error("mask: WCT_FLAG_SWAP5 needs K = 1 (style-swap is not a per-region affine map; got K = %d)", K);
    return WCT_ERR_ARG;
  }
  if (flags & WCT_FLAG_STYLE_SHARED) { wct_set_error("mask: WCT_FLAG_STYLE_SHARED is for wct_stylize_batch_dev"); return WCT_ERR_ARG; }
  std::vector<int> nk((size_t)n_levels * WCT_MIX_MAX);
  int H = Hc, W = Wc;
  for (int i = 0; i < n_levels; ++i) {                   // the geometry of the content chain (wct_output_size)
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    int h, w;
    level_dims(H, W, levels[i], &h, &w);
    mask_counts(mask, Hc, Wc, h, w, 1 << (levels[i] - 1), K, &nk[(size_t)i * WCT_MIX_MAX]);
    H = h << (levels[i] - 1); W = w << (levels[i] - 1);
  }
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->mask_in, (size_t)Hc * Wc));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, mask, (size_t)Hc * Wc, hipMemcpyHostToDevice, c->stream));
  return stylize_multi(c, content, Hc, Wc, styles, Hs, Ws, K, levels, n_levels, flags, out,
                       [&](int i, int l, int C, int h, int w, const float* const* fs, const int* Ns, const WctFeatStats*) {
                         const MaskGeom g = {(const uint8_t*)c->mask_in.p, Hc, Wc, w, 1 << (l - 1)};
                         return run_transform_masked(c, (float*)c->feat_c.p, h * w, g, &nk[(size_t)i * WCT_MIX_MAX], fs, Ns, K, C,
                                                     alpha, flags, -1.f, (half_t*)c->wct_out.p, nullptr, nullptr);
                       });
}

// ---------------------------------------------------------------------------
// prepared styles: the style side once, any number of contents (wct.py:70-106 / stylize_video.py:88-121 with a fixed style)
// ---------------------------------------------------------------------------
static int style_live(const wct_ctx* c, const wct_style* st) {
  if (st && std::find(c->styles.begin(), c->styles.end(), st) != c->styles.end()) return WCT_OK;
  wct_set_error("prepared style %p is not a live handle of this context (freed, or prepared by another context)", (const void*)st);
  return WCT_ERR_STATE;
}

static StyleState* state_find(wct_style* st, int level, const WctStyleKey& key, int kind) {
  for (auto& e : st->cache[level])
    if (e.kind == kind && e.key.nslab == key.nslab && e.key.nsplit == key.nsplit && e.key.ksplit == key.ksplit) return &e;
  return nullptr;
}

struct StyleNeed { int level; WctStyleKey key; int kind; };

// Computes the states `needs` of a handle (none of them cached) on the ctx stream: ONE encoder pass of the style with a tap per
// level needed, then launch_style_state per state.  Blocking, and the eigensolves are checked before a state is kept: on
// WCT_ERR_NOCONV (or any error) none of them stays in the cache.
static int style_fill(wct_ctx* c, wct_style* st, const std::vector<StyleNeed>& needs) {
  if (needs.empty()) return WCT_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));               // (a state evicted below may belong to frames still in flight)
  int deepest = 0;
  float* taps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (const StyleNeed& n : needs) {
    int h, w;
    level_dims(st->Hs, st->Ws, n.level, &h, &w);
    TRY(ensure(c, c->feat_s[n.level], (size_t)h * w * LEVEL_C[n.level] * 4));
    taps[n.level] = (float*)c->feat_s[n.level].p;
    deepest = std::max(deepest, n.level);
  }
  TRY(run_encoder(c, st->img, 1, st->Hs, st->Ws, 0, deepest, taps));
  std::vector<float*> fresh;
  int rc = WCT_OK;
  for (const StyleNeed& n : needs) {
    const int C = LEVEL_C[n.level];
    int h, w;
    level_dims(st->Hs, st->Ws, n.level, &h, &w);
    auto& lv = st->cache[n.level];
    float* buf = nullptr;
    if ((int)lv.size() >= STYLE_CACHE_KEYS) {            // the oldest state that this call does not use makes room
      int old = -1;
      for (int i = 0; i < (int)lv.size(); ++i)
        if (lv[i].stamp != c->style_clock && (old < 0 || lv[i].stamp < lv[old].stamp)) old = i;
      if (old >= 0) { buf = lv[old].buf; lv.erase(lv.begin() + old); }
    }
    if (!buf && hipMalloc((void**)&buf, wct_style_state_floats(C) * sizeof(float)) != hipSuccess) {
      wct_set_error("hipMalloc failed (prepared style state, relu%d_1)", n.level);
      rc = WCT_ERR_NOMEM;
      break;
    }
    lv.push_back(StyleState{n.key, n.kind, buf, c->style_clock});
    fresh.push_back(buf);
    if (hipMemsetAsync(buf, 0, wct_style_state_floats(C) * sizeof(float), c->stream) != hipSuccess) { wct_set_error("hipMemsetAsync failed"); rc = WCT_ERR_HIP; break; }
    if ((rc = ensure(c, c->wct_ws, wct_style_workspace_bytes(C, h * w, n.key)))) break;
    ProfScope ps(c, n.kind == 2 ? 7 : 5, 0, 0);
    if ((rc = launch_style_state(taps[n.level], h * w, C, n.key, n.kind == 2, n.kind == 1 ? WCT_MODE_NP : WCT_MODE_TF, -1.f, c->wct_ws.p,
                                 c->wct_ws.cap, c->eig_fail_dev, c->stream, buf)))
      break;
  }
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { wct_set_error("hipStreamSynchronize failed (prepared style)"); rc = WCT_ERR_HIP; }
  if (!rc) rc = eig_status(c);
  if (rc) {                                               // keep nothing of a failed fill
    hipStreamSynchronize(c->stream);
    for (auto& lv : st->cache)
      for (size_t i = lv.size(); i-- > 0;)
        if (std::find(fresh.begin(), fresh.end(), lv[i].buf) != fresh.end()) { hipFree(lv[i].buf); lv.erase(lv.begin() + i); }
  }
  return rc;
}

static int style_kind(unsigned flags) { return (flags & WCT_FLAG_ADAIN) ? 2 : ((flags & WCT_FLAG_MODE_NP) ? 1 : 0); }

static int style_flags_ok(unsigned flags) {
  if (flags & WCT_FLAG_SWAP5) {
    wct_set_error("prepared style: WCT_FLAG_SWAP5 needs the style's relu5_1 map and patches, which a handle does not hold");
    return WCT_ERR_ARG;
  }
  if (flags & WCT_FLAG_STYLE_SHARED) { wct_set_error("prepared style: WCT_FLAG_STYLE_SHARED is for wct_stylize_batch_dev"); return WCT_ERR_ARG; }
  return WCT_OK;
}

extern "C" int wct_style_prepare(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const int* levels, int n_levels, unsigned flags,
                                 wct_style** out) {
  ARG_CHECK(c && style && levels && out && n_levels >= 1 && n_levels <= 16 && Hs >= 2 && Ws >= 2);
  *out = nullptr;
  TRY(style_flags_ok(flags));
  unsigned set = 0;
  int deepest = 0;
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    set |= 1u << levels[i];
    deepest = std::max(deepest, levels[i]);
  }
  TRY(check_min_size("style", Hs, Ws, deepest));
  if (!c->enc_loaded) { wct_set_error("encoder weights not set (wct_set_encoder)"); return WCT_ERR_STATE; }
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  struct Guard { wct_style* st; ~Guard() { free_style(st); } } g = {new wct_style()};
  wct_style* st = g.st;
  st->Hs = Hs; st->Ws = Ws; st->level_set = set;
  const size_t n = (size_t)Hs * Ws * 3;
  HIP_TRY(hipMalloc((void**)&st->img, n * sizeof(float)));
  void* ds;
  TRY(stage_in(c, 1, style, n * ((flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1), &ds));
  if (flags & WCT_FLAG_IMAGES_F32) HIP_TRY(hipMemcpyAsync(st->img, ds, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  else TRY(launch_u8_to_f32((const uint8_t*)ds, st->img, n, c->stream));
  // the states of "a content as large as the style", in the mode the flags name; every other key on first use
  ++c->style_clock;
  std::vector<StyleNeed> needs;
  for (int l = 1; l <= 5; ++l) {
    if (!(set & (1u << l))) continue;
    int h, w;
    level_dims(Hs, Ws, l, &h, &w);
    needs.push_back(StyleNeed{l, wct_style_key(LEVEL_C[l], h * w, h * w), style_kind(flags)});
  }
  TRY(style_fill(c, st, needs));
  c->styles.push_back(st);
  g.st = nullptr;
  *out = st;
  return WCT_OK;
}

extern "C" void wct_style_free(wct_ctx* c, wct_style* st) {
  if (!c || !st) return;
  auto it = std::find(c->styles.begin(), c->styles.end(), st);
  if (it == c->styles.end()) return;                      // not ours, or freed already
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);                        // frames in flight may still read its states
  c->styles.erase(it);
  free_style(st);
}

// The body of the wct_stylize_prepared* calls (their pointer and flag checks done): B contents [B][Hc][Wc][3] on the device, K
// handles; lambda null: one style for all B (K = 1), else the mix weights of K styles (B = 1).  Asynchronous unless a handle
// has to compute a state (style_fill), which happens before anything of the content chain is enqueued.
static int warm_live(const wct_ctx* c, const wct_warm* wm);
static int stylize_prepared_dev(wct_ctx* c, const void* content, int Hc, int Wc, int B, const wct_style* const* styles, int K,
                                const float* lambda, const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out,
                                wct_warm* warm = nullptr /* with one style (lambda null): start the content solves from it */) {
  HIP_TRY(hipSetDevice(c->device));
  for (int k = 0; k < K; ++k) TRY(style_live(c, styles[k]));
  if (warm) {
    TRY(warm_live(c, warm));
    if (flags & WCT_FLAG_ADAIN) { wct_set_error("warm start: WCT_FLAG_ADAIN has no eigensolve to start"); return WCT_ERR_ARG; }
    unsigned set = 0;
    for (int i = 0; i < n_levels; ++i) { ARG_CHECK(levels[i] >= 1 && levels[i] <= 5); set |= 1u << levels[i]; }
    if (set != warm->level_set) {
      wct_set_error("warm start: the levels of the call (set 0x%x) are not the levels the state was created for (0x%x)", set, warm->level_set);
      return WCT_ERR_ARG;
    }
  }
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    for (int k = 0; k < K; ++k)
      if (!(styles[k]->level_set & (1u << levels[i]))) {
        wct_set_error("prepared style %d was not prepared for relu%d_1", k, levels[i]);
        return WCT_ERR_ARG;
      }
    if (!c->dec[levels[i]].loaded) { wct_set_error("decoder weights for relu%d_1 not set", levels[i]); return WCT_ERR_STATE; }
  }
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));

  // the states of every level, before any launch of the content chain: style k serves the layout of (content, style k)
  const int kind = style_kind(flags);
  ++c->style_clock;
  std::vector<WctStyleRef> refs(n_levels);
  std::vector<int> ns((size_t)n_levels * WCT_MIX_MAX);
  for (int k = 0; k < K; ++k) {
    wct_style* st = const_cast<wct_style*>(styles[k]);
    std::vector<StyleNeed> all, missing;
    int H = Hc, W = Wc;
    for (int i = 0; i < n_levels; ++i) {
      const int l = levels[i];
      int h, w, hs, ws;
      level_dims(H, W, l, &h, &w);
      level_dims(st->Hs, st->Ws, l, &hs, &ws);
      ns[(size_t)i * WCT_MIX_MAX + k] = hs * ws;
      const StyleNeed n = {l, wct_style_key(LEVEL_C[l], h * w, hs * ws), kind};
      all.push_back(n);
      StyleState* e = state_find(st, l, n.key, kind);
      if (e) e->stamp = c->style_clock;
      else if (std::none_of(missing.begin(), missing.end(), [&](const StyleNeed& m) {
                 return m.level == l && m.key.nslab == n.key.nslab && m.key.nsplit == n.key.nsplit && m.key.ksplit == n.key.ksplit; }))
        missing.push_back(n);
      H = h << (l - 1); W = w << (l - 1);
    }
    TRY(style_fill(c, st, missing));
    for (int i = 0; i < n_levels; ++i) {
      StyleState* e = state_find(st, all[i].level, all[i].key, kind);
      if (!e) { wct_set_error("prepared style %d: the state of relu%d_1 is gone", k, all[i].level); return WCT_ERR_STATE; }
      refs[i].state[k] = e->buf;
    }
  }

  const float* img_c = (const float*)content;
  const size_t nc = (size_t)B * Hc * Wc * 3;
  if (!(flags & WCT_FLAG_IMAGES_F32)) {
    TRY(ensure(c, c->img_c, nc * 4));
    ProfScope ps(c, 7, 0, (double)nc * 5);
    TRY(launch_u8_to_f32((const uint8_t*)content, (float*)c->img_c.p, nc, c->stream));
    img_c = (const float*)c->img_c.p;
  }
  constexpr size_t UROW = 32 * UMAX_SLOTS;                           // (the content's row of wct_stylize_batch_dev)
  TRY(ensure(c, c->umax, 7 * UROW * sizeof(unsigned)));
  if (fuse_stats()) HIP_TRY(hipMemsetAsync(c->umax.p, 0, UROW * sizeof(unsigned), c->stream));
  auto no_style = [](int, int, int* hs, int* ws) { *hs = *ws = 0; return (const float*)nullptr; };     // (style-swap alone asks)
  if (warm && std::find(c->warm_used.begin(), c->warm_used.end(), warm) == c->warm_used.end()) c->warm_used.push_back(warm);
  return stylize_levels(c, img_c, content, B, Hc, Wc, levels, n_levels, flags, UROW * sizeof(unsigned), 1, no_style,
                        [&](int i, int l, int C, int h, int w, const WctFeatStats& st) {
                          const int* Ns = &ns[(size_t)i * WCT_MIX_MAX];
                          if (!lambda && warm) {
                            const WctWarmRef wr = {warm->basis[l], warm->valid[l] ? 1 : 0};
                            TRY(run_transform(c, (float*)c->feat_c.p, h * w, nullptr, Ns[0], C, B, alpha, flags, -1.f,
                                              (half_t*)c->wct_out.p, nullptr, nullptr, &st, &refs[i], &wr));
                            warm->valid[l] = true;              // (the basis of frame B - 1 is enqueued)
                            return (int)WCT_OK;
                          }
                          if (!lambda)
                            return run_transform(c, (float*)c->feat_c.p, h * w, nullptr, Ns[0], C, B, alpha, flags, -1.f,
                                                 (half_t*)c->wct_out.p, nullptr, nullptr, &st, &refs[i]);
                          return run_transform_mix(c, (float*)c->feat_c.p, h * w, nullptr, Ns, K, lambda, C, alpha, flags, -1.f,
                                                   (half_t*)c->wct_out.p, nullptr, nullptr, &st, &refs[i]);
                        }, out);
}

// host content in, host frame out, around stylize_prepared_dev (B = 1)
static int stylize_prepared_host(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* const* styles, int K,
                                 const float* lambda, const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out,
                                 wct_warm* warm = nullptr) {
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));
  void* dc;
  TRY(stage_in(c, 0, content, (size_t)Hc * Wc * 3 * ((flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1), &dc));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  TRY(stylize_prepared_dev(c, dc, Hc, Wc, 1, styles, K, lambda, levels, n_levels, alpha, flags, (uint8_t*)c->stage[2].p, warm));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

extern "C" int wct_stylize_prepared(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                    int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16);
  TRY(style_flags_ok(flags));
  return stylize_prepared_host(c, content, Hc, Wc, &style, 1, nullptr, levels, n_levels, alpha, flags, out);
}

extern "C" int wct_stylize_prepared_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const wct_style* style,
                                              const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32);
  TRY(style_flags_ok(flags));
  return stylize_prepared_dev(c, content, Hc, Wc, B, &style, 1, nullptr, levels, n_levels, alpha, flags, out);
}

extern "C" int wct_stylize_prepared_mix(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* const* styles, int K,
                                        const float* weights, const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && styles && out && levels && n_levels >= 1 && n_levels <= 16);
  float lambda[WCT_MIX_MAX];
  TRY(mix_weights(weights, K, lambda));
  TRY(style_flags_ok(flags));
  return stylize_prepared_host(c, content, Hc, Wc, styles, K, lambda, levels, n_levels, alpha, flags, out);
}

// ---------------------------------------------------------------------------
// video warm start (stylize_video.py:112-135 calls predict() per frame and solves every content covariance from scratch): the
// content eigensolves of a call start from the eigenvectors of the previous call's last frame (csrc/warm.hip)
// ---------------------------------------------------------------------------
static int warm_live(const wct_ctx* c, const wct_warm* wm) {
  if (wm && std::find(c->warms.begin(), c->warms.end(), wm) != c->warms.end()) return WCT_OK;
  wct_set_error("warm state %p is not a live state of this context (freed, or created by another context)", (const void*)wm);
  return WCT_ERR_STATE;
}

extern "C" int wct_warm_create(wct_ctx* c, const int* levels, int n_levels, wct_warm** out) {
  ARG_CHECK(c && levels && out && n_levels >= 1 && n_levels <= 16);
  *out = nullptr;
  for (int i = 0; i < n_levels; ++i) ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
  HIP_TRY(hipSetDevice(c->device));
  struct Guard { wct_warm* wm; ~Guard() { free_warm(wm); } } g = {new wct_warm()};
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i];
    if (g.wm->basis[l]) continue;
    g.wm->level_set |= 1u << l;
    if (hipMalloc((void**)&g.wm->basis[l], (size_t)LEVEL_C[l] * LEVEL_C[l] * sizeof(float)) != hipSuccess) {
      wct_set_error("hipMalloc failed (warm state, relu%d_1)", l);
      return WCT_ERR_NOMEM;
    }
  }
  c->warms.push_back(g.wm);
  *out = g.wm;
  g.wm = nullptr;
  return WCT_OK;
}

extern "C" void wct_warm_free(wct_ctx* c, wct_warm* wm) {
  if (!c || !wm) return;
  auto it = std::find(c->warms.begin(), c->warms.end(), wm);
  if (it == c->warms.end()) return;                       // not ours, or freed already
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);                        // frames in flight may still read its bases
  c->warms.erase(it);
  c->warm_used.erase(std::remove(c->warm_used.begin(), c->warm_used.end(), wm), c->warm_used.end());
  free_warm(wm);
}

extern "C" int wct_warm_reset(wct_ctx* c, wct_warm* wm) {
  ARG_CHECK(c != nullptr);
  TRY(warm_live(c, wm));
  for (bool& v : wm->valid) v = false;
  return WCT_OK;
}

extern "C" int wct_warm_basis(wct_ctx* c, const wct_warm* wm, int level, int* valid, float* V_host) {
  ARG_CHECK(c && valid);
  TRY(warm_live(c, wm));
  if (level < 1 || level > 5 || !(wm->level_set & (1u << level))) {
    wct_set_error("warm state: relu%d_1 is not in the state's level set", level);
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *valid = wm->valid[level] ? 1 : 0;
  if (V_host && wm->valid[level]) TRY(fetch(c, V_host, wm->basis[level], (size_t)LEVEL_C[level] * LEVEL_C[level] * sizeof(float)));
  return WCT_OK;
}

extern "C" int wct_stylize_prepared_warm(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                         int n_levels, float alpha, unsigned flags, wct_warm* warm, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16);
  TRY(style_flags_ok(flags));
  TRY(warm_live(c, warm));
  return stylize_prepared_host(c, content, Hc, Wc, &style, 1, nullptr, levels, n_levels, alpha, flags, out, warm);
}

extern "C" int wct_stylize_prepared_batch_dev_warm(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const wct_style* style,
                                                   const int* levels, int n_levels, float alpha, unsigned flags, wct_warm* warm,
                                                   uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32);
  TRY(style_flags_ok(flags));
  TRY(warm_live(c, warm));
  return stylize_prepared_dev(c, content, Hc, Wc, B, &style, 1, nullptr, levels, n_levels, alpha, flags, out, warm);
}

// the op-level twin of wct_transform: one (content, style) pair of feature matrices, the content solve started from the
// state's basis of `level`
extern "C" int wct_transform_warm(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C, float alpha,
                                  unsigned flags, wct_warm* warm, int level, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out);
  TRY(warm_live(c, warm));
  if (flags & (WCT_FLAG_ADAIN | WCT_FLAG_SWAP5 | WCT_FLAG_STYLE_SHARED | WCT_FLAG_IMAGES_F32 | WCT_FLAG_CONTENT_COLORS)) {
    wct_set_error("wct_transform_warm: the flags take WCT_FLAG_MODE_NP alone (AdaIN has no eigensolve, style-swap no warm start)");
    return WCT_ERR_ARG;
  }
  if (level < 1 || level > 5 || !(warm->level_set & (1u << level))) {
    wct_set_error("warm state: relu%d_1 is not in the state's level set", level);
    return WCT_ERR_ARG;
  }
  if (C != LEVEL_C[level]) {
    wct_set_error("warm state: relu%d_1 has %d channels, the features have %d", level, LEVEL_C[level], C);
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->stage[3], 256));
  c->warm_used.push_back(warm);
  const WctWarmRef wr = {warm->basis[level], warm->valid[level] ? 1 : 0};
  TRY(run_transform(c, (float*)dc, Nc, (float*)ds, Ns, C, 1, alpha, flags, -1.f, nullptr, (float*)c->stage[2].p, (int*)c->stage[3].p,
                    nullptr, nullptr, &wr));
  warm->valid[level] = true;
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) TRY(fetch(c, sweeps_out, c->stage[3].p, 2 * sizeof(int)));
  return eig_status(c);
}

// Spatial control of B frames on prepared styles: one label map per frame (on the HOST: every level's labels are counted here,
// before any launch, and size the launches), K handles shared by all frames.  The level transform runs the frames in GROUPS of at
// most WCT_PLAN_PAIRS = 32 live (frame, region) pairs -- one batched eigensolve of 64 slots, the style slots dead -- through
// launch_wct_masked_batch; a matrix's eigensystem does not depend on its batch, so the grouping does not show in the frames.
// Pair (f, k) takes handle k's state under wct_style_key(C, N_fk, Ns_k); the missing ones are filled in front of the content
// chain (style_fill), and a state the running call uses is never evicted (its stamp is the call's), so a level's cache holds
// as many keys as the call with the most distinct region sizes needed (at least STYLE_CACHE_KEYS, at most B per label).
static int stylize_prepared_masked_dev(wct_ctx* c, const void* content, int Hc, int Wc, int B, const uint8_t* masks,
                                       const wct_style* const* styles, int K, const int* levels, int n_levels, float alpha,
                                       unsigned flags, uint8_t* out) {
  HIP_TRY(hipSetDevice(c->device));
  if (K < 1 || K > WCT_MIX_MAX) { wct_set_error("mask: K = %d styles, must be 1 .. %d", K, (int)WCT_MIX_MAX); return WCT_ERR_ARG; }
  for (int k = 0; k < K; ++k) TRY(style_live(c, styles[k]));
  TRY(mask_check(masks, (size_t)B * Hc * Wc, K));
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    for (int k = 0; k < K; ++k)
      if (!(styles[k]->level_set & (1u << levels[i]))) {
        wct_set_error("prepared style %d was not prepared for relu%d_1", k, levels[i]);
        return WCT_ERR_ARG;
      }
    if (!c->dec[levels[i]].loaded) { wct_set_error("decoder weights for relu%d_1 not set", levels[i]); return WCT_ERR_STATE; }
  }
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));

  // the labels of every level and frame, counted on the host: nk [level][frame][WCT_MIX_MAX]
  const size_t fstride = (size_t)B * WCT_MIX_MAX;
  std::vector<int> nk((size_t)n_levels * fstride), ns((size_t)n_levels * WCT_MIX_MAX);
  {
    int H = Hc, W = Wc;
    for (int i = 0; i < n_levels; ++i) {
      const int l = levels[i];
      int h, w;
      level_dims(H, W, l, &h, &w);
      for (int f = 0; f < B; ++f)
        mask_counts(masks + (size_t)f * Hc * Wc, Hc, Wc, h, w, 1 << (l - 1), K, &nk[i * fstride + (size_t)f * WCT_MIX_MAX]);
      for (int k = 0; k < K; ++k) {
        int hs, ws;
        level_dims(styles[k]->Hs, styles[k]->Ws, l, &hs, &ws);
        ns[(size_t)i * WCT_MIX_MAX + k] = hs * ws;
      }
      H = h << (l - 1); W = w << (l - 1);
    }
  }

  // the states of every live (level, frame, region), before any launch of the content chain
  const int kind = style_kind(flags);
  ++c->style_clock;
  auto same_key = [](const WctStyleKey& a, const WctStyleKey& b) { return a.nslab == b.nslab && a.nsplit == b.nsplit && a.ksplit == b.ksplit; };
  auto key_of = [&](int i, int f, int k) {
    return wct_style_key(LEVEL_C[levels[i]], nk[i * fstride + (size_t)f * WCT_MIX_MAX + k], ns[(size_t)i * WCT_MIX_MAX + k]);
  };
  for (int k = 0; k < K; ++k) {
    wct_style* st = const_cast<wct_style*>(styles[k]);
    std::vector<StyleNeed> missing;
    for (int i = 0; i < n_levels; ++i)
      for (int f = 0; f < B; ++f) {
        if (nk[i * fstride + (size_t)f * WCT_MIX_MAX + k] < 2) continue;
        const StyleNeed n = {levels[i], key_of(i, f, k), kind};
        StyleState* e = state_find(st, n.level, n.key, kind);
        if (e) e->stamp = c->style_clock;
        else if (std::none_of(missing.begin(), missing.end(), [&](const StyleNeed& m) { return m.level == n.level && same_key(m.key, n.key); }))
          missing.push_back(n);
      }
    TRY(style_fill(c, st, missing));
  }
  std::vector<const float*> states((size_t)n_levels * fstride, nullptr);
  for (int i = 0; i < n_levels; ++i)
    for (int f = 0; f < B; ++f)
      for (int k = 0; k < K; ++k) {
        if (nk[i * fstride + (size_t)f * WCT_MIX_MAX + k] < 2) continue;
        StyleState* e = state_find(const_cast<wct_style*>(styles[k]), levels[i], key_of(i, f, k), kind);
        if (!e) { wct_set_error("prepared style %d: the state of relu%d_1 is gone", k, levels[i]); return WCT_ERR_STATE; }
        states[i * fstride + (size_t)f * WCT_MIX_MAX + k] = e->buf;
      }

  TRY(ensure(c, c->mask_in, (size_t)B * Hc * Wc));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, masks, (size_t)B * Hc * Wc, hipMemcpyHostToDevice, c->stream));
  const float* img_c = (const float*)content;
  const size_t nc = (size_t)B * Hc * Wc * 3;
  if (!(flags & WCT_FLAG_IMAGES_F32)) {
    TRY(ensure(c, c->img_c, nc * 4));
    ProfScope ps(c, 7, 0, (double)nc * 5);
    TRY(launch_u8_to_f32((const uint8_t*)content, (float*)c->img_c.p, nc, c->stream));
    img_c = (const float*)c->img_c.p;
  }
  constexpr size_t UROW = 32 * UMAX_SLOTS;
  TRY(ensure(c, c->umax, 7 * UROW * sizeof(unsigned)));
  if (fuse_stats()) HIP_TRY(hipMemsetAsync(c->umax.p, 0, UROW * sizeof(unsigned), c->stream));
  auto no_style = [](int, int, int* hs, int* ws) { *hs = *ws = 0; return (const float*)nullptr; };
  return stylize_levels(c, img_c, content, B, Hc, Wc, levels, n_levels, flags, UROW * sizeof(unsigned), 1, no_style,
                        [&](int i, int l, int C, int h, int w, const WctFeatStats&) {
                          const int Nc = h * w;
                          const int* Ns = &ns[(size_t)i * WCT_MIX_MAX];
                          for (int f0 = 0; f0 < B;) {                  // a group: frames f0 .. f1 - 1, at most WCT_PLAN_PAIRS pairs
                            const int* gnk = &nk[i * fstride + (size_t)f0 * WCT_MIX_MAX];
                            int f1 = f0 + 1;
                            while (f1 < B && wct_masked_batch_pairs(f1 + 1 - f0, gnk, K) <= 32) ++f1;
                            const int G = f1 - f0;
                            WctStyleSlots slots = {};
                            int P = 0;
                            for (int f = f0; f < f1; ++f)
                              for (int k = 0; k < K; ++k)
                                if (nk[i * fstride + (size_t)f * WCT_MIX_MAX + k] >= 2)
                                  slots.state[P++] = states[i * fstride + (size_t)f * WCT_MIX_MAX + k];
                            const MaskGeom g = {(const uint8_t*)c->mask_in.p + (size_t)f0 * Hc * Wc, Hc, Wc, w, 1 << (l - 1)};
                            const float* fc = (const float*)c->feat_c.p + (size_t)f0 * Nc * C;
                            half_t* o16 = (half_t*)c->wct_out.p + (size_t)f0 * Nc * C;
                            const double rows = (double)G * Nc;
                            // (the covariance stage is charged the compaction and gather as well; no style rows are read)
                            const StageCost cost = {2.0 * C * C * rows, 6.0 * rows * C * 4, 2.0 * C * C * rows + 6.0 * C * C * C * P,
                                                    rows * C * (4 + 2), 4.0 * rows * C * 4 + rows * C * 6};
                            TRY(run_stages(c, wct_masked_batch_workspace_bytes(C, Nc, G, gnk, Ns, K), flags, cost, [&](int mode, int stages) {
                              if (!stages)
                                return launch_adain_masked_batch(fc, Nc, G, g, gnk, Ns, K, slots, C, alpha, 1e-5f, o16, nullptr, c->wct_ws.p,
                                                                 c->wct_ws.cap, c->stream);
                              return launch_wct_masked_batch(fc, Nc, G, g, gnk, Ns, K, slots, C, alpha, mode, -1.f, o16, nullptr, c->wct_ws.p,
                                                             c->wct_ws.cap, stages, c->stream, c->eig_fail_dev);
                            }));
                            f0 = f1;
                          }
                          return (int)WCT_OK;
                        }, out);
}

static int prepared_masked_flags_ok(unsigned flags) {
  if (flags & WCT_FLAG_SWAP5) {
    wct_set_error("mask: WCT_FLAG_SWAP5 needs the style's relu5_1 map and patches, which a handle does not hold (and style-swap is "
                  "not a per-region affine map)");
    return WCT_ERR_ARG;
  }
  if (flags & WCT_FLAG_STYLE_SHARED) { wct_set_error("mask: WCT_FLAG_STYLE_SHARED is for wct_stylize_batch_dev"); return WCT_ERR_ARG; }
  return WCT_OK;
}

extern "C" int wct_stylize_prepared_masked_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const uint8_t* masks,
                                                     const wct_style* const* styles, int K, const int* levels, int n_levels,
                                                     float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && masks && styles && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32 && Hc >= 2 && Wc >= 2);
  TRY(prepared_masked_flags_ok(flags));
  return stylize_prepared_masked_dev(c, content, Hc, Wc, B, masks, styles, K, levels, n_levels, alpha, flags, out);
}

// host content in, host frame out: the B = 1 case of the batch call
extern "C" int wct_stylize_prepared_masked(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* mask,
                                           const wct_style* const* styles, int K, const int* levels, int n_levels, float alpha,
                                           unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && mask && styles && out && levels && n_levels >= 1 && n_levels <= 16 && Hc >= 2 && Wc >= 2);
  TRY(prepared_masked_flags_ok(flags));
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));
  void* dc;
  TRY(stage_in(c, 0, content, (size_t)Hc * Wc * 3 * ((flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1), &dc));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  TRY(stylize_prepared_masked_dev(c, dc, Hc, Wc, 1, mask, styles, K, levels, n_levels, alpha, flags, (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

// ---------------------------------------------------------------------------
// decoder training (model.py:123-223, train.py:129-196): one optimiser step
// ---------------------------------------------------------------------------
namespace {
struct TrainArena {
  char* base; size_t off;
  template <typename T> T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};
struct EncStep { int idx; int h, w; half_t* out; half_t* pooled; int ph, pw; };      // idx into enc[]; (h, w) conv dims
struct DecStep { int conv; int up; int h, w; const half_t* in; half_t* out; };       // (h, w) = conv output dims
}  // namespace

// Adam moments (zero) and the gradient arena of a decoder, allocated on first use.  Gradients of all layers live in
// one contiguous buffer ([w0][b0][w1][b1]..., every piece 64-float aligned) so that data-parallel training needs a
// single all-reduce per step (wct_train_grad_buffer).
static int ensure_train_state(wct_ctx* c, Decoder& d) {
  if (!d.mw.empty()) return WCT_OK;
  const int nconv = (int)d.w32.size();
  size_t total = 0;
  auto pad = [](size_t n) { return (n + 63) & ~(size_t)63; };
  for (int i = 0; i < nconv; ++i) total += pad((size_t)9 * d.cin[i] * d.cout[i]) + pad((size_t)d.cout[i]);
  HIP_TRY(hipMalloc((void**)&d.grad_arena, total * sizeof(float)));
  HIP_TRY(hipMemsetAsync(d.grad_arena, 0, total * sizeof(float), c->stream));
  d.grad_count = total;
  size_t off = 0;
  for (int i = 0; i < nconv; ++i) {
    const size_t nw = (size_t)9 * d.cin[i] * d.cout[i], nb = (size_t)d.cout[i];
    float* p[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[4] = {nw * 4, nw * 4, nb * 4, nb * 4};
    for (int k = 0; k < 4; ++k) { HIP_TRY(hipMalloc((void**)&p[k], bytes[k])); HIP_TRY(hipMemsetAsync(p[k], 0, bytes[k], c->stream)); }
    d.mw.push_back(p[0]); d.vw.push_back(p[1]); d.mb.push_back(p[2]); d.vb.push_back(p[3]);
    d.gw.push_back(d.grad_arena + off); off += pad(nw);
    d.gb.push_back(d.grad_arena + off); off += pad(nb);
  }
  return WCT_OK;
}

// Adam on every conv of the decoder from the gradients currently in the arena, then refresh the fp16 forward weights
static int apply_adam(wct_ctx* c, Decoder& d, float lr, float beta1, float beta2, float eps, int step) {
  hipStream_t s = c->stream;
  const float lr_t = lr * sqrtf(1.f - powf(beta2, (float)step)) / (1.f - powf(beta1, (float)step));
  int ci = 0;
  for (int i = 0; i < (int)d.w32.size(); ++i) {
    const size_t nw = (size_t)9 * d.cin[i] * d.cout[i];
    TRY(launch_adam(d.w32[i], d.mw[i], d.vw[i], d.gw[i], nw, lr_t, beta1, beta2, eps, s));
    TRY(launch_adam(d.b32[i], d.mb[i], d.vb[i], d.gb[i], (size_t)d.cout[i], lr_t, beta1, beta2, eps, s));
    if (d.cout[i] == 3) {
      TRY(launch_pack_last_frag(d.w32[i], d.last_w, s));
      HIP_TRY(hipMemcpyAsync(d.last_b, d.b32[i], 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
      ConvLayer& l = d.convs[ci++];
      TRY(launch_pack_conv_frag(d.w32[i], l.w, l.cin, l.cout, s));
      if (l.ww) TRY(launch_pack_conv_wino_frag(d.w32[i], l.ww, l.cin, l.cout, s));
      HIP_TRY(hipMemcpyAsync(l.b, d.b32[i], (size_t)l.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  }
  return WCT_OK;
}

// images: host fp32 [B][H][W][3] in [0,1] (train.py:72-83).  losses_out[4] = feature, pixel, tv, total (host).
// step = 1-based optimiser step (Adam bias correction); lr is the already decayed learning rate (model.py:17-19).
extern "C" int wct_train_step(wct_ctx* c, int level, const float* images, int B, int H, int W,
                              float feature_weight, float pixel_weight, float tv_weight,
                              float lr, float beta1, float beta2, float eps, int step, float* losses_out) {
  ARG_CHECK(c && images && losses_out && level >= 1 && level <= 5 && B >= 1 && B <= 64 && step >= 1);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->enc_loaded) { wct_set_error("encoder weights not set (wct_set_encoder)"); return WCT_ERR_STATE; }
  // every forward layer of a training step on the direct kernel: the backward pass differentiates THAT arithmetic (fp16-rounded
  // operands, exact products), and the gradient tests hold it to 1e-4
  struct DirectOnly { wct_ctx* c; DirectOnly(wct_ctx* x) : c(x) { c->no_wino = true; } ~DirectOnly() { c->no_wino = false; } } direct_only(c);
  Decoder& d = c->dec[level];
  if (!d.loaded) { wct_set_error("decoder weights for relu%d_1 not set (wct_set_decoder)", level); return WCT_ERR_STATE; }
  const int scale = 1 << (level - 1);
  ARG_CHECK(H % scale == 0 && W % scale == 0 && H / scale >= 2 && W / scale >= 2);   // the decoder returns exactly H x W
  hipStream_t s = c->stream;
  const int C = LEVEL_C[level];
  const int h = H / scale, w = W / scale;
  const int nconv = (int)d.w32.size();
  static const int seq_tap[12] = {0, 2, 0, 3, 0, 0, 0, 4, 0, 0, 0, 5};
  static const int pool_after[12] = {1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0};
  int tap_idx = -1;
  for (int i = 0; i < 12 && level > 1; ++i) if (seq_tap[i] == level) tap_idx = i;

  // optimiser state, allocated on first use
  TRY(ensure_train_state(c, d));

  // ---- carve the workspace (first pass sizes, second pass pointers)
  std::vector<EncStep> enc_steps;
  std::vector<DecStep> dec_steps;
  float *X = nullptr, *F = nullptr, *Fp = nullptr, *D = nullptr, *g0 = nullptr, *g1 = nullptr, *col = nullptr, *gp = nullptr,
        *partial = nullptr, *wt = nullptr, *dloss = nullptr;
  half_t *A0 = nullptr, *e0 = nullptr;
  double* lpart = nullptr;
  size_t total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) TRY(ensure(c, c->train_ws, total));
    TrainArena ar = {pass ? (char*)c->train_ws.p : nullptr, 0};
    enc_steps.clear(); dec_steps.clear();
    size_t gmax = (size_t)B * H * W * 64, colmax = 0, gpmax = 0, partmax = 256 * 512, wtmax = 0;
    X = ar.take<float>((size_t)B * H * W * 3);
    F = ar.take<float>((size_t)B * h * w * C);
    Fp = ar.take<float>((size_t)B * h * w * C);
    A0 = ar.take<half_t>((size_t)B * h * w * C);
    D = ar.take<float>((size_t)B * H * W * 3);
    // decoder activations
    {
      int hh = h, ww = w, up = 0, ci = 0;
      const half_t* cur = A0;
      for (auto& st : d.plan) {
        if (st.kind == 'U') { up = 1; hh *= 2; ww *= 2; continue; }
        half_t* out = st.cout == 3 ? nullptr : ar.take<half_t>((size_t)B * hh * ww * st.cout);
        dec_steps.push_back({ci, up, hh, ww, cur, out});
        const size_t px = (size_t)B * hh * ww, pxp = (size_t)B * (hh + 2) * (ww + 2);
        colmax = std::max(colmax, std::max(px * 9 * st.cin, pxp * 9 * st.cout));
        gpmax = std::max(gpmax, pxp * st.cin);
        gmax = std::max(gmax, std::max(px * st.cin, px * (size_t)std::max(st.cout, 4)));
        partmax = std::max(partmax, (size_t)conv_wgrad_splits(B, hh, ww) * 9 * st.cin * st.cout);
        wtmax = std::max(wtmax, (size_t)9 * st.cin * st.cout);
        cur = out; up = 0; ++ci;
      }
    }
    // encoder pass over the decoded image, every activation kept
    e0 = ar.take<half_t>((size_t)B * H * W * 64);
    {
      int hh = H, ww = W;
      colmax = std::max(colmax, (size_t)B * (hh + 2) * (ww + 2) * 9 * 64);
      gpmax = std::max(gpmax, (size_t)B * (hh + 2) * (ww + 2) * 64);
      for (int i = 0; i <= tap_idx; ++i) {
        const int cout = ENC_COUT[i], cin = ENC_CIN[i];
        EncStep es = {i, hh, ww, nullptr, nullptr, 0, 0};
        if (i != tap_idx) es.out = ar.take<half_t>((size_t)B * hh * ww * cout);
        const size_t pxp = (size_t)B * (hh + 2) * (ww + 2);
        colmax = std::max(colmax, pxp * 9 * cout);
        gpmax = std::max(gpmax, pxp * cin);
        gmax = std::max(gmax, (size_t)B * hh * ww * std::max(cin, cout));
        if (pool_after[i] && i != tap_idx) {
          es.ph = (hh + 1) / 2; es.pw = (ww + 1) / 2;
          es.pooled = ar.take<half_t>((size_t)B * es.ph * es.pw * cout);
          hh = es.ph; ww = es.pw;
        }
        enc_steps.push_back(es);
      }
    }
    g0 = ar.take<float>(gmax); g1 = ar.take<float>(gmax);
    col = ar.take<float>(colmax); gp = ar.take<float>(gpmax);
    partial = ar.take<float>(partmax); wt = ar.take<float>(wtmax);
    lpart = ar.take<double>(1024); dloss = ar.take<float>(16);      // 4 losses + scratch of the backward GEMMs
    total = ar.off;
  }

  // ---- forward
  HIP_TRY(hipMemcpyAsync(X, images, (size_t)B * H * W * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  {
    float* taps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    taps[level] = F;
    TRY(run_encoder(c, X, B, H, W, 0, level, taps));                       // content features (the target of the feature loss)
  }
  TRY(launch_f32_to_f16(F, A0, (size_t)B * h * w * C, s));
  for (auto& ds : dec_steps) {
    const int cin = d.cin[ds.conv], cout = d.cout[ds.conv];
    if (cout == 3) {
      ConvLastArgs a;
      a.x = ds.in; a.wfrag = d.last_w; a.bias = d.last_b; a.y = D; a.B = B; a.H = ds.h; a.W = ds.w;
      TRY(launch_conv_last(a, s));
    } else {
      TRY(run_conv(c, d.convs[ds.conv], ds.in, ds.out, nullptr, B, ds.h, ds.w, ds.up, 1));
    }
    (void)cin;
  }
  {  // encoder over the decoded image (not clipped in training: model.py:176), pools as separate kernels
    ConvFirstArgs a;
    a.x = D; a.wfrag = c->first_w; a.bias = c->first_b; a.y16 = level > 1 ? e0 : nullptr; a.y32 = level == 1 ? Fp : nullptr;
    a.B = B; a.H = H; a.W = W; a.clamp01 = 0; a.usum = nullptr; a.umax = nullptr;
    TRY(launch_conv_first(a, s));
    const half_t* cur = e0;
    for (auto& es : enc_steps) {
      const bool last = es.idx == tap_idx;
      TRY(run_conv(c, c->enc[es.idx], cur, last ? nullptr : es.out, last ? Fp : nullptr, B, es.h, es.w, 0, 1));
      cur = es.out;
      if (es.pooled) { TRY(launch_maxpool2x2(es.out, es.pooled, B, es.h, es.w, ENC_COUT[es.idx], s)); cur = es.pooled; }
    }
  }

  // ---- losses and the gradient w.r.t. the decoded image
  const size_t nF = (size_t)B * h * w * C, nD = (size_t)B * H * W * 3;
  float* g = g0; float* gother = g1;
  TRY(launch_mse(Fp, F, nF, feature_weight, g, 0, lpart, dloss + 0, s));     // g = d feature_loss / d F'
  TRY(launch_relu_mask32(g, Fp, nF, s));
  if (level == 1) {
    TRY(launch_conv_first_dgrad(g, c->first_w32, gp, B, H, W, s));
  } else {
    for (int k = (int)enc_steps.size() - 1; k >= 0; --k) {
      const EncStep& es = enc_steps[k];
      const int cin = ENC_CIN[es.idx], cout = ENC_COUT[es.idx];
      TRY(launch_pow2_scale(g, (size_t)B * es.h * es.w * cout, dloss + 8, s));
      TRY(launch_conv_dgrad(g, c->enc_wt[es.idx], B, es.h, es.w, cin, cout, col, gp, gother, dloss + 8, s));   // w.r.t. the conv input
      std::swap(g, gother);
      if (k > 0) {
        const EncStep& pv = enc_steps[k - 1];
        if (pv.pooled) {
          TRY(launch_maxpool_adjoint(pv.out, g, gother, B, pv.h, pv.w, ENC_COUT[pv.idx], s));
          std::swap(g, gother);
        }
        TRY(launch_relu_mask16(g, pv.out, (size_t)B * pv.h * pv.w * ENC_COUT[pv.idx], s));
      } else {
        TRY(launch_relu_mask16(g, e0, (size_t)B * H * W * 64, s));
      }
    }
    TRY(launch_conv_first_dgrad(g, c->first_w32, gp, B, H, W, s));
  }
  TRY(launch_reflect_fold(gp, gother, B, H, W, 3, s));                       // d feature_loss / d D
  g = gother; gother = (g == g0) ? g1 : g0;
  TRY(launch_mse(D, X, nD, pixel_weight, g, 1, lpart, dloss + 1, s));        // += d pixel_loss / d D
  TRY(launch_tv(D, B, H, W, 3, tv_weight, g, lpart, dloss + 2, s));           // += d tv_loss / d D

  // ---- decoder backward: weight / bias gradients, data gradients down to the second conv
  for (int k = (int)dec_steps.size() - 1; k >= 0; --k) {
    const DecStep& ds = dec_steps[k];
    const int cin = d.cin[ds.conv], cout = d.cout[ds.conv];
    const size_t px = (size_t)B * ds.h * ds.w;
    if (cout != 3) TRY(launch_relu_mask16(g, ds.out, px * cout, s));
    TRY(launch_bias_grad(g, px, cout, partial, d.gb[ds.conv], s));
    int cpad = cout;
    if (cout == 3) {           // the GEMM operands want 16-byte rows: pad the 3-channel gradient to 4
      TRY(launch_pad3to4(g, gother, px, s));
      std::swap(g, gother);
      cpad = 4;
    }
    TRY(launch_pow2_scale(g, px * cpad, dloss + 8, s));                  // one scale per gradient tensor, both GEMMs use it
    TRY(launch_conv_wgrad(ds.in, ds.up, g, cpad, B, ds.h, ds.w, cin, cout, col, partial, conv_wgrad_splits(B, ds.h, ds.w), d.gw[ds.conv], dloss + 8, s));
    if (k > 0) {
      TRY(launch_transpose_w(d.w32[ds.conv], wt, cin, cout, cpad, s));
      TRY(launch_conv_dgrad(g, wt, B, ds.h, ds.w, cin, cpad, col, gp, gother, dloss + 8, s));
      std::swap(g, gother);
      if (ds.up) {
        TRY(launch_upsample_adjoint(g, gother, B, ds.h / 2, ds.w / 2, cin, s));
        std::swap(g, gother);
      }
    }
  }

  // ---- Adam (model.py:199: beta1 0.9, beta2 0.999 in the reference), then refresh the fp16 forward weights
  if (lr != 0.f) TRY(apply_adam(c, d, lr, beta1, beta2, eps, step));
  float hl[4];
  HIP_TRY(hipMemcpyAsync(hl, dloss, 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  losses_out[0] = hl[0]; losses_out[1] = hl[1]; losses_out[2] = hl[2]; losses_out[3] = hl[0] + hl[1] + hl[2];
  return WCT_OK;
}

// the decoder's current fp32 weights (after training steps) and the gradients of the last wct_train_step,
// conv `layer` of the plan (the output conv is the last); any pointer may be NULL
extern "C" int wct_get_decoder_layer(wct_ctx* c, int level, int layer, float* w_hwio, float* bias, float* grad_w, float* grad_b) {
  ARG_CHECK(c && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  Decoder& d = c->dec[level];
  if (!d.loaded) { wct_set_error("decoder weights for relu%d_1 not set (wct_set_decoder)", level); return WCT_ERR_STATE; }
  ARG_CHECK(layer >= 0 && layer < (int)d.w32.size());
  const size_t nw = (size_t)9 * d.cin[layer] * d.cout[layer] * sizeof(float), nb = (size_t)d.cout[layer] * sizeof(float);
  if ((grad_w || grad_b) && d.gw.empty()) { wct_set_error("no training step has run for relu%d_1", level); return WCT_ERR_STATE; }
  if (w_hwio) HIP_TRY(hipMemcpyAsync(w_hwio, d.w32[layer], nw, hipMemcpyDeviceToHost, c->stream));
  if (bias) HIP_TRY(hipMemcpyAsync(bias, d.b32[layer], nb, hipMemcpyDeviceToHost, c->stream));
  if (grad_w) HIP_TRY(hipMemcpyAsync(grad_w, d.gw[layer], nw, hipMemcpyDeviceToHost, c->stream));
  if (grad_b) HIP_TRY(hipMemcpyAsync(grad_b, d.gb[layer], nb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}

// Data-parallel training: run wct_train_step with lr = 0 on every rank's shard, all-reduce (average) the gradient
// buffer this returns over RCCL, then wct_train_apply on every rank.  *grad_dev is ONE contiguous device buffer of
// *count floats holding the gradients of all layers of the decoder (the layout is private; it is the same on every
// rank).  The single-process sequence train_step(lr=0) + train_apply(lr) equals train_step(lr) bit for bit.
extern "C" int wct_train_grad_buffer(wct_ctx* c, int level, float** grad_dev, size_t* count) {
  ARG_CHECK(c && grad_dev && count && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  Decoder& d = c->dec[level];
  if (!d.loaded) { wct_set_error("decoder weights for relu%d_1 not set (wct_set_decoder)", level); return WCT_ERR_STATE; }
  TRY(ensure_train_state(c, d));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *grad_dev = d.grad_arena; *count = d.grad_count;
  return WCT_OK;
}
extern "C" int wct_train_apply(wct_ctx* c, int level, float lr, float beta1, float beta2, float eps, int step) {
  ARG_CHECK(c && level >= 1 && level <= 5 && step >= 1);
  HIP_TRY(hipSetDevice(c->device));
  Decoder& d = c->dec[level];
  if (!d.loaded || d.mw.empty()) { wct_set_error("no gradients for relu%d_1: run wct_train_step first", level); return WCT_ERR_STATE; }
  TRY(apply_adam(c, d, lr, beta1, beta2, eps, step));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}
