// What the units behind the C ABI of libwct_hip.so (include/wct_hip.h) share: the context and what hangs off it, and the
// host-side drivers that one unit (api_*.hip; DESIGN.md section 4 says which holds what) defines and another calls.  Internal:
// not installed, not part of include/.
#pragma once
#include "common.h"
#include "../../include/wct_hip.h"

#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <memory>
#include <vector>
#include <cmath>
#include <algorithm>

// a device buffer that grows on demand (ensure) and releases its memory with its owner
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) hipFree(p); }
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
// what a handle is refilled from: the style image and, for a style region (wct_style_prepare_region*), its label map.  The sibling
// handles of one wct_style_prepare_regions call share one (by reference count: each is freed on its own).
struct StyleSource {
  float* img = nullptr;                              // [Hs][Ws][3] fp32 in [0,1]
  uint8_t* map = nullptr;                            // [Hs][Ws] labels, or null: a whole-image handle
  StyleSource() = default;
  StyleSource(const StyleSource&) = delete;
  StyleSource& operator=(const StyleSource&) = delete;
  ~StyleSource() { if (img) hipFree(img); if (map) hipFree(map); }
};
struct wct_style {
  int Hs = 0, Ws = 0;
  unsigned level_set = 0;                            // bit l: relu<l>_1 is served
  std::shared_ptr<StyleSource> src;
  int label = -1;                                    // >= 0: a style region -- the rows of this label of src->map alone
  int rows[6] = {0};                                 // per served level: the rows its statistics use (a region: counted on the host;
                                                     // else h * w).  Every style key and style workspace is formed from these.
  std::vector<StyleState> cache[6];
  ~wct_style() {
    for (auto& lv : cache)
      for (auto& e : lv) if (e.buf) hipFree(e.buf);
  }
};

// A warm state (wct_warm_create): per level of its set the C x C basis the content eigensolves of a call start from -- the
// re-orthonormalised eigenvectors of the last frame of the previous call -- and whether it holds one yet
struct wct_warm {
  unsigned level_set = 0;                            // bit l: relu<l>_1 is served
  float* basis[6] = {nullptr};
  bool valid[6] = {false};
  ~wct_warm() { for (float* b : basis) if (b) hipFree(b); }
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
  DevBuf mask_in;                  // spatial control: the label map (wct_stylize_masked) or the row labels (wct_*_masked); the
                                   // strength map of wct_transform_strength, wct_adain_strength and wct_stylize_prepared_strength
  DevBuf region_ws;                // style regions: a level's partition (perm, seg_off), the compaction's scratch and the gathered rows
  DevBuf tex_noise, tex[2];        // texture synthesis: the noise images, and the uint8 frames between two passes (alternating)
  DevBuf band_f, band_g, band_img; // banded stylization: a level's full fp32 feature map and its fp16 transform (either may pass
                                   // 2^31 bytes: every launch sees a slice), and the decoded image of one band with its halo
  DevBuf wrap_img, wrap_g, wrap_f; // periodic synthesis (wrap.hip): a level's image with its wrap-around halo (then the decoded image
                                   // with its halo), the fp16 transform with its halo, and the tap cropped to the tile
  DevBuf resize_tab;               // on-device resize: the tap and bounds tables of the last geometry (resize_geom; H = 0: none yet),
  std::vector<int> resize_host;    // and the host copy they were uploaded from
  ResizeGeom resize_geom = {};
  DevBuf guided_ab;                // guided smoothing (guided.hip, guided_color.hip): the coefficient map between the two passes,
                                   // 24 B per pixel under the grey guide, 48 B under the colour guide
  DevBuf up_c, up_s;               // guided upsampling in a stylize call (wct_stylize_prepared_upsampled*): the contents resized to the working
                                   // size and the small stylized frames.  The op's two maps (48 B per SMALL pixel, 96 B under the colour guide) live in guided_ab
  int guided_radius = 8, guided_eps = 650;   // what WCT_FLAG_GUIDED filters with (wct_set_guided; eps 0.01 of the [0,1]^2 convention)
  int guided_guide = WCT_GUIDE_GREY;         // ... and through which guide (wct_set_guided_guide)
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

inline constexpr int LEVEL_C[6] = {0, 64, 128, 256, 512, 512};
inline constexpr int ENC_CIN[12] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
inline constexpr int ENC_COUT[12] = {64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
// enc[i] (conv1_2 .. conv5_1): the level whose relu*_1 it produces (0 = none), and whether a 'same' max-pool follows it
// (conv1_2, conv2_2, conv3_4, conv4_4 -- their outputs feed nothing but the pool)
inline constexpr int ENC_TAP[12] = {0, 2, 0, 3, 0, 0, 0, 4, 0, 0, 0, 5};
inline constexpr int ENC_POOL_AFTER[12] = {1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0};

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

// what the stages of a transform are charged in their profile classes: covariance (4), apply (6), or the one AdaIN launch (7)
struct StageCost { double cov_flops, cov_bytes, apply_flops, apply_bytes, adain_bytes; };

// ---- api_ctx.hip ----------------------------------------------------------
int ensure(wct_ctx* c, DevBuf& b, size_t bytes);                                    // b holds at least `bytes` (may sync and reallocate)
int stage_in(wct_ctx* c, int slot, const void* host, size_t bytes, void** dev);     // host -> c->stage[slot], enqueued
int fetch(wct_ctx* c, void* host, const void* dev, size_t bytes);                   // device -> host, then a stream sync
int eig_status(wct_ctx* c);    // after a stream sync: did an eigensolve of this call fail?
int eig_stale(wct_ctx* c);     // at the start of a blocking call: failures that earlier asynchronous work left unread
void free_layer(ConvLayer& l);
void free_decoder(Decoder& d);

// ---- api_weights.hip ------------------------------------------------------
int upload(wct_ctx* c, const void* host, size_t bytes, void** dev);                 // hipMalloc + copy, blocking
int pack_conv(wct_ctx* c, const float* w_hwio, const float* b, int cin, int cout, ConvLayer* out);

// ---- api_drivers.hip (device pointers, batch B) ---------------------------
// the call block of a launcher on the context's workspace, stream and status words; the caller adds alpha, eps, the outputs
// and the sweeps (all zero here)
static inline WctCall ctx_call(wct_ctx* c, int mode, int stages) {
  WctCall r = {};
  r.mode = mode; r.stages = stages; r.workspace = c->wct_ws.p; r.workspace_bytes = c->wct_ws.cap;
  r.eig_fail = c->eig_fail_dev; r.stream = c->stream;
  return r;
}
// One transform by a variant's launcher, launch(ctx_call of the stage): AdaIN (stages = 0) in one launch, or the covariance,
// eigensolve and apply stages, each timed in its class
template <typename Launch>
static int run_stages(wct_ctx* c, size_t ws_bytes, unsigned flags, const StageCost& cost, Launch&& launch) {
  TRY(ensure(c, c->wct_ws, ws_bytes));
  if (flags & WCT_FLAG_ADAIN) {
    ProfScope ps(c, 7, 0, cost.adain_bytes);
    return launch(ctx_call(c, 0, 0));
  }
  const int mode = (flags & WCT_FLAG_MODE_NP) ? WCT_MODE_NP : WCT_MODE_TF;
  {
    ProfScope ps(c, 4, cost.cov_flops, cost.cov_bytes);
    TRY(launch(ctx_call(c, mode, WCT_STAGE_COV)));
  }
  {
    ProfScope ps(c, 5, 0, 0);
    TRY(launch(ctx_call(c, mode, WCT_STAGE_EIG)));
  }
  ProfScope ps(c, 6, cost.apply_flops, cost.apply_bytes);
  return launch(ctx_call(c, mode, WCT_STAGE_APPLY));
}
void level_dims(int H, int W, int level, int* h, int* w);
int check_min_size(const char* what, int H, int W, int level);
// The geometry of a content chain: level i (relu<l>_1, C channels) sees H x W, its feature map is h x w, and the next level
// sees the decoder's h << (l - 1) by w << (l - 1) -- ceil pooling then x2 upsampling; the frames are Ho x Wo
struct ChainLevel { int l, C, H, W, h, w; };
struct Chain { std::vector<ChainLevel> lv; int Ho, Wo; };
int chain_geometry(int Hc, int Wc, const int* levels, int n_levels, Chain* out);
int run_conv(wct_ctx* c, const ConvLayer& l, const half_t* x, half_t* y16, float* y32, int B, int H, int W, int upsample, int relu,
             int pool = 0, float* usum = nullptr, unsigned* umax = nullptr, bool tap_layer = false);
// run_encoder: taps32[l] the fp32 tap of relu<l>_1 or null; usum[l] / umax[l] the statistics of a tap, taken by the epilogue that
// writes it.  Level 1 alone also takes usum[1] WITHOUT taps32[1] (a level 1 whose readers compute relu1_1 from the image): the
// unit sums are then taken and no fp32 map is stored, and conv1_1 stays a launch of its own -- it is NOT moved into conv1_2's
// loader as it is when neither is given -- which writes the fp16 map for conv1_2 (deepest = 1: nothing at all).
int run_encoder(wct_ctx* c, const float* img, int B, int H, int W, int clamp01, int deepest, float* const taps32[6],
                float* const* usum = nullptr, unsigned* const* umax = nullptr);
int run_decoder(wct_ctx* c, int level, const half_t* feat16, int B, int h, int w, float* img_out);
int run_transform(wct_ctx* c, const float* fc, int Nc, const float* fs, int Ns, int C, int P, float alpha, unsigned flags, float eps,
                  half_t* out16, float* out32, int* sweeps_dev, const WctFeatStats* st = nullptr,
                  const WctStyleRef* prep = nullptr /* a prepared style: fs may be null */,
                  const WctWarmRef* warm = nullptr /* a warm state's basis for this level */,
                  const WctStrength* sm = nullptr /* a strength map per pair: the blend moves into the apply's rows */,
                  const WctImageSrc* src = nullptr /* relu1_1: covariance and apply from the images; fc and fs may be null */);
int mix_weights(const float* weights, int K, float* lambda);
int run_transform_mix(wct_ctx* c, const float* fc, int Nc, const float* const* fs, const int* Ns, int K, const float* lambda, int C,
                      float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev,
                      const WctFeatStats* st = nullptr, const WctStyleRef* prep = nullptr /* K prepared styles: fs may be null */);
int mask_check(const uint8_t* labels, size_t n, int K);
void mask_counts(const uint8_t* mask, int Hm, int Wm, int h, int w, int stride, int K, int* nk);
int run_transform_masked(wct_ctx* c, const float* fc, int Nc, const MaskGeom& g, const int* nk, const float* const* fs, const int* Ns,
                         int K, int C, float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev);

// ---- banded.hip (B = 1: a level in bands of rows and chunks of feature rows, every launch inside the 2^31-byte limits) ----
// the automatic band height of a chain (0: the whole-image call takes every level of it); a caller's band height checked
int band_rows_for(const Chain& chain, int* band_rows);
int band_rows_check(const Chain& chain, int band_rows);
// run_encoder to relu<level>_1 of img [H][W][3] band by band into the full map F [h][w][C] fp32; run_decoder of the full map
// G [h][w][C] fp16 band by band into img_out [h << (l - 1)][w << (l - 1)][3]: the whole pass's bits
int run_encoder_banded(wct_ctx* c, const float* img, int H, int W, int clamp01, int level, int band_rows, float* F);
int run_decoder_banded(wct_ctx* c, int level, const half_t* G, int h, int w, int band_rows, float* img_out);
// the chunks of an h x w map (rows: feature rows per chunk, K: how many), and run_transform over K chunks of n_full rows of
// fc [Nc][C] (the last chunk: what is left) with the content statistics pooled; K = 1 is run_transform itself
int chunk_rule(int h, int w, int C, int stat_rows, int* rows, int* K);
int run_transform_chunked(wct_ctx* c, const float* fc, size_t Nc, int n_full, int K, const float* fs, int Ns, int C, float alpha,
                          unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev, const WctStyleRef* prep = nullptr);

// the wrap plan (periodic synthesis): the halo of a level -- image pixels around the encoder's input, feature pixels in front of
// and behind the decoder's --, and the checks of a tile H x W for a chain (its geometry into *chain): the size rule, the launch limits
void wrap_halo(int level, int* enc, int* dec_before, int* dec_after);
int wrap_chain_check(int H, int W, const int* levels, int n_levels, Chain* chain);

// (banded.hip as well: the wrap drivers)  run_encoder to relu<level>_1 of B tiles img [B][H][W][3] (H, W multiples of 2^(level - 1)) extended periodically by the level's
// halo, the interior of the tap into tap [B][h][w][C] fp32 (c->wrap_img and c->feat_c hold the padded maps); run_decoder of B maps
// G [B][h][w][C] fp16 extended the same way, the interior of the image into img_out [B][h << (l - 1)][w << (l - 1)][3]
int run_encoder_wrap(wct_ctx* c, const float* img, int B, int H, int W, int clamp01, int level, float* tap);
int run_decoder_wrap(wct_ctx* c, int level, const half_t* G, int B, int h, int w, float* img_out);
// what the two need in c->wrap_img / c->feat_c and c->wrap_g / c->wrap_img, ensured here: a driver calls them before its first launch
int wrap_encoder_buffers(wct_ctx* c, int B, int H, int W, int level);
int wrap_decoder_buffers(wct_ctx* c, int B, int h, int w, int level);

// ---- api_ops.hip ----------------------------------------------------------
// guided smoothing of B uint8 frames on the device (guided.hip, or guided_color.hip under WCT_GUIDE_COLOR), the coefficient map in
// c->guided_ab (ensured here); out may be stylized
int run_guided_filter(wct_ctx* c, const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                      int radius, int eps_q, int guide, uint8_t* out);

// guided upsampling of B small uint8 frames on the device (guided_up.hip, or guided_up_color.hip under WCT_GUIDE_COLOR): its maps
// in c->guided_ab (ensured here); out overlaps no input (the callers check or own the buffers).  guided_up_guide_check: a guide
// that is neither of the two is WCT_ERR_ARG with a message that names the argument
int guided_up_guide_check(int guide);
int run_guided_upsample(wct_ctx* c, const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B,
                        int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, int guide, uint8_t* out);

// ---- api_stylize.hip ------------------------------------------------------
int warm_live(const wct_ctx* c, const wct_warm* wm);     // WCT_ERR_STATE unless wm is a live warm state of c
