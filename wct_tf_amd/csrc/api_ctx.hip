// The context behind the C ABI (include/wct_hip.h): its life, the error text, sync and eigensolver status, device memory,
// staging of host arrays, profiling.  Nothing here touches the CPU oracle.
#include "api.h"

#include <stdarg.h>

static thread_local char g_err[512] = "";
void wct_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* wct_last_error(void) { return g_err; }

int ensure(wct_ctx* c, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return WCT_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (b.p) HIP_TRY(hipFree(b.p));
  b.p = nullptr; b.cap = 0;
  size_t want = bytes + bytes / 8 + 4096;
  HIP_TRY(hipMalloc(&b.p, want));
  b.cap = want;
  return WCT_OK;
}

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

void free_layer(ConvLayer& l) {
  if (l.w) hipFree(l.w);
  if (l.b) hipFree(l.b);
  if (l.ww) hipFree(l.ww);
  l = ConvLayer();
}
void free_decoder(Decoder& d) {
  for (auto& l : d.convs) free_layer(l);
  for (auto* v : {&d.w32, &d.b32, &d.mw, &d.vw, &d.mb, &d.vb})
    for (float* p : *v) if (p) hipFree(p);
  if (d.grad_arena) hipFree(d.grad_arena);
  if (d.last_w) hipFree(d.last_w);
  if (d.last_b) hipFree(d.last_b);
  d = Decoder();
}

extern "C" void wct_destroy(wct_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (wct_style* st : c->styles) delete st;
  for (wct_warm* wm : c->warms) delete wm;
  if (c->first_w) hipFree(c->first_w);
  if (c->first_b) hipFree(c->first_b);
  if (c->first_w32) hipFree(c->first_w32);
  for (int i = 0; i < 12; ++i) if (c->enc_wt[i]) hipFree(c->enc_wt[i]);
  for (auto& l : c->enc) free_layer(l);
  for (auto& d : c->dec) free_decoder(d);
  for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (auto& e : c->free_events) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->eig_fail) hipHostFree(c->eig_fail);
  hipStreamDestroy(c->stream);
  delete c;                                               // (every DevBuf releases itself, the device still current)
}

// the solves behind the bases that the warm states in c->warm_used took have been judged: a failure leaves those states cold
static void warm_settle(wct_ctx* c, bool failed) {
  if (failed)
    for (wct_warm* wm : c->warm_used)
      for (bool& v : wm->valid) v = false;
  c->warm_used.clear();
}

// The status words, after a stream sync: did any eigensolve since the last read fail?  Clears them and settles the warm states.
// stale: the failures are those of EARLIER asynchronous work, named for what they are.
static int eig_read(wct_ctx* c, bool stale) {
  const int n_open = c->eig_fail[0], n_nan = c->eig_fail[1];
  warm_settle(c, n_open || n_nan);
  if (!n_open && !n_nan) return WCT_OK;
  c->eig_fail[0] = c->eig_fail[1] = 0;
  if (stale)
    wct_set_error("eigensolver failures of an EARLIER asynchronous wct_stylize_batch_dev call that was not followed by wct_sync "
                  "(%d matri%s still rotating after the sweep budget, %d with non-finite entries): the frames of that call are "
                  "not reliable; the present call was not started", n_open, n_open == 1 ? "x" : "ces", n_nan);
  else
    wct_set_error("eigensolver: %d covariance matri%s still rotating after the sweep budget, %d with non-finite entries "
                  "(NaN/Inf features?); the outputs of this call are not reliable", n_open, n_open == 1 ? "x" : "ces", n_nan);
  return WCT_ERR_NOCONV;
}

// After a stream sync: did any eigensolve of this call fail?  The frames / features of the call are still written (best effort,
// like LAPACK's "did not converge" info > 0), but the status is loud: WCT_STATUS_NOCONV.
int eig_status(wct_ctx* c) { return eig_read(c, false); }

// At the START of a blocking call: failures still pending in the status words were raised by EARLIER asynchronous work
// (wct_stylize_batch_dev calls that nobody followed with wct_sync).  They are reported now -- loudly, but named for what
// they are, and before this call runs, so that its own status and sweep counts are never mixed with them.
int eig_stale(wct_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  return eig_read(c, true);
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

int stage_in(wct_ctx* c, int slot, const void* host, size_t bytes, void** dev) {
  TRY(ensure(c, c->stage[slot], bytes));
  HIP_TRY(hipMemcpyAsync(c->stage[slot].p, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = c->stage[slot].p;
  return WCT_OK;
}
int fetch(wct_ctx* c, void* host, const void* dev, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return WCT_OK;
}

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
