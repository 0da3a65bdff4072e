// The op-level entry points: host arrays in, host arrays out, one operation of the path each (the tests and the CPU oracle
// compare them one by one).
#include "api.h"

// The strength map of one h x w feature map of Nc rows (host, Hm x Wm) into c->mask_in, enqueued; *sm: its device form
static int stage_strength(wct_ctx* c, const uint8_t* smap, int Hm, int Wm, int Nc, int h, int w, int stride, WctStrength* sm) {
  if (!smap) { wct_set_error("strength map: no map"); return WCT_ERR_ARG; }
  if (Hm < 1 || Wm < 1 || h < 1 || w < 1 || stride < 1 || (long long)h * w != Nc) {
    wct_set_error("strength map: a %dx%d map at stride %d for %d rows as %dx%d feature pixels", Hm, Wm, stride, Nc, h, w);
    return WCT_ERR_ARG;
  }
  TRY(ensure(c, c->mask_in, (size_t)Hm * Wm));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, smap, (size_t)Hm * Wm, hipMemcpyHostToDevice, c->stream));
  *sm = WctStrength{(const uint8_t*)c->mask_in.p, Hm, Wm, w, stride};
  return WCT_OK;
}

// A style region at op level: the hs x ws x C style map into stage 1 and its row labels into c->mask_in, then the rows of `label`
// selected on the device (mask.hip: the compaction of the prepared-style fill, and its segment gather) into c->region_ws.
// *rows: the n selected rows, in pixel order.  Fewer than 2 rows are refused, for WCT and AdaIN alike.
static int stage_region(wct_ctx* c, const float* style, int hs, int ws, int C, const uint8_t* labels, int label, const float** rows, int* n) {
  if (!labels) { wct_set_error("style region: no label map"); return WCT_ERR_ARG; }
  if (label < 0 || label >= WCT_MIX_MAX) { wct_set_error("style region: label %d, must be 0 .. %d", label, (int)WCT_MIX_MAX - 1); return WCT_ERR_ARG; }
  ARG_CHECK(hs >= 1 && ws >= 1 && C >= 4 && C % 4 == 0 && (long long)hs * ws < (1ll << 31));
  const int N = hs * ws;
  int cnt = 0;
  for (int i = 0; i < N; ++i) cnt += labels[i] == label;
  if (cnt < 2) { wct_set_error("style region: label %d has %d rows of the %dx%d style map (a region needs at least 2)", label, cnt, hs, ws); return WCT_ERR_ARG; }
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->mask_in, (size_t)N));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, labels, (size_t)N, hipMemcpyHostToDevice, c->stream));
  void* ds;
  TRY(stage_in(c, 1, style, (size_t)N * C * 4, &ds));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t perm_b = up((size_t)N * sizeof(int)), seg_b = up((WCT_MIX_MAX + 1) * sizeof(int)), cws_b = up(mask_compact_workspace_bytes(N));
  TRY(ensure(c, c->region_ws, perm_b + seg_b + cws_b + (size_t)cnt * C * 4));
  char* base = (char*)c->region_ws.p;
  int *perm = (int*)base, *seg_off = (int*)(base + perm_b);
  float* out = (float*)(base + perm_b + seg_b + cws_b);
  TRY(launch_mask_compact(MaskGeom{(const uint8_t*)c->mask_in.p, hs, ws, ws, 1}, N, label + 1, perm, seg_off, base + perm_b + seg_b, c->stream));
  TRY(launch_mask_gather_segment((const float*)ds, perm, seg_off, label, cnt, C, out, c->stream));
  *rows = out; *n = cnt;
  return WCT_OK;
}

// One (content, style) pair of feature matrices through run_transform.  warm (with its level): the content solve starts from the
// state's basis of that level, which then takes this pair's.  sm: a strength map on the device (stage_strength).
static int transform_pair(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C, float alpha, unsigned flags,
                          float eps, wct_warm* warm, int level, float* out, int* sweeps_out, const WctStrength* sm = nullptr,
                          const float* style_dev = nullptr /* the style rows on the device already (stage_region): `style` is unused */) {
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void *dc, *ds = (void*)style_dev;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  if (!style_dev) TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->stage[3], 256));
  WctWarmRef wr = {};
  if (warm) {
    c->warm_used.push_back(warm);
    wr = {warm->basis[level], warm->valid[level] ? 1 : 0};
  }
  TRY(run_transform(c, (float*)dc, Nc, (float*)ds, Ns, C, 1, alpha, flags, eps, nullptr, (float*)c->stage[2].p, (int*)c->stage[3].p,
                    nullptr, nullptr, warm ? &wr : nullptr, sm));
  if (warm) warm->valid[level] = true;
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) TRY(fetch(c, sweeps_out, c->stage[3].p, 2 * sizeof(int)));
  return eig_status(c);
}

extern "C" int wct_transform(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C,
                             float alpha, int mode, float eps, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out && (mode == WCT_NP || mode == WCT_TF));
  return transform_pair(c, content, Nc, style, Ns, C, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps, nullptr, 0, out, sweeps_out);
}

// wct_transform with the style rows selected on the device: the rows of `label` of the hs x ws style map
extern "C" int wct_transform_region(wct_ctx* c, const float* content, int Nc, const float* style, int hs, int ws, int C,
                                    const uint8_t* labels, int label, float alpha, int mode, float eps, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out && (mode == WCT_NP || mode == WCT_TF));
  const float* rows;
  int n;
  TRY(stage_region(c, style, hs, ws, C, labels, label, &rows, &n));
  return transform_pair(c, content, Nc, nullptr, n, C, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps, nullptr, 0, out, sweeps_out,
                        nullptr, rows);
}

extern "C" int wct_transform_strength(wct_ctx* c, const float* content, int Nc, int h, int w, const uint8_t* smap, int Hm, int Wm,
                                      int stride, const float* style, int Ns, int C, float alpha, int mode, float eps, float* out,
                                      int* sweeps_out) {
  ARG_CHECK(c && content && style && out && (mode == WCT_NP || mode == WCT_TF));
  HIP_TRY(hipSetDevice(c->device));
  WctStrength sm;
  TRY(stage_strength(c, smap, Hm, Wm, Nc, h, w, stride, &sm));
  return transform_pair(c, content, Nc, style, Ns, C, alpha, mode == WCT_NP ? WCT_FLAG_MODE_NP : 0, eps, nullptr, 0, out, sweeps_out, &sm);
}

// wct_transform with the content statistics pooled over chunks of chunk_rows rows (the last chunk: what is left, a single
// left-over row joins the chunk before it); one chunk is wct_transform itself
extern "C" int wct_transform_chunked(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C, float alpha, int mode,
                                     float eps, int chunk_rows, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out && (mode == WCT_NP || mode == WCT_TF) && chunk_rows >= 0 && Nc >= 2);
  const unsigned flags = mode == WCT_NP ? WCT_FLAG_MODE_NP : 0;
  if (chunk_rows == 0 || chunk_rows >= Nc) return transform_pair(c, content, Nc, style, Ns, C, alpha, flags, eps, nullptr, 0, out, sweeps_out);
  if (chunk_rows < 2) { wct_set_error("chunk_rows = %d: a chunk needs at least 2 rows for a covariance", chunk_rows); return WCT_ERR_ARG; }
  int K = (Nc + chunk_rows - 1) / chunk_rows;
  if (Nc - (K - 1) * chunk_rows < 2) --K;
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->stage[3], 256));
  TRY(run_transform_chunked(c, (float*)dc, (size_t)Nc, chunk_rows, K, (float*)ds, Ns, C, alpha, flags, eps, nullptr, (float*)c->stage[2].p,
                            (int*)c->stage[3].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4));
  if (sweeps_out) TRY(fetch(c, sweeps_out, c->stage[3].p, 2 * sizeof(int)));
  return eig_status(c);
}

// the warm twin of wct_transform: the content solve started from the state's basis of `level`
extern "C" int wct_transform_warm(wct_ctx* c, const float* content, int Nc, const float* style, int Ns, int C, float alpha,
                                  unsigned flags, wct_warm* warm, int level, float* out, int* sweeps_out) {
  ARG_CHECK(c && content && style && out);
  TRY(warm_live(c, warm));
  if (flags & (WCT_FLAG_ADAIN | WCT_FLAG_SWAP5 | WCT_FLAG_STYLE_SHARED | WCT_FLAG_IMAGES_F32 | WCT_FLAG_CONTENT_COLORS | WCT_FLAG_GUIDED)) {
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
  return transform_pair(c, content, Nc, style, Ns, C, alpha, flags, -1.f, warm, level, out, sweeps_out);
}

// the call block of the AdaIN ops: fp32 into stage 2
static WctCall adain_call(wct_ctx* c, float alpha, float epsilon) {
  WctCall r = ctx_call(c, 0, 0);
  r.alpha = alpha; r.eps = epsilon; r.out32 = (float*)c->stage[2].p;
  return r;
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
  TRY(launch_adain((float*)dc, Nc, (float*)ds, Ns, C, 1, WCT_SKIP_NONE, adain_call(c, alpha, epsilon), nullptr, nullptr));
  return fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4);
}

// wct_adain with the style rows selected on the device (wct_transform_region's rule, its < 2 rows refusal included)
extern "C" int wct_adain_region(wct_ctx* c, const float* content, int Nc, const float* style, int hs, int ws, int C, const uint8_t* labels,
                                int label, float alpha, float epsilon, float* out) {
  ARG_CHECK(c && content && style && out);
  const float* rows;
  int n;
  TRY(stage_region(c, style, hs, ws, C, labels, label, &rows, &n));
  void* dc;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->wct_ws, wct_workspace_bytes(C, Nc, n, 1)));
  TRY(launch_adain((float*)dc, Nc, rows, n, C, 1, WCT_SKIP_NONE, adain_call(c, alpha, epsilon), nullptr, nullptr));
  return fetch(c, out, c->stage[2].p, (size_t)Nc * C * 4);
}

extern "C" int wct_adain_strength(wct_ctx* c, const float* content, int Nc, int h, int w, const uint8_t* smap, int Hm, int Wm, int stride,
                                  const float* style, int Ns, int C, float alpha, float epsilon, float* out) {
  ARG_CHECK(c && content && style && out);
  HIP_TRY(hipSetDevice(c->device));
  WctStrength sm;
  TRY(stage_strength(c, smap, Hm, Wm, Nc, h, w, stride, &sm));
  void *dc, *ds;
  TRY(stage_in(c, 0, content, (size_t)Nc * C * 4, &dc));
  TRY(stage_in(c, 1, style, (size_t)Ns * C * 4, &ds));
  TRY(ensure(c, c->stage[2], (size_t)Nc * C * 4));
  TRY(ensure(c, c->wct_ws, wct_workspace_bytes(C, Nc, Ns, 1)));
  TRY(launch_adain((float*)dc, Nc, (float*)ds, Ns, C, 1, WCT_SKIP_NONE, adain_call(c, alpha, epsilon), nullptr, nullptr, &sm));
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
  TRY(launch_adain_mix((float*)dc, Nc, ds, Ns, K, lambda, C, adain_call(c, alpha, epsilon), nullptr, nullptr));
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
  TRY(launch_adain_masked((float*)dc, Nc, g, nk, ds, Ns, K, C, adain_call(c, alpha, epsilon)));
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
  // the order check is jacobi_make_group's, made here before anything is sized by C: a refused call stages and launches nothing
  ARG_CHECK(c && A && evals && evecs && nmat >= 1 && nmat <= 64 && C % 32 == 0 && C >= 32 && C <= 1024);
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
  float* taps[6] = {};
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

// The band height of a banded twin: the caller's, checked, or (0) the automatic one -- one band where the whole-image call runs
static int twin_band_rows(int H, int W, int level, int* band_rows) {
  Chain chain;
  TRY(chain_geometry(H, W, &level, 1, &chain));
  if (*band_rows) return band_rows_check(chain, *band_rows);
  TRY(band_rows_for(chain, band_rows));
  if (!*band_rows) *band_rows = (H + 15) / 16 * 16;
  return WCT_OK;
}

extern "C" int wct_encode_banded(wct_ctx* c, const float* img01, int H, int W, int level, int band_rows, float* feat) {
  ARG_CHECK(c && img01 && feat && level >= 1 && level <= 5 && band_rows >= 0);
  HIP_TRY(hipSetDevice(c->device));
  TRY(twin_band_rows(H, W, level, &band_rows));
  int h, w;
  level_dims(H, W, level, &h, &w);
  void* dimg;
  TRY(stage_in(c, 0, img01, (size_t)H * W * 3 * 4, &dimg));
  const size_t fb = (size_t)h * w * LEVEL_C[level] * 4;
  TRY(ensure(c, c->band_f, fb));
  TRY(run_encoder_banded(c, (float*)dimg, H, W, 0, level, band_rows, (float*)c->band_f.p));
  return fetch(c, feat, c->band_f.p, fb);
}

extern "C" int wct_decode_banded(wct_ctx* c, const float* feat, int h, int w, int level, int band_rows, float* img) {
  ARG_CHECK(c && feat && img && level >= 1 && level <= 5 && band_rows >= 0 && h >= 2 && w >= 2 && h <= (1 << 26) && w <= (1 << 26));
  HIP_TRY(hipSetDevice(c->device));
  const int C = LEVEL_C[level], scale = 1 << (level - 1);
  TRY(twin_band_rows(h * scale, w * scale, level, &band_rows));
  void* df;
  const size_t n = (size_t)h * w * C;
  TRY(stage_in(c, 0, feat, n * 4, &df));
  TRY(ensure(c, c->band_g, n * 2));
  TRY(launch_f32_to_f16((float*)df, (half_t*)c->band_g.p, n, c->stream));
  const size_t ib = (size_t)h * scale * w * scale * 3 * 4;
  TRY(ensure(c, c->img_t[0], ib));
  TRY(run_decoder_banded(c, level, (half_t*)c->band_g.p, h, w, band_rows, (float*)c->img_t[0].p));
  return fetch(c, img, c->img_t[0].p, ib);
}

// Wrap-around halos, op level (csrc/wrap.hip; the plan and the drivers in banded.hip)
extern "C" int wct_wrap_pad_batch_dev(wct_ctx* c, const float* in, int B, int H, int W, int C, int top, int bottom, int left, int right,
                                      float* out) {
  ARG_CHECK(c != nullptr);
  if (!in || !out) { wct_set_error("wrap pad: null map pointer"); return WCT_ERR_ARG; }
  if (B < 1 || B > 32) { wct_set_error("wrap pad: B = %d maps, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (H < 1 || W < 1 || C < 1 || top < 0 || bottom < 0 || left < 0 || right < 0) {
    wct_set_error("wrap pad: a %dx%dx%d map with pads %d %d %d %d (sizes >= 1, pads >= 0)", H, W, C, top, bottom, left, right);
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  ProfScope ps(c, 7, 0, 2.0 * B * ((double)top + H + bottom) * ((double)left + W + right) * C * 4);
  return launch_wrap_pad(in, out, B, H, W, C, 4, top, bottom, left, right, c->stream);
}

extern "C" int wct_wrap_pad(wct_ctx* c, const float* x, int H, int W, int C, int top, int bottom, int left, int right, float* y) {
  ARG_CHECK(c && x && y && H >= 1 && W >= 1 && C >= 1 && top >= 0 && bottom >= 0 && left >= 0 && right >= 0);
  HIP_TRY(hipSetDevice(c->device));
  const unsigned long long out_elems = ((unsigned long long)top + H + bottom) * ((unsigned long long)left + W + right) * (unsigned long long)C;
  if (out_elems >= (1ull << 29)) {                           // (launch_wrap_pad's bound, before the staging buffers are sized)
    wct_set_error("wrap pad: the padded %dx%dx%d map passes 2^31 bytes in one launch", H, W, C);
    return WCT_ERR_ARG;
  }
  void* dx;
  TRY(stage_in(c, 0, x, (size_t)H * W * C * 4, &dx));
  TRY(ensure(c, c->stage[1], (size_t)out_elems * 4));
  TRY(wct_wrap_pad_batch_dev(c, (const float*)dx, 1, H, W, C, top, bottom, left, right, (float*)c->stage[1].p));
  return fetch(c, y, c->stage[1].p, (size_t)out_elems * 4);
}

extern "C" int wct_encode_wrap(wct_ctx* c, const float* img01, int H, int W, int level, float* feat) {
  ARG_CHECK(c && img01 && feat && level >= 1 && level <= 5);
  HIP_TRY(hipSetDevice(c->device));
  Chain chain;
  TRY(wrap_chain_check(H, W, &level, 1, &chain));
  void* dimg;
  TRY(stage_in(c, 0, img01, (size_t)H * W * 3 * 4, &dimg));
  const size_t fb = (size_t)chain.lv[0].h * chain.lv[0].w * LEVEL_C[level] * 4;
  TRY(ensure(c, c->wrap_f, fb));
  TRY(run_encoder_wrap(c, (const float*)dimg, 1, H, W, 0, level, (float*)c->wrap_f.p));
  return fetch(c, feat, c->wrap_f.p, fb);
}

extern "C" int wct_decode_wrap(wct_ctx* c, const float* feat, int h, int w, int level, float* img) {
  ARG_CHECK(c && feat && img && level >= 1 && level <= 5 && h >= 1 && w >= 1 && h <= (1 << 26) && w <= (1 << 26));
  HIP_TRY(hipSetDevice(c->device));
  const int C = LEVEL_C[level], scale = 1 << (level - 1);
  Chain chain;
  TRY(wrap_chain_check(h * scale, w * scale, &level, 1, &chain));
  void* df;
  const size_t n = (size_t)h * w * C;
  TRY(stage_in(c, 0, feat, n * 4, &df));
  TRY(ensure(c, c->wct_out, n * 2));
  TRY(launch_f32_to_f16((float*)df, (half_t*)c->wct_out.p, n, c->stream));
  const size_t ib = (size_t)h * scale * w * scale * 3 * 4;
  TRY(ensure(c, c->img_t[0], ib));
  TRY(run_decoder_wrap(c, level, (const half_t*)c->wct_out.p, 1, h, w, (float*)c->img_t[0].p));
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

// Guided smoothing, op level (csrc/guided.hip, csrc/guided_color.hip).  run_guided_filter: the two launches on B frames resident on
// the device, their coefficient map in the context's workspace; the stylize chain ends in it under WCT_FLAG_GUIDED
int run_guided_filter(wct_ctx* c, const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                      int radius, int eps_q, int guide, uint8_t* out) {
  TRY(guided_check(B, Ho, Wo, Hc, Wc, radius, eps_q, guide));
  TRY(ensure(c, c->guided_ab, guided_workspace_bytes(B, Ho, Wo, guide)));
  // per pixel: s and c read twice (the entering and the leaving row), the map written once and read twice, the frame written
  const int map = guide == WCT_GUIDE_COLOR ? 48 : 24;
  ProfScope ps(c, 7, 0, (double)B * Ho * Wo * (2 * 3 + 2 * 3 * (content_f32 ? 4 : 1) + 3 * map + 3 * (content_f32 ? 4 : 1) + 3));
  return launch_guided_filter(stylized, content, content_f32, B, Ho, Wo, Hc, Wc, radius, eps_q, guide, c->guided_ab.p, out, c->stream);
}

extern "C" int wct_set_guided(wct_ctx* c, int radius, int eps_q) {
  ARG_CHECK(c != nullptr);
  TRY(guided_check(1, 1, 1, 1, 1, radius, eps_q, WCT_GUIDE_GREY));
  c->guided_radius = radius; c->guided_eps = eps_q;
  return WCT_OK;
}

extern "C" int wct_set_guided_guide(wct_ctx* c, int guide) {
  ARG_CHECK(c != nullptr);
  TRY(guided_check(1, 1, 1, 1, 1, 1, 1, guide));
  c->guided_guide = guide;
  return WCT_OK;
}

extern "C" int wct_guided_filter_guide_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc,
                                                 int Wc, int B, int radius, int eps_q, int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_check(B, Ho, Wo, Hc, Wc, radius, eps_q, guide));
  HIP_TRY(hipSetDevice(c->device));
  return run_guided_filter(c, stylized, content, 0, B, Ho, Wo, Hc, Wc, radius, eps_q, guide, out);
}

extern "C" int wct_guided_filter_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc,
                                           int B, int radius, int eps_q, uint8_t* out) {
  return wct_guided_filter_guide_batch_dev(c, stylized, Ho, Wo, content, Hc, Wc, B, radius, eps_q, WCT_GUIDE_GREY, out);
}

extern "C" int wct_guided_filter_guide(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc,
                                       int radius, int eps_q, int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_check(1, Ho, Wo, Hc, Wc, radius, eps_q, guide));
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc;
  TRY(stage_in(c, 0, stylized, (size_t)Ho * Wo * 3, &ds));
  TRY(stage_in(c, 1, content, (size_t)Hc * Wc * 3, &dc));
  TRY(wct_guided_filter_guide_batch_dev(c, (uint8_t*)ds, Ho, Wo, (uint8_t*)dc, Hc, Wc, 1, radius, eps_q, guide, (uint8_t*)ds));    // (in place)
  return fetch(c, out, ds, (size_t)Ho * Wo * 3);
}

extern "C" int wct_guided_filter(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int radius,
                                 int eps_q, uint8_t* out) {
  return wct_guided_filter_guide(c, stylized, Ho, Wo, content, Hc, Wc, radius, eps_q, WCT_GUIDE_GREY, out);
}

// Guided upsampling, op level (csrc/guided_up.hip, csrc/guided_up_color.hip).  run_guided_upsample: the three launches on B frames
// resident on the device; wct_stylize_prepared_upsampled* end in it
int guided_up_guide_check(int guide) {
  if (guide == WCT_GUIDE_GREY || guide == WCT_GUIDE_COLOR) return WCT_OK;
  wct_set_error("guided upsample: guide %d, must be WCT_GUIDE_GREY (%d) or WCT_GUIDE_COLOR (%d)", guide, WCT_GUIDE_GREY, WCT_GUIDE_COLOR);
  return WCT_ERR_ARG;
}

int run_guided_upsample(wct_ctx* c, const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B,
                        int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, int guide, uint8_t* out) {
  TRY(guided_up_check(B, h, w, hc, wc, H, W, radius, eps_q));
  TRY(guided_up_guide_check(guide));
  const bool color = guide == WCT_GUIDE_COLOR;
  TRY(ensure(c, c->guided_ab, color ? guided_up_color_workspace_bytes(B, h, w) : guided_up_workspace_bytes(B, h, w)));
  // per small pixel: s and c read twice and the map written (pass 1), the map read twice and the means written; per full pixel
  // the content read and the frame written; the means are read through the cache, once per pixel at ratio 1 and less above it
  const int cb = content_f32 ? 4 : 1;
  const double map = color ? 48.0 : 24.0;
  ProfScope ps(c, 7, 0, (double)B * h * w * (2 * 3 + 2 * 3 * cb + 4 * map) + (double)B * H * W * (3 * cb + 3) + (double)B * hc * wc * map);
  if (color)
    return launch_guided_upsample_color(stylized, content_small, content_full, content_f32, B, h, w, hc, wc, H, W, radius, eps_q,
                                        c->guided_ab.p, out, c->stream);
  return launch_guided_upsample(stylized, content_small, content_full, content_f32, B, h, w, hc, wc, H, W, radius, eps_q, c->guided_ab.p,
                                out, c->stream);
}

static bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uint8_t *pa = (const uint8_t*)a, *pb = (const uint8_t*)b;
  return pa < pb + nb && pb < pa + na;
}

static int guided_upsample_checks(const void* stylized, const void* content_small, const void* content_full, const void* out, int B, int h,
                                  int w, int hc, int wc, int H, int W, int radius, int eps_q, int guide) {
  if (!stylized) { wct_set_error("guided upsample: stylized is a null pointer"); return WCT_ERR_ARG; }
  if (!content_small) { wct_set_error("guided upsample: content_small is a null pointer"); return WCT_ERR_ARG; }
  if (!content_full) { wct_set_error("guided upsample: content_full is a null pointer"); return WCT_ERR_ARG; }
  if (!out) { wct_set_error("guided upsample: out is a null pointer"); return WCT_ERR_ARG; }
  TRY(guided_up_check(B, h, w, hc, wc, H, W, radius, eps_q));
  return guided_up_guide_check(guide);
}

extern "C" int wct_guided_upsample_guide_batch_dev(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc,
                                                   int wc, const uint8_t* content_full, int H, int W, int B, int radius, int eps_q,
                                                   int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_upsample_checks(stylized, content_small, content_full, out, B, h, w, hc, wc, H, W, radius, eps_q, guide));
  const size_t nout = (size_t)B * H * W * 3;
  if (bytes_overlap(out, nout, stylized, (size_t)B * h * w * 3) || bytes_overlap(out, nout, content_small, (size_t)B * hc * wc * 3) ||
      bytes_overlap(out, nout, content_full, nout)) {
    wct_set_error("guided upsample: out overlaps an input (a full pixel reads small pixels that other blocks have long left)");
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  return run_guided_upsample(c, stylized, content_small, content_full, 0, B, h, w, hc, wc, H, W, radius, eps_q, guide, out);
}

extern "C" int wct_guided_upsample_batch_dev(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc,
                                             int wc, const uint8_t* content_full, int H, int W, int B, int radius, int eps_q,
                                             uint8_t* out) {
  return wct_guided_upsample_guide_batch_dev(c, stylized, h, w, content_small, hc, wc, content_full, H, W, B, radius, eps_q, WCT_GUIDE_GREY,
                                             out);
}

extern "C" int wct_guided_upsample_guide(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                                         const uint8_t* content_full, int H, int W, int radius, int eps_q, int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_upsample_checks(stylized, content_small, content_full, out, 1, h, w, hc, wc, H, W, radius, eps_q, guide));   // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc, *dC;
  TRY(stage_in(c, 0, stylized, (size_t)h * w * 3, &ds));
  TRY(stage_in(c, 1, content_small, (size_t)hc * wc * 3, &dc));
  TRY(stage_in(c, 2, content_full, (size_t)H * W * 3, &dC));
  TRY(ensure(c, c->stage[3], (size_t)H * W * 3));
  TRY(wct_guided_upsample_guide_batch_dev(c, (uint8_t*)ds, h, w, (uint8_t*)dc, hc, wc, (uint8_t*)dC, H, W, 1, radius, eps_q, guide,
                                          (uint8_t*)c->stage[3].p));
  return fetch(c, out, c->stage[3].p, (size_t)H * W * 3);
}

extern "C" int wct_guided_upsample(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                                   const uint8_t* content_full, int H, int W, int radius, int eps_q, uint8_t* out) {
  return wct_guided_upsample_guide(c, stylized, h, w, content_small, hc, wc, content_full, H, W, radius, eps_q, WCT_GUIDE_GREY, out);
}

// Temporal guided smoothing, op level (csrc/guided_time.hip): frames f0 .. f1 - 1 of a clip of F resident frames, the coefficient
// map of the whole clip in the workspace of the 2-D op
extern "C" int wct_guided_filter_time_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc,
                                                int Wc, int F, int radius, int eps_q, int frames_t, int f0, int f1, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter along time: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->guided_ab, guided_workspace_bytes(F, Ho, Wo, GUIDE_GREY)));
  // per pixel of the n1 frames of pass 1: s and c read twice in each of the up to 2T + 1 frames of the window, the map written;
  // of the n2 frames of pass 2: the map read twice in each frame of the window, c read, the frame written
  const int n1 = (f1 + frames_t > F ? F : f1 + frames_t) - (f0 - frames_t < 0 ? 0 : f0 - frames_t), n2 = f1 - f0, win = 2 * frames_t + 1;
  ProfScope ps(c, 7, 0, (double)Ho * Wo * (n1 * (win * 2 * 6 + 24.0) + n2 * (win * 2 * 24.0 + 3 + 3)));
  return launch_guided_time(stylized, content, 0, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, c->guided_ab.p, out, c->stream);
}

extern "C" int wct_guided_filter_time(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int F,
                                      int radius, int eps_q, int frames_t, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter along time: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, 0, F));                 // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc;
  TRY(stage_in(c, 0, stylized, (size_t)F * Ho * Wo * 3, &ds));
  TRY(stage_in(c, 1, content, (size_t)F * Hc * Wc * 3, &dc));
  TRY(wct_guided_filter_time_batch_dev(c, (uint8_t*)ds, Ho, Wo, (uint8_t*)dc, Hc, Wc, F, radius, eps_q, frames_t, 0, F, (uint8_t*)ds));
  return fetch(c, out, ds, (size_t)F * Ho * Wo * 3);
}

extern "C" int wct_guided_time_max_radius(int frames_t) { return guided_time_max_radius(frames_t); }

// Temporal guided smoothing along camera motion, op level (csrc/guided_motion.hip).  The estimator: the guide planes, the partial
// sums and the steps live in the workspace of the guided ops, which the filter only uses afterwards on the same stream
extern "C" int wct_motion_global_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int F, int range, int32_t* pos_out) {
  ARG_CHECK(c != nullptr);
  if (!content || !pos_out) { wct_set_error("global motion: null pointer"); return WCT_ERR_ARG; }
  TRY(motion_check(F, Hc, Wc, range));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->guided_ab, motion_workspace_bytes(F, Hc, Wc, range)));
  const int32_t* steps_dev = nullptr;
  int32_t steps[31 * 2];
  {
    // per pair: (2 range + 1)^2 candidates of Hc Wc / 4 byte differences; the planes written once and read once per candidate row
    const double cand = (2.0 * range + 1) * (2.0 * range + 1);
    ProfScope ps(c, 7, 0, (double)F * Hc * Wc * 4 + (double)(F - 1) * cand * Hc * Wc * 0.5);
    TRY(launch_motion_global(content, F, Hc, Wc, range, c->guided_ab.p, &steps_dev, c->stream));
  }
  if (F > 1) TRY(fetch(c, steps, steps_dev, (size_t)(F - 1) * 8));
  pos_out[0] = pos_out[1] = 0;
  for (int f = 0; f + 1 < F; ++f) {
    pos_out[2 * f + 2] = pos_out[2 * f] + steps[2 * f];
    pos_out[2 * f + 3] = pos_out[2 * f + 1] + steps[2 * f + 1];
  }
  return WCT_OK;
}

extern "C" int wct_motion_global(wct_ctx* c, const uint8_t* contents, int Hc, int Wc, int F, int range, int32_t* pos_out) {
  ARG_CHECK(c != nullptr);
  if (!contents || !pos_out) { wct_set_error("global motion: null pointer"); return WCT_ERR_ARG; }
  TRY(motion_check(F, Hc, Wc, range));                                                        // (before the staging buffer is sized)
  HIP_TRY(hipSetDevice(c->device));
  void* dc;
  TRY(stage_in(c, 1, contents, (size_t)F * Hc * Wc * 3, &dc));
  return wct_motion_global_batch_dev(c, (const uint8_t*)dc, Hc, Wc, F, range, pos_out);
}

extern "C" int wct_guided_filter_motion_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc,
                                                  int Wc, int F, int radius, int eps_q, int frames_t, const int32_t* pos, int f0, int f1,
                                                  uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter along motion: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_motion_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos));
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->guided_ab, guided_workspace_bytes(F, Ho, Wo, GUIDE_GREY)));
  // the traffic of wct_guided_filter_time_batch_dev: the same loads, shifted
  const int n1 = (f1 + frames_t > F ? F : f1 + frames_t) - (f0 - frames_t < 0 ? 0 : f0 - frames_t), n2 = f1 - f0, win = 2 * frames_t + 1;
  ProfScope ps(c, 7, 0, (double)Ho * Wo * (n1 * (win * 2 * 6 + 24.0) + n2 * (win * 2 * 24.0 + 3 + 3)));
  return launch_guided_motion(stylized, content, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, pos, f0, f1, c->guided_ab.p, out, c->stream);
}

extern "C" int wct_guided_filter_motion(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int F,
                                        int radius, int eps_q, int frames_t, const int32_t* pos, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!stylized || !content || !out) { wct_set_error("guided filter along motion: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_motion_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, 0, F, pos));            // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc;
  TRY(stage_in(c, 0, stylized, (size_t)F * Ho * Wo * 3, &ds));
  TRY(stage_in(c, 1, content, (size_t)F * Hc * Wc * 3, &dc));
  TRY(wct_guided_filter_motion_batch_dev(c, (uint8_t*)ds, Ho, Wo, (uint8_t*)dc, Hc, Wc, F, radius, eps_q, frames_t, pos, 0, F,
                                         (uint8_t*)ds));
  return fetch(c, out, ds, (size_t)F * Ho * Wo * 3);
}

// Temporal guided smoothing under a chosen guide, op level: WCT_GUIDE_GREY routes to the two ops above (with or without
// positions), WCT_GUIDE_COLOR to csrc/guided_color_time.hip, whose coefficient map of the whole clip (48 B per pixel, twice the
// grey one) sits in the same workspace, sized before any launch
static int guided_time_guide_check(int guide) {
  if (guide == WCT_GUIDE_GREY || guide == WCT_GUIDE_COLOR) return WCT_OK;
  wct_set_error("guided filter along time: guide %d, must be WCT_GUIDE_GREY (%d) or WCT_GUIDE_COLOR (%d)", guide, WCT_GUIDE_GREY,
                WCT_GUIDE_COLOR);
  return WCT_ERR_ARG;
}

extern "C" int wct_guided_filter_time_guide_batch_dev(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc,
                                                      int Wc, int F, int radius, int eps_q, int frames_t, int guide, const int32_t* pos,
                                                      int f0, int f1, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_time_guide_check(guide));
  if (guide == WCT_GUIDE_GREY)
    return pos ? wct_guided_filter_motion_batch_dev(c, stylized, Ho, Wo, content, Hc, Wc, F, radius, eps_q, frames_t, pos, f0, f1, out)
               : wct_guided_filter_time_batch_dev(c, stylized, Ho, Wo, content, Hc, Wc, F, radius, eps_q, frames_t, f0, f1, out);
  if (!stylized || !content || !out) { wct_set_error("guided filter along time: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_color_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos));
  // (the check keeps F Ho Wo 3 below 2^31, so the product below is below 2^35; the test stands for a size_t of 32 bits)
  const unsigned long long pixels = (unsigned long long)F * (unsigned long long)Ho * (unsigned long long)Wo;
  if (pixels > (unsigned long long)SIZE_MAX / 48) {
    wct_set_error("guided filter along time: the colour guide's workspace of %d frames of %dx%d at 48 B per pixel overflows size_t", F, Ho,
                  Wo);
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->guided_ab, guided_workspace_bytes(F, Ho, Wo, GUIDE_COLOR)));
  // per pixel of the n1 frames of pass 1: s and c read twice in each of the up to 2T + 1 frames of the window, the map written;
  // of the n2 frames of pass 2: the map read twice in each frame of the window, c read, the frame written
  const int n1 = (f1 + frames_t > F ? F : f1 + frames_t) - (f0 - frames_t < 0 ? 0 : f0 - frames_t), n2 = f1 - f0, win = 2 * frames_t + 1;
  ProfScope ps(c, 7, 0, (double)Ho * Wo * (n1 * (win * 2 * 6 + 48.0) + n2 * (win * 2 * 48.0 + 3 + 3)));
  return launch_guided_color_time(stylized, content, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, pos, f0, f1, c->guided_ab.p, out,
                                  c->stream);
}

extern "C" int wct_guided_filter_time_guide(wct_ctx* c, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc,
                                            int F, int radius, int eps_q, int frames_t, int guide, const int32_t* pos, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_time_guide_check(guide));
  if (guide == WCT_GUIDE_GREY)
    return pos ? wct_guided_filter_motion(c, stylized, Ho, Wo, content, Hc, Wc, F, radius, eps_q, frames_t, pos, out)
               : wct_guided_filter_time(c, stylized, Ho, Wo, content, Hc, Wc, F, radius, eps_q, frames_t, out);
  if (!stylized || !content || !out) { wct_set_error("guided filter along time: null image pointer"); return WCT_ERR_ARG; }
  TRY(guided_color_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, 0, F, pos));         // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc;
  TRY(stage_in(c, 0, stylized, (size_t)F * Ho * Wo * 3, &ds));
  TRY(stage_in(c, 1, content, (size_t)F * Hc * Wc * 3, &dc));
  TRY(wct_guided_filter_time_guide_batch_dev(c, (uint8_t*)ds, Ho, Wo, (uint8_t*)dc, Hc, Wc, F, radius, eps_q, frames_t, guide, pos, 0, F,
                                             (uint8_t*)ds));
  return fetch(c, out, ds, (size_t)F * Ho * Wo * 3);
}

// Temporal guided upsampling, op level (csrc/guided_up_time.hip): frames f0 .. f1 - 1 of a clip of F resident small frames, delivered
// against their full contents; the coefficient map of the clip and the means of the delivered frames in the workspace of the
// guided ops
static int guided_upsample_time_checks(const void* stylized, const void* content_small, const void* content_full, const void* out, int F,
                                       int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, int frames_t, int f0, int f1,
                                       const int32_t* pos) {
  if (!stylized) { wct_set_error("guided upsample along time: stylized is a null pointer"); return WCT_ERR_ARG; }
  if (!content_small) { wct_set_error("guided upsample along time: content_small is a null pointer"); return WCT_ERR_ARG; }
  if (!content_full) { wct_set_error("guided upsample along time: content_full is a null pointer"); return WCT_ERR_ARG; }
  if (!out) { wct_set_error("guided upsample along time: out is a null pointer"); return WCT_ERR_ARG; }
  return guided_up_time_check(F, h, w, hc, wc, H, W, radius, eps_q, frames_t, f0, f1, pos);
}

extern "C" int wct_guided_upsample_time_batch_dev(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc,
                                                  int wc, const uint8_t* content_full, int H, int W, int F, int radius, int eps_q,
                                                  int frames_t, const int32_t* pos, int f0, int f1, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_upsample_time_checks(stylized, content_small, content_full, out, F, h, w, hc, wc, H, W, radius, eps_q, frames_t, f0, f1, pos));
  const size_t nout = (size_t)(f1 - f0) * H * W * 3;
  if (bytes_overlap(out, nout, stylized, (size_t)F * h * w * 3) || bytes_overlap(out, nout, content_small, (size_t)F * hc * wc * 3) ||
      bytes_overlap(out, nout, content_full, nout)) {
    wct_set_error("guided upsample along time: out overlaps an input (a full pixel reads small pixels that other blocks have long left)");
    return WCT_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->guided_ab, guided_up_time_workspace_bytes(F, h, w, f0, f1)));
  // per small pixel of the n1 frames of pass 1: s and c read twice in each frame of the window, the map written; of the n2 delivered
  // frames: the map read twice in each frame of the window, the means written; per full pixel the content read and the frame
  // written, the means read through the cache
  const int n1 = (f1 + frames_t > F ? F : f1 + frames_t) - (f0 - frames_t < 0 ? 0 : f0 - frames_t), n2 = f1 - f0, win = 2 * frames_t + 1;
  ProfScope ps(c, 7, 0, (double)h * w * (n1 * (win * 2 * 6 + 24.0) + n2 * (win * 2 * 24.0 + 24.0)) + (double)n2 * H * W * 6 +
                            (double)n2 * hc * wc * 24.0);
  return launch_guided_upsample_time(stylized, content_small, content_full, F, h, w, hc, wc, H, W, radius, eps_q, frames_t, pos, f0, f1,
                                     c->guided_ab.p, out, c->stream);
}

extern "C" int wct_guided_upsample_time(wct_ctx* c, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                                        const uint8_t* content_full, int H, int W, int F, int radius, int eps_q, int frames_t,
                                        const int32_t* pos, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(guided_upsample_time_checks(stylized, content_small, content_full, out, F, h, w, hc, wc, H, W, radius, eps_q, frames_t, 0, F,
                                  pos));                                                      // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  void *ds, *dc, *dC;
  TRY(stage_in(c, 0, stylized, (size_t)F * h * w * 3, &ds));
  TRY(stage_in(c, 1, content_small, (size_t)F * hc * wc * 3, &dc));
  TRY(stage_in(c, 2, content_full, (size_t)F * H * W * 3, &dC));
  TRY(ensure(c, c->stage[3], (size_t)F * H * W * 3));
  TRY(wct_guided_upsample_time_batch_dev(c, (uint8_t*)ds, h, w, (uint8_t*)dc, hc, wc, (uint8_t*)dC, H, W, F, radius, eps_q, frames_t, pos,
                                         0, F, (uint8_t*)c->stage[3].p));
  return fetch(c, out, c->stage[3].p, (size_t)F * H * W * 3);
}

// Seeded noise images for texture synthesis, op level (csrc/noise.hip): the refusals both calls share
static int texture_noise_checks(int H, int W, int B, const void* out) {
  if (!out) { wct_set_error("texture noise: null output pointer"); return WCT_ERR_ARG; }
  if (B < 1 || B > 32) { wct_set_error("texture noise: B = %d images, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (H < 1 || W < 1) { wct_set_error("texture noise: an empty %dx%d image", H, W); return WCT_ERR_ARG; }
  return WCT_OK;
}

extern "C" int wct_texture_noise_batch_dev(wct_ctx* c, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                           uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(texture_noise_checks(H, W, B, out));
  HIP_TRY(hipSetDevice(c->device));
  ProfScope ps(c, 7, 0, (double)B * H * W * 3);
  return launch_texture_noise(out, B, H, W, seed, first_sample, smooth, c->stream);
}

extern "C" int wct_texture_noise(wct_ctx* c, int H, int W, unsigned seed, unsigned sample, int smooth, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(texture_noise_checks(H, W, 1, out));
  HIP_TRY(hipSetDevice(c->device));
  if ((unsigned long long)H * (unsigned long long)W * 3ull >= (1ull << 31)) {              // (before the staging buffer is sized)
    wct_set_error("texture noise: a %dx%dx3 image passes 2^31 bytes", H, W);
    return WCT_ERR_ARG;
  }
  TRY(ensure(c, c->stage[0], (size_t)H * W * 3));
  TRY(wct_texture_noise_batch_dev(c, H, W, 1, seed, sample, smooth, (uint8_t*)c->stage[0].p));
  return fetch(c, out, c->stage[0].p, (size_t)H * W * 3);
}

// On-device resize, op level (csrc/resize.hip): the refusals both calls share
static int resize_checks(const void* in, int H, int W, int B, int h, int w, const void* out) {
  if (!in || !out) { wct_set_error("resize: null image pointer"); return WCT_ERR_ARG; }
  if (B < 1 || B > 32) { wct_set_error("resize: B = %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (H < 1 || W < 1 || h < 1 || w < 1) { wct_set_error("resize: an empty image, %dx%d to %dx%d", H, W, h, w); return WCT_ERR_ARG; }
  return resize_check_bytes(B, H, W, h, w);
}

// The tables of (H, W, h, w) in c->resize_tab: built and uploaded when the geometry is not the last call's.  Only then does the
// call wait for the stream (the tables that earlier launches still read are about to be replaced).
static int resize_tables(wct_ctx* c, int H, int W, int h, int w) {
  const ResizeGeom& g = c->resize_geom;
  if (g.H == H && g.W == W && g.h == h && g.w == w) return WCT_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->resize_geom = ResizeGeom{};
  const size_t n = resize_table_ints(H, W, h, w);
  c->resize_host.resize(n);
  ResizeGeom plan;
  TRY(resize_plan(H, W, h, w, &plan, c->resize_host.data()));
  TRY(ensure(c, c->resize_tab, n * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(c->resize_tab.p, c->resize_host.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  c->resize_geom = plan;
  return WCT_OK;
}

extern "C" int wct_resize_batch_dev(wct_ctx* c, const uint8_t* in, int H, int W, int B, int h, int w, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(resize_checks(in, H, W, B, h, w, out));
  const size_t nin = (size_t)B * H * W * 3, nout = (size_t)B * h * w * 3;
  if (in < out + nout && out < in + nin) { wct_set_error("resize: the output overlaps the input"); return WCT_ERR_ARG; }
  HIP_TRY(hipSetDevice(c->device));
  ProfScope ps(c, 7, 0, (double)nin + (double)nout);
  if (h == H && w == W) {                                    // a copy
    HIP_TRY(hipMemcpyAsync(out, in, nin, hipMemcpyDeviceToDevice, c->stream));
    return WCT_OK;
  }
  TRY(resize_tables(c, H, W, h, w));
  return launch_resize(in, out, B, c->resize_geom, (const int*)c->resize_tab.p, c->stream);
}

extern "C" int wct_resize(wct_ctx* c, const uint8_t* img, int H, int W, int h, int w, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(resize_checks(img, H, W, 1, h, w, out));               // (before the staging buffers are sized)
  HIP_TRY(hipSetDevice(c->device));
  if (h != H || w != W) TRY(resize_tables(c, H, W, h, w));   // (the plan's refusal: before the image is read)
  void* din;
  TRY(stage_in(c, 0, img, (size_t)H * W * 3, &din));
  TRY(ensure(c, c->stage[1], (size_t)h * w * 3));
  TRY(wct_resize_batch_dev(c, (uint8_t*)din, H, W, 1, h, w, (uint8_t*)c->stage[1].p));
  return fetch(c, out, c->stage[1].p, (size_t)h * w * 3);
}
