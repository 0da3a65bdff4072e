// The chain geometry and the drivers of the encoder, the decoders and the transforms: device pointers in, launches on the
// context's stream, each timed in its profile class.
#include "api.h"

void level_dims(int H, int W, int level, int* h, int* w) {
  for (int l = 1; l < level; ++l) { H = (H + 1) / 2; W = (W + 1) / 2; }   // 'same' pooling = ceil
  *h = H; *w = W;
}

// every 3x3 conv reflect-pads its input by one pixel, which needs a map of at least 2x2 (tf.pad REFLECT refuses a
// padding >= the dimension just the same): the feature map of the deepest level must still be 2x2
int check_min_size(const char* what, int H, int W, int level) {
  int h, w;
  level_dims(H, W, level, &h, &w);
  if (h < 2 || w < 2) {
    wct_set_error("%s %dx%d is too small for relu%d_1: its %dx%d feature map cannot be reflect-padded (need >= %dx%d pixels)",
                  what, H, W, level, h, w, (1 << (level - 1)) + 1, (1 << (level - 1)) + 1);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

int chain_geometry(int Hc, int Wc, const int* levels, int n_levels, Chain* out) {
  ARG_CHECK(levels && out && n_levels >= 1 && Hc >= 2 && Wc >= 2);
  out->lv.clear();
  int H = Hc, W = Wc;
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    const int l = levels[i];
    TRY(check_min_size("content", H, W, l));
    int h, w;
    level_dims(H, W, l, &h, &w);
    out->lv.push_back(ChainLevel{l, LEVEL_C[l], H, W, h, w});
    H = h << (l - 1); W = w << (l - 1);
  }
  out->Ho = H; out->Wo = W;
  return WCT_OK;
}

int run_conv(wct_ctx* c, const ConvLayer& l, const half_t* x, half_t* y16, float* y32, int B, int H, int W, int upsample, int relu,
             int pool, float* usum, unsigned* umax, bool tap_layer) {
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
int run_encoder(wct_ctx* c, const float* img, int B, int H, int W, int clamp01, int deepest, float* const taps32[6],
                float* const* usum, unsigned* const* umax) {
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
  // usum[1] without taps32[1]: the statistics of relu1_1 without the fp32 tap -- a level 1 whose readers compute relu1_1 from the
  // image themselves (WctImageSrc).  conv1_1 then stays a launch of its own, which takes the unit sums beside the fp16 map it
  // writes for conv1_2 (deepest = 1: the statistics alone, nothing stored): cheaper than the fused launch and a statistics pass.
  const bool stats1 = usum && usum[1] && !taps32[1];
  const bool fuse_conv1 = fuse_conv1_env && deepest > 1 && !taps32[1] && !stats1;
  if (!fuse_conv1) {
    ConvFirstArgs a;
    a.x = img; a.wfrag = c->first_w; a.bias = c->first_b;
    a.y16 = deepest > 1 ? cur : nullptr; a.y32 = taps32[1];
    a.B = B; a.H = H; a.W = W; a.clamp01 = clamp01;
    a.usum = usum && (taps32[1] || stats1) ? usum[1] : nullptr; a.umax = a.usum ? umax[1] : nullptr;
    const double px = (double)B * H * W;
    ProfScope ps(c, 1, 2.0 * px * 27 * 64, px * (12 + 64 * ((a.y16 ? 2 : 0) + (a.y32 ? 4 : 0)) + (stats1 ? 64 * 4 / 16.0 : 0)));
    TRY(launch_conv_first(a, c->stream));
  }
  if (deepest == 1) return WCT_OK;
  // (a pool that follows a layer is fused into that layer's epilogue: ENC_POOL_AFTER)
  int h = H, w = W;
  for (int i = 0; i < 12; ++i) {
    const ConvLayer& l = c->enc[i];
    const int tap = ENC_TAP[i];
    const bool last = tap == deepest;
    const bool fuse = ENC_POOL_AFTER[i];
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
int run_decoder(wct_ctx* c, int level, const half_t* feat16, int B, int h, int w, float* img_out) {
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

int run_transform(wct_ctx* c, const float* fc, int Nc, const float* fs, int Ns, int C, int P, float alpha, unsigned flags, float eps,
                  half_t* out16, float* out32, int* sweeps_dev, const WctFeatStats* st, const WctStyleRef* prep, const WctWarmRef* warm,
                  const WctStrength* sm, const WctImageSrc* src) {
  ARG_CHECK(!src || !(flags & WCT_FLAG_ADAIN));
  const WctSkip skip = (flags & WCT_FLAG_STYLE_SHARED) ? WCT_SKIP_SHARED_STYLE : WCT_SKIP_NONE;
  // (a strength map: the apply's epilogue reads the fp32 features once more, and one byte per pixel)
  // (src: the covariance and the apply read the images, 12 bytes a row -- the covariance the unit sums as well -- instead of the
  //  256-byte rows, and add conv1_1's products)
  const StageCost cost = {(double)P * 2.0 * C * (C + (src ? 27 : 0)) * ((double)Nc + Ns),
                          (double)P * ((double)Nc + Ns) * (src ? 12 + C * 4 / 16.0 : 2.0 * C * 4),
                          (double)P * (2.0 * C * (C + (src ? 27 : 0)) * Nc + 6.0 * C * C * C),
                          src ? (double)P * Nc * (12 + C * ((out16 ? 2 : 0) + (out32 ? 4 : 0))) :
                          (double)P * Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0) + (sm ? 4 : 0)) + (sm ? (double)P * Nc : 0.0),
                          (double)P * (2.0 * Nc + 2.0 * Ns) * C * 4 + (double)P * Nc * C * 6 + (sm ? (double)P * Nc : 0.0)};
  return run_stages(c, wct_workspace_bytes(C, Nc, Ns, P), flags, cost, [&](WctCall r) {
    r.alpha = alpha; r.eps = r.stages ? eps : 1e-5f; r.out16 = out16; r.out32 = out32; r.sweeps_dev = sweeps_dev;
    if (!r.stages) return launch_adain(fc, Nc, fs, Ns, C, P, skip, r, st, prep, sm);
    return launch_wct(fc, Nc, fs, Ns, C, P, skip, r, st, prep, warm, sm, src);
  });
}

// lambda[k] = weights[k] / sum(weights) (Li et al. 2017, sec. 4.2); refuses K outside 1 .. WCT_MIX_MAX and weights that are
// negative, not finite or sum to zero
int mix_weights(const float* weights, int K, float* lambda) {
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
int run_transform_mix(wct_ctx* c, const float* fc, int Nc, const float* const* fs, const int* Ns, int K, const float* lambda, int C,
                      float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev, const WctFeatStats* st,
                      const WctStyleRef* prep) {
  double ns = 0;
  for (int k = 0; k < K; ++k) ns += Ns[k];
  // (the mix of the K colouring matrices is timed with the tail it belongs to)
  const StageCost cost = {2.0 * C * C * (Nc + ns), 2.0 * (Nc + ns) * C * 4, 2.0 * C * C * Nc + 6.0 * C * C * C * (K + 1) + 2.0 * C * C * K,
                          (double)Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)), (2.0 * Nc + 2.0 * ns) * C * 4 + (double)Nc * C * 6};
  return run_stages(c, wct_mix_workspace_bytes(C, Nc, Ns, K, lambda), flags, cost, [&](WctCall r) {
    r.alpha = alpha; r.eps = r.stages ? eps : 1e-5f; r.out16 = out16; r.out32 = out32; r.sweeps_dev = sweeps_dev;
    if (!r.stages) return launch_adain_mix(fc, Nc, fs, Ns, K, lambda, C, r, st, prep);
    return launch_wct_mix(fc, Nc, fs, Ns, K, lambda, C, r, st, prep);
  });
}

// Spatial control: refuses K outside 1 .. WCT_MIX_MAX and any label >= K in the n labels
int mask_check(const uint8_t* labels, size_t n, int K) {
  if (K < 1 || K > WCT_MIX_MAX) { wct_set_error("mask: K = %d styles, must be 1 .. %d", K, (int)WCT_MIX_MAX); return WCT_ERR_ARG; }
  uint8_t top = 0;
  for (size_t i = 0; i < n; ++i) top = labels[i] > top ? labels[i] : top;
  if (top >= K) { wct_set_error("mask: label %d with K = %d styles (labels must be 0 .. K - 1)", (int)top, K); return WCT_ERR_ARG; }
  return WCT_OK;
}

// nk[k] = the rows of label k in an h x w feature map (MaskGeom's rule), on the host: it sizes the launches, and nothing is read back
void mask_counts(const uint8_t* mask, int Hm, int Wm, int h, int w, int stride, int K, int* nk) {
  for (int k = 0; k < K; ++k) nk[k] = 0;
  for (int i = 0; i < h; ++i) {
    const uint8_t* row = mask + (size_t)std::min(i * stride, Hm - 1) * Wm;
    for (int j = 0; j < w; ++j) ++nk[row[std::min(j * stride, Wm - 1)]];
  }
}

// the masked counterpart of run_transform (device pointers; one content of Nc rows labelled by g, K styles); sweeps_dev [2P] or null
int run_transform_masked(wct_ctx* c, const float* fc, int Nc, const MaskGeom& g, const int* nk, const float* const* fs, const int* Ns,
                         int K, int C, float alpha, unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev) {
  double ns = 0;
  int P = 0;
  for (int k = 0; k < K; ++k) { ns += nk[k] >= 2 ? Ns[k] : 0; P += nk[k] >= 2; }
  // (the covariance stage is charged the compaction and gather as well)
  const StageCost cost = {2.0 * C * C * (Nc + ns), (4.0 * Nc + 2.0 * (Nc + ns)) * C * 4, 2.0 * C * C * Nc + 6.0 * C * C * C * P,
                          (double)Nc * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)), (4.0 * Nc + 2.0 * ns) * C * 4 + (double)Nc * C * 6};
  return run_stages(c, wct_masked_workspace_bytes(C, Nc, nk, Ns, K), flags, cost, [&](WctCall r) {
    r.alpha = alpha; r.eps = r.stages ? eps : 1e-5f; r.out16 = out16; r.out32 = out32; r.sweeps_dev = sweeps_dev;
    if (!r.stages) return launch_adain_masked(fc, Nc, g, nk, fs, Ns, K, C, r);
    return launch_wct_masked(fc, Nc, g, nk, fs, Ns, K, C, r);
  });
}
