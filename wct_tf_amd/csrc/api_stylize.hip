// The stylize entry points: one predict() (wct.py:70-106) as a chain of launches on the context's stream -- with style images,
// with prepared styles, with a warm start, and with spatial control of a video on prepared styles.
#include "api.h"

extern "C" int wct_output_size(int Hc, int Wc, const int* levels, int n_levels, int* Ho, int* Wo) {
  ARG_CHECK(Ho && Wo);
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));
  *Ho = chain.Ho; *Wo = chain.Wo;
  return WCT_OK;
}

// The level check of every stylize driver: each level in range, served by all K handles (none with style images), its decoder loaded
static int check_levels(const wct_ctx* c, const int* levels, int n_levels, const wct_style* const* handles = nullptr, int K = 0) {
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    for (int k = 0; k < K; ++k)
      if (!(handles[k]->level_set & (1u << levels[i]))) {
        wct_set_error("prepared style %d was not prepared for relu%d_1", k, levels[i]);
        return WCT_ERR_ARG;
      }
    if (!c->dec[levels[i]].loaded) { wct_set_error("decoder weights for relu%d_1 not set", levels[i]); return WCT_ERR_STATE; }
  }
  return WCT_OK;
}

// The checks of a stylize call with style images before any launch: the levels and their decoders, the content chain (*chain), K
// styles large enough for the deepest level (*deepest)
static int stylize_checks(wct_ctx* c, int Hc, int Wc, const uint8_t* const* styles, const int* Hs, const int* Ws, int K,
                          const int* levels, int n_levels, int* deepest, Chain* chain) {
  TRY(check_levels(c, levels, n_levels));
  TRY(chain_geometry(Hc, Wc, levels, n_levels, chain));
  *deepest = *std::max_element(levels, levels + n_levels);
  for (int k = 0; k < K; ++k) { ARG_CHECK(styles[k]); TRY(check_min_size("style", Hs[k], Ws[k], *deepest)); }
  return WCT_OK;
}

static size_t sample_bytes(unsigned flags) { return (flags & WCT_FLAG_IMAGES_F32) ? sizeof(float) : 1; }   // per colour sample of the inputs

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
constexpr size_t UROW = 32 * UMAX_SLOTS;       // words per row of c->umax: 32 images
static bool fuse_stats() {
  static const int on = getenv("WCT_FUSE_STATS") ? atoi(getenv("WCT_FUSE_STATS")) : 1;
  return on != 0;
}

// The content chain of a stylize call (model.py:77-101) on B contents img_c [B][Hc][Wc][3] fp32: per level of `chain` the encoder
// pass with a tap (and its unit sums, umax row 0 -- its first umax_clear bytes cleared from level clear_from on), the transform, and
// the decoder into the ping-pong images; then the uint8 frames into out (wct.py:66-68).
// style_at(l, b, &hs, &ws): pair b's style features of relu<l>_1, hs x ws.  transform(i, g, st): level i (g: relu<g.l>_1, g.C
// channels) of the g.h x g.w contents in c->feat_c -> c->wct_out (fp16), st the content's unit sums.  WCT_FLAG_SWAP5 runs the
// style-swap at relu5_1 instead.  WCT_FLAG_CONTENT_COLORS: the last launch puts the frames' luminance on the colours of
// content_raw, the contents as the caller gave them ([B][Hc][Wc][3] on the device: uint8, or fp32 with WCT_FLAG_IMAGES_F32).
// WCT_FLAG_GUIDED: the uint8 frames are then filtered in place with content_raw as guide (guided.hip or guided_color.hip: the context's radius,
// eps_q and guide), and the colour op, if flagged too, runs after that as the stand-alone uint8 kernel.
template <typename StyleAt, typename Transform>
static int stylize_levels(wct_ctx* c, const float* img_c, const void* content_raw, int B, const Chain& chain, unsigned flags,
                          size_t umax_clear, int clear_from, StyleAt&& style_at, Transform&& transform, uint8_t* out,
                          bool l1_img = false) {
  unsigned* const umax_c = (unsigned*)c->umax.p;
  const float* cur = img_c;
  for (int i = 0; i < (int)chain.lv.size(); ++i) {
    const ChainLevel& g = chain.lv[i];
    const int l = g.l, C = g.C, h = g.h, w = g.w;
    // l1_img (wct_stylize_batch_dev): the transform of relu1_1 computes its rows from the level's input image -- no tap, the
    // encoder pass leaves the unit sums alone and c->feat_c is not grown for the level
    const bool from_image = l == 1 && l1_img;
    float* ctaps[6] = {};
    if (!from_image) {
      TRY(ensure(c, c->feat_c, (size_t)B * h * w * C * 4));
      ctaps[l] = (float*)c->feat_c.p;
    }
    float* us_c[6] = {};
    unsigned* um_c[6] = {};
    if (fuse_stats() && w % 16 == 0) {
      TRY(ensure(c, c->usum_c, (size_t)B * h * (w / 16) * C * 4));
      us_c[l] = (float*)c->usum_c.p; um_c[l] = umax_c;
      if (i >= clear_from) HIP_TRY(hipMemsetAsync(umax_c, 0, umax_clear, c->stream));
    }
    WctFeatStats st = {};
    st.u[0] = us_c[l]; st.umax[0] = um_c[l];
    // level i>0 encodes clip(previous decoded, 0, 1) (model.py:86): the clamp is in the conv1_1 loader
    TRY(run_encoder(c, cur, B, g.H, g.W, i > 0, l, ctaps, us_c, um_c));
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
      TRY(transform(i, g, st));
    DevBuf& dst = c->img_t[i & 1];                     // the decoder's h << (l - 1) by w << (l - 1) image: the next level's input
    TRY(ensure(c, dst, (size_t)B * (h << (l - 1)) * (w << (l - 1)) * 3 * 4));
    TRY(run_decoder(c, l, (half_t*)c->wct_out.p, B, h, w, (float*)dst.p));
    cur = (float*)dst.p;
  }
  const int H = chain.Ho, W = chain.Wo, Hc = chain.lv[0].H, Wc = chain.lv[0].W;
  const int f32 = (flags & WCT_FLAG_IMAGES_F32) ? 1 : 0;
  if (flags & WCT_FLAG_GUIDED) {
    // the frames by the chain's own rule, filtered in place against the content; the colour op, if asked for, runs last on them
    {
      ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 5);
      TRY(launch_f32_to_u8(cur, out, (size_t)B * H * W * 3, c->stream));
    }
    TRY(run_guided_filter(c, out, content_raw, f32, B, H, W, Hc, Wc, c->guided_radius, c->guided_eps, c->guided_guide, out));
    if (!(flags & WCT_FLAG_CONTENT_COLORS)) return WCT_OK;
    ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 2 + (double)B * Hc * Wc * 3 * (f32 ? 4 : 1));
    return launch_content_colors_u8_any(out, content_raw, f32, B, H, W, Hc, Wc, out, c->stream);
  }
  if (flags & WCT_FLAG_CONTENT_COLORS) {
    ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 5 + (double)B * Hc * Wc * 3 * (f32 ? 4 : 1));
    return launch_content_colors_f32(cur, content_raw, f32, B, H, W, Hc, Wc, out, c->stream);
  }
  ProfScope ps(c, 7, 0, (double)B * H * W * 3 * 5);
  return launch_f32_to_u8(cur, out, (size_t)B * H * W * 3, c->stream);
}

// Host frame in, host frame out, around a device driver (B = 1): failures that earlier asynchronous work left are reported first,
// the content goes through stage 0 and the frame comes back through stage 2.  enqueue(content_dev, out_dev) is the driver's call.
template <typename Enqueue>
static int host_frame(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const int* levels, int n_levels, unsigned flags,
                      uint8_t* out, Enqueue&& enqueue) {
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int Ho, Wo;
  TRY(wct_output_size(Hc, Wc, levels, n_levels, &Ho, &Wo));
  void* dc;
  TRY(stage_in(c, 0, content, (size_t)Hc * Wc * 3 * sample_bytes(flags), &dc));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  TRY(enqueue(dc, (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

extern "C" int wct_stylize_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* style,
                                     int Hs, int Ws, int B, const int* levels, int n_levels, float alpha,
                                     unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && style && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32);
  HIP_TRY(hipSetDevice(c->device));
  int deepest;
  Chain chain;
  TRY(stylize_checks(c, Hc, Wc, &style, &Hs, &Ws, 1, levels, n_levels, &deepest, &chain));

  // WCT_FLAG_STYLE_SHARED: `style` is ONE image for all B pairs (a video with a fixed style); its encoder pass,
  // statistics and eigensystems are computed once per call instead of once per pair
  const int shared = (flags & WCT_FLAG_STYLE_SHARED) ? 1 : 0;
  const int Bs = shared ? 1 : B;
  const float *img_c, *img_s;
  TRY(images_f32(c, flags, content, (size_t)B * Hc * Wc * 3, style, (size_t)Bs * Hs * Ws * 3, &img_c, &img_s));
  const bool want_stats = fuse_stats();
  TRY(ensure(c, c->umax, 7 * UROW * sizeof(unsigned)));
  unsigned* const umax_c = (unsigned*)c->umax.p;                    // row 0: content (per level), rows 1..5: style levels
  if (want_stats) HIP_TRY(hipMemsetAsync(c->umax.p, 0, 7 * UROW * sizeof(unsigned), c->stream));
  // relu1_1 from the images: plain WCT with the epilogue statistics on, every width at level 1 a multiple of
  // 16.  The style's fp32 relu1_1 is then never stored -- its conv1_1 pass takes the unit sums beside the fp16 map conv1_2 reads
  // (run_encoder: unit sums without a tap) -- and the covariance of both sides is computed from the images.
  // (WCT_L1_FROM_IMAGE=0: the stored map; test hook, read once per process)
  static const int l1_env = getenv("WCT_L1_FROM_IMAGE") ? atoi(getenv("WCT_L1_FROM_IMAGE")) : 1;
  bool l1_img = false;
  if (l1_env && want_stats && !(flags & WCT_FLAG_ADAIN) && Ws % 16 == 0)
    for (const ChainLevel& g : chain.lv)
      if (g.l == 1) l1_img = true;
  for (const ChainLevel& g : chain.lv)
    if (g.l == 1 && g.W % 16 != 0) l1_img = false;
  // ONE style pass with a tap per requested level (model.py:69-75)
  float* taps[6] = {};
  float* us_s[6] = {};
  unsigned* um_s[6] = {};
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i];
    int h, w;
    level_dims(Hs, Ws, l, &h, &w);
    if (!(l == 1 && l1_img)) {
      TRY(ensure(c, c->feat_s[l], (size_t)Bs * h * w * LEVEL_C[l] * 4));
      taps[l] = (float*)c->feat_s[l].p;
    }
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
  return stylize_levels(c, img_c, content, B, chain, flags, UROW * sizeof(unsigned), 1, style_at,
                        [&](int i, const ChainLevel& g, WctFeatStats st) {
                          int hs, ws;
                          const float* fs = style_at(g.l, 0, &hs, &ws);
                          st.u[1] = us_s[g.l]; st.umax[1] = um_s[g.l];
                          if (g.l == 1 && l1_img) {
                            // level i encodes the contents (i = 0) or the previous level's decoded images, clamped (stylize_levels)
                            const float* in = i == 0 ? img_c : (const float*)c->img_t[(i - 1) & 1].p;
                            const WctImageSrc src = {{{in, g.H, g.W, i > 0}, {img_s, Hs, Ws, 0}}, c->first_w, c->first_b};
                            return run_transform(c, nullptr, g.h * g.w, nullptr, hs * ws, g.C, B, alpha, flags, -1.f,
                                                 (half_t*)c->wct_out.p, nullptr, nullptr, &st, nullptr, nullptr, nullptr, &src);
                          }
                          return run_transform(c, (float*)c->feat_c.p, g.h * g.w, fs, hs * ws, g.C, B, alpha, flags, -1.f,
                                               (half_t*)c->wct_out.p, nullptr, nullptr, &st);
                        }, out, l1_img);
}

extern "C" int wct_stylize(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* style, int Hs, int Ws,
                           const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && style && out);
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    void* ds;
    TRY(stage_in(c, 1, style, (size_t)Hs * Ws * 3 * sample_bytes(flags), &ds));
    return wct_stylize_batch_dev(c, (uint8_t*)dc, Hc, Wc, (uint8_t*)ds, Hs, Ws, 1, levels, n_levels, alpha, flags, frame);
  });
}

// The body of wct_stylize_mix / wct_stylize_masked (their checks done): the style encoder runs once per style (sizes may differ),
// then the content chain with B = 1, `level_transform` in the place of the single-style transform.
// level_transform(g, fs, Ns, st): stylize_levels' transform of level g, fs[k] / Ns[k] style k's features of the level.
// (Not through host_frame: its checks come before the report of stale failures.)
// WCT_FLAG_SWAP5 (K = 1) runs wct_stylize's style-swap at relu5_1 instead.
template <typename LevelTransform>
static int stylize_multi(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* const* styles, const int* Hs,
                         const int* Ws, int K, const int* levels, int n_levels, unsigned flags, uint8_t* out,
                         LevelTransform&& level_transform) {
  HIP_TRY(hipSetDevice(c->device));
  int deepest;
  Chain chain;
  TRY(stylize_checks(c, Hc, Wc, styles, Hs, Ws, K, levels, n_levels, &deepest, &chain));
  TRY(eig_stale(c));
  // inputs: the content in stage 0, the K styles back to back in mix_in
  const size_t px = sample_bytes(flags);
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
    float* taps[6] = {};
    for (int i = 0; i < n_levels; ++i) taps[levels[i]] = (float*)c->feat_mix[levels[i]].p + foff[levels[i]][k];
    TRY(run_encoder(c, img_s + soff[k], 1, Hs[k], Ws[k], 0, deepest, taps));
  }

  // the content chain, B = 1: pair k is style k (the style-swap takes K = 1); its umax row is cleared at every level
  TRY(ensure(c, c->umax, 32 * UMAX_SLOTS * sizeof(unsigned)));
  const size_t frame_bytes = (size_t)chain.Ho * chain.Wo * 3;
  TRY(ensure(c, c->stage[2], frame_bytes));
  auto style_at = [&](int l, int k, int* hs, int* ws) {
    level_dims(Hs[k], Ws[k], l, hs, ws);
    return (const float*)c->feat_mix[l].p + foff[l][k];
  };
  TRY(stylize_levels(c, img_c, dc, 1, chain, flags, UMAX_SLOTS * sizeof(unsigned), 0, style_at,
                     [&](int, const ChainLevel& g, const WctFeatStats& st) {
                       const float* fs[WCT_MIX_MAX];
                       int Ns[WCT_MIX_MAX];
                       for (int k = 0; k < K; ++k) {
                         int hs, ws;
                         fs[k] = style_at(g.l, k, &hs, &ws);
                         Ns[k] = hs * ws;
                       }
                       return level_transform(g, fs, Ns, &st);
                     }, (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, frame_bytes));
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
                       [&](const ChainLevel& g, const float* const* fs, const int* Ns, const WctFeatStats* st) {
                         return run_transform_mix(c, (float*)c->feat_c.p, g.h * g.w, fs, Ns, K, lambda, g.C, alpha, flags, -1.f,
                                                  (half_t*)c->wct_out.p, nullptr, nullptr, st);
                       });
}

// One predict() with spatial control at every level (Li et al. 2017, sec. 4.2, Fig. 7): stylize_multi with the masked transform
// in the place of the single-style transform.  The labels of a level are counted on the host (they size its launches; nothing is
// read back) when the chain, whose geometry says which pixels they are, reaches the level.
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
  for (int i = 0; i < n_levels; ++i) ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);    // (before anything is enqueued)
  HIP_TRY(hipSetDevice(c->device));
  TRY(ensure(c, c->mask_in, (size_t)Hc * Wc));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, mask, (size_t)Hc * Wc, hipMemcpyHostToDevice, c->stream));
  return stylize_multi(c, content, Hc, Wc, styles, Hs, Ws, K, levels, n_levels, flags, out,
                       [&](const ChainLevel& g, const float* const* fs, const int* Ns, const WctFeatStats*) {
                         int nk[WCT_MIX_MAX];
                         mask_counts(mask, Hc, Wc, g.h, g.w, 1 << (g.l - 1), K, nk);
                         const MaskGeom mg = {(const uint8_t*)c->mask_in.p, Hc, Wc, g.w, 1 << (g.l - 1)};
                         return run_transform_masked(c, (float*)c->feat_c.p, g.h * g.w, mg, nk, fs, Ns, K, g.C, alpha, flags, -1.f,
                                                     (half_t*)c->wct_out.p, nullptr, nullptr);
                       });
}

// ---------------------------------------------------------------------------
// video warm start (stylize_video.py:112-135 calls predict() per frame and solves every content covariance from scratch): the
// content eigensolves of a call start from the eigenvectors of the previous call's last frame (csrc/warm.hip)
// ---------------------------------------------------------------------------
int warm_live(const wct_ctx* c, const wct_warm* wm) {
  if (wm && std::find(c->warms.begin(), c->warms.end(), wm) != c->warms.end()) return WCT_OK;
  wct_set_error("warm state %p is not a live state of this context (freed, or created by another context)", (const void*)wm);
  return WCT_ERR_STATE;
}

extern "C" int wct_warm_create(wct_ctx* c, const int* levels, int n_levels, wct_warm** out) {
  ARG_CHECK(c && levels && out && n_levels >= 1 && n_levels <= 16);
  *out = nullptr;
  for (int i = 0; i < n_levels; ++i) ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
  HIP_TRY(hipSetDevice(c->device));
  std::unique_ptr<wct_warm> wm(new wct_warm());
  for (int i = 0; i < n_levels; ++i) {
    const int l = levels[i];
    if (wm->basis[l]) continue;
    wm->level_set |= 1u << l;
    if (hipMalloc((void**)&wm->basis[l], (size_t)LEVEL_C[l] * LEVEL_C[l] * sizeof(float)) != hipSuccess) {
      wct_set_error("hipMalloc failed (warm state, relu%d_1)", l);
      return WCT_ERR_NOMEM;
    }
  }
  c->warms.push_back(wm.get());
  *out = wm.release();
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
  delete wm;
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

// ---------------------------------------------------------------------------
// prepared styles: the style side once, any number of contents (wct.py:70-106 / stylize_video.py:88-121 with a fixed style)
// ---------------------------------------------------------------------------
static int style_live(const wct_ctx* c, const wct_style* st) {
  if (st && std::find(c->styles.begin(), c->styles.end(), st) != c->styles.end()) return WCT_OK;
  wct_set_error("prepared style %p is not a live handle of this context (freed, or prepared by another context)", (const void*)st);
  return WCT_ERR_STATE;
}

static bool same_key(const WctStyleKey& a, const WctStyleKey& b) { return a.nslab == b.nslab && a.nsplit == b.nsplit && a.ksplit == b.ksplit; }

static StyleState* state_find(wct_style* st, int level, const WctStyleKey& key, int kind) {
  for (auto& e : st->cache[level])
    if (e.kind == kind && same_key(e.key, key)) return &e;
  return nullptr;
}

struct StyleNeed { int level; WctStyleKey key; };

// the rows a handle's statistics use at a level: what every style key and style workspace is formed from (a whole-image handle:
// h * w of the style's feature map; a style region: the rows of its label, counted when it was prepared)
static int style_rows(const wct_style* st, int level) { return st->rows[level]; }

// the rows of `label` in the h x w feature map of a level (MaskGeom's rule at `stride`), counted on the host
static int region_count(const uint8_t* map, int Hm, int Wm, int h, int w, int stride, int label) {
  int n = 0;
  for (int i = 0; i < h; ++i) {
    const uint8_t* row = map + (size_t)std::min(i * stride, Hm - 1) * Wm;
    for (int j = 0; j < w; ++j) n += row[std::min(j * stride, Wm - 1)] == label;
  }
  return n;
}

// Computes the states needs[g] of the G handles of `group` for one kind (none of them cached) on the ctx stream.  The handles share
// their source -- one handle, or the siblings of wct_style_prepare_regions --, so there is ONE encoder pass of the style with a tap
// per level needed and, for style regions, ONE compaction of each level's labels (mask.hip); then per state the rows of the
// handle's label are gathered (n_k * C floats) in front of launch_style_state.  A whole-image handle takes the tap itself: the
// launches it always took.  Blocking, and the eigensolves are checked before a state is kept: on WCT_ERR_NOCONV (or any error)
// none of them stays in a cache.
static int style_fill(wct_ctx* c, wct_style* const* group, int G, int kind, const std::vector<StyleNeed>* needs) {
  bool any = false;
  for (int g = 0; g < G; ++g) any = any || !needs[g].empty();
  if (!any) return WCT_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));               // (a state evicted below may belong to frames still in flight)
  const wct_style* st0 = group[0];
  const bool region = st0->label >= 0;
  int deepest = 0, labels = 0;
  size_t row_floats = 0;
  float* taps[6] = {};
  for (int g = 0; g < G; ++g)
    for (const StyleNeed& n : needs[g]) {
      int h, w;
      level_dims(st0->Hs, st0->Ws, n.level, &h, &w);
      TRY(ensure(c, c->feat_s[n.level], (size_t)h * w * LEVEL_C[n.level] * 4));
      taps[n.level] = (float*)c->feat_s[n.level].p;
      deepest = std::max(deepest, n.level);
      labels = std::max(labels, group[g]->label + 1);
      row_floats = std::max(row_floats, (size_t)style_rows(group[g], n.level) * LEVEL_C[n.level]);
    }
  // a region's scratch in c->region_ws: per level needed its partition (perm, seg_off), then the compaction's counts and the rows
  int *perm[6] = {}, *seg_off[6] = {};
  void* compact_ws = nullptr;
  float* rows = nullptr;
  if (region) {
    size_t off = 0, poff[6] = {}, soff[6] = {}, cbytes = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    for (int l = 1; l <= 5; ++l) {
      if (!taps[l]) continue;
      int h, w;
      level_dims(st0->Hs, st0->Ws, l, &h, &w);
      poff[l] = take((size_t)h * w * sizeof(int));
      soff[l] = take((WCT_MIX_MAX + 1) * sizeof(int));
      cbytes = std::max(cbytes, mask_compact_workspace_bytes(h * w));
    }
    const size_t coff = take(cbytes), roff = take(row_floats * sizeof(float));
    TRY(ensure(c, c->region_ws, off));
    char* base = (char*)c->region_ws.p;
    for (int l = 1; l <= 5; ++l)
      if (taps[l]) { perm[l] = (int*)(base + poff[l]); seg_off[l] = (int*)(base + soff[l]); }
    compact_ws = base + coff;
    rows = (float*)(base + roff);
  }
  TRY(run_encoder(c, st0->src->img, 1, st0->Hs, st0->Ws, 0, deepest, taps));
  if (region)
    for (int l = 1; l <= 5; ++l) {
      if (!taps[l]) continue;
      int h, w;
      level_dims(st0->Hs, st0->Ws, l, &h, &w);
      ProfScope ps(c, 7, 0, (double)h * w * 2);
      TRY(launch_mask_compact(MaskGeom{st0->src->map, st0->Hs, st0->Ws, w, 1 << (l - 1)}, h * w, labels, perm[l], seg_off[l], compact_ws,
                              c->stream));
    }
  std::vector<float*> fresh;
  int rc = WCT_OK;
  for (int g = 0; g < G && !rc; ++g) {
    wct_style* st = group[g];
    int gathered = 0;                                     // the level whose rows of this handle `rows` holds
    for (const StyleNeed& n : needs[g]) {
      const int C = LEVEL_C[n.level], Ns = style_rows(st, n.level);
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
      lv.push_back(StyleState{n.key, kind, buf, c->style_clock});
      fresh.push_back(buf);
      if (hipMemsetAsync(buf, 0, wct_style_state_floats(C) * sizeof(float), c->stream) != hipSuccess) { wct_set_error("hipMemsetAsync failed"); rc = WCT_ERR_HIP; break; }
      const float* feat = taps[n.level];
      if (region) {
        if (gathered != n.level) {
          ProfScope ps(c, 7, 0, (double)Ns * C * 8);
          if ((rc = launch_mask_gather_segment(taps[n.level], perm[n.level], seg_off[n.level], st->label, Ns, C, rows, c->stream))) break;
          gathered = n.level;
        }
        feat = rows;
      }
      if ((rc = ensure(c, c->wct_ws, wct_style_workspace_bytes(C, Ns, n.key)))) break;
      ProfScope ps(c, kind == 2 ? 7 : 5, 0, 0);
      WctCall r = ctx_call(c, kind == 1 ? WCT_MODE_NP : WCT_MODE_TF, WCT_STAGE_ALL);
      r.eps = -1.f;
      if ((rc = launch_style_state(feat, Ns, C, n.key, kind == 2, r, buf))) break;
    }
  }
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { wct_set_error("hipStreamSynchronize failed (prepared style)"); rc = WCT_ERR_HIP; }
  if (!rc) rc = eig_status(c);
  if (rc) {                                               // keep nothing of a failed fill
    hipStreamSynchronize(c->stream);
    for (int g = 0; g < G; ++g)
      for (auto& lv : group[g]->cache)
        for (size_t i = lv.size(); i-- > 0;)
          if (std::find(fresh.begin(), fresh.end(), lv[i].buf) != fresh.end()) { hipFree(lv[i].buf); lv.erase(lv.begin() + i); }
  }
  return rc;
}

// The states `needs` of handle k of the running call (duplicates allowed), one buffer per need in *bufs: the cached ones are stamped
// with the call -- a state the running call uses is never evicted --, the distinct missing ones computed by ONE style_fill
static int style_states(wct_ctx* c, int k, wct_style* st, int kind, const std::vector<StyleNeed>& needs, std::vector<const float*>* bufs) {
  std::vector<StyleNeed> missing;
  for (const StyleNeed& n : needs) {
    StyleState* e = state_find(st, n.level, n.key, kind);
    if (e) e->stamp = c->style_clock;
    else if (std::none_of(missing.begin(), missing.end(), [&](const StyleNeed& m) { return m.level == n.level && same_key(m.key, n.key); }))
      missing.push_back(n);
  }
  TRY(style_fill(c, &st, 1, kind, &missing));
  bufs->clear();
  for (const StyleNeed& n : needs) {
    StyleState* e = state_find(st, n.level, n.key, kind);
    if (!e) { wct_set_error("prepared style %d: the state of relu%d_1 is gone", k, n.level); return WCT_ERR_STATE; }
    bufs->push_back(e->buf);
  }
  return WCT_OK;
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

// The checks of the wct_style_prepare* calls before anything is staged (their pointers checked by the caller): the flags, the
// levels (*set, *deepest), the size of the style, the encoder; then stale failures are reported
static int prepare_checks(wct_ctx* c, int Hs, int Ws, const int* levels, int n_levels, unsigned flags, unsigned* set, int* deepest) {
  TRY(style_flags_ok(flags));
  *set = 0; *deepest = 0;
  for (int i = 0; i < n_levels; ++i) {
    ARG_CHECK(levels[i] >= 1 && levels[i] <= 5);
    *set |= 1u << levels[i];
    *deepest = std::max(*deepest, levels[i]);
  }
  TRY(check_min_size("style", Hs, Ws, *deepest));
  if (!c->enc_loaded) { wct_set_error("encoder weights not set (wct_set_encoder)"); return WCT_ERR_STATE; }
  HIP_TRY(hipSetDevice(c->device));
  return eig_stale(c);
}

// the source of a handle on the device: the host image (uint8, or fp32 with WCT_FLAG_IMAGES_F32) as fp32, and the label map if any
static int source_upload(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const uint8_t* map, unsigned flags,
                         std::shared_ptr<StyleSource>* out) {
  auto src = std::make_shared<StyleSource>();
  const size_t n = (size_t)Hs * Ws * 3;
  HIP_TRY(hipMalloc((void**)&src->img, n * sizeof(float)));
  void* ds;
  TRY(stage_in(c, 1, style, n * sample_bytes(flags), &ds));
  if (flags & WCT_FLAG_IMAGES_F32) HIP_TRY(hipMemcpyAsync(src->img, ds, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  else TRY(launch_u8_to_f32((const uint8_t*)ds, src->img, n, c->stream));
  if (map) {
    HIP_TRY(hipMalloc((void**)&src->map, (size_t)Hs * Ws));
    HIP_TRY(hipMemcpyAsync(src->map, map, (size_t)Hs * Ws, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));             // (the caller's map may go once the call returns)
  }
  *out = std::move(src);
  return WCT_OK;
}

// a handle of `set` on src (label < 0: the whole image; else the rows of `label` of the host map) with its rows per level counted;
// *small: the first served level at which a region has fewer than 2 rows (0: none), its count in *small_rows
static std::unique_ptr<wct_style> new_handle(const std::shared_ptr<StyleSource>& src, int Hs, int Ws, unsigned set, const uint8_t* map,
                                             int label, int* small, int* small_rows) {
  std::unique_ptr<wct_style> st(new wct_style());
  st->Hs = Hs; st->Ws = Ws; st->level_set = set; st->src = src; st->label = label;
  *small = 0;
  for (int l = 1; l <= 5; ++l) {
    if (!(set & (1u << l))) continue;
    int h, w;
    level_dims(Hs, Ws, l, &h, &w);
    st->rows[l] = label < 0 ? h * w : region_count(map, Hs, Ws, h, w, 1 << (l - 1), label);
    if (st->rows[l] < 2 && !*small) { *small = l; *small_rows = st->rows[l]; }
  }
  return st;
}

// the states a handle is prepared with: those of "a content as large as the style", every other key on first use
static std::vector<StyleNeed> prepare_needs(const wct_style* st) {
  std::vector<StyleNeed> needs;
  for (int l = 1; l <= 5; ++l) {
    if (!(st->level_set & (1u << l))) continue;
    int h, w;
    level_dims(st->Hs, st->Ws, l, &h, &w);
    needs.push_back(StyleNeed{l, wct_style_key(LEVEL_C[l], h * w, style_rows(st, l))});
  }
  return needs;
}

// wct_style_prepare (map null) and wct_style_prepare_region
static int style_prepare(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const uint8_t* map, int label, const int* levels, int n_levels,
                         unsigned flags, wct_style** out) {
  unsigned set;
  int deepest, small, small_rows;
  TRY(prepare_checks(c, Hs, Ws, levels, n_levels, flags, &set, &deepest));
  std::shared_ptr<StyleSource> src;
  if (map) {                                              // (counted before anything is staged: a refusal costs no upload)
    std::unique_ptr<wct_style> probe = new_handle(src, Hs, Ws, set, map, label, &small, &small_rows);
    if (small) {
      wct_set_error("style region: label %d has %d rows at relu%d_1 of the %dx%d style (a region needs at least 2 at every level)", label,
                    small_rows, small, Hs, Ws);
      return WCT_ERR_ARG;
    }
  }
  TRY(source_upload(c, style, Hs, Ws, map, flags, &src));
  std::unique_ptr<wct_style> owner = new_handle(src, Hs, Ws, set, map, map ? label : -1, &small, &small_rows);
  wct_style* st = owner.get();
  ++c->style_clock;
  const std::vector<StyleNeed> needs = prepare_needs(st);
  TRY(style_fill(c, &st, 1, style_kind(flags), &needs));
  c->styles.push_back(st);
  *out = owner.release();
  return WCT_OK;
}

extern "C" int wct_style_prepare(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const int* levels, int n_levels, unsigned flags,
                                 wct_style** out) {
  ARG_CHECK(c && style && levels && out && n_levels >= 1 && n_levels <= 16 && Hs >= 2 && Ws >= 2);
  *out = nullptr;
  return style_prepare(c, style, Hs, Ws, nullptr, -1, levels, n_levels, flags, out);
}

static int region_map_ok(const uint8_t* map) {
  if (map) return WCT_OK;
  wct_set_error("style region: no label map");
  return WCT_ERR_ARG;
}

extern "C" int wct_style_prepare_region(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const uint8_t* map, int label, const int* levels,
                                        int n_levels, unsigned flags, wct_style** out) {
  ARG_CHECK(c && style && levels && out && n_levels >= 1 && n_levels <= 16 && Hs >= 2 && Ws >= 2);
  *out = nullptr;
  TRY(region_map_ok(map));
  if (label < 0 || label >= WCT_MIX_MAX) { wct_set_error("style region: label %d, must be 0 .. %d", label, (int)WCT_MIX_MAX - 1); return WCT_ERR_ARG; }
  return style_prepare(c, style, Hs, Ws, map, label, levels, n_levels, flags, out);
}

extern "C" int wct_style_prepare_regions(wct_ctx* c, const uint8_t* style, int Hs, int Ws, const uint8_t* map, int K, const int* levels,
                                         int n_levels, unsigned flags, wct_style** out) {
  ARG_CHECK(c && style && levels && out && n_levels >= 1 && n_levels <= 16 && Hs >= 2 && Ws >= 2);
  if (K < 1 || K > WCT_MIX_MAX) { wct_set_error("style regions: K = %d regions, must be 1 .. %d", K, (int)WCT_MIX_MAX); return WCT_ERR_ARG; }
  for (int k = 0; k < K; ++k) out[k] = nullptr;
  TRY(region_map_ok(map));
  TRY(mask_check(map, (size_t)Hs * Ws, K));
  unsigned set;
  int deepest;
  TRY(prepare_checks(c, Hs, Ws, levels, n_levels, flags, &set, &deepest));
  std::shared_ptr<StyleSource> src;
  TRY(source_upload(c, style, Hs, Ws, map, flags, &src));
  // a handle per region that can carry a style (>= 2 rows at every level); ONE fill for all of them
  std::vector<std::unique_ptr<wct_style>> owners;
  std::vector<wct_style*> group;
  std::vector<std::vector<StyleNeed>> needs;
  std::vector<int> label;
  for (int k = 0; k < K; ++k) {
    int small, small_rows;
    std::unique_ptr<wct_style> st = new_handle(src, Hs, Ws, set, map, k, &small, &small_rows);
    if (small) continue;
    needs.push_back(prepare_needs(st.get()));
    group.push_back(st.get());
    label.push_back(k);
    owners.push_back(std::move(st));
  }
  if (group.empty()) return WCT_OK;
  ++c->style_clock;
  TRY(style_fill(c, group.data(), (int)group.size(), style_kind(flags), needs.data()));
  for (size_t g = 0; g < group.size(); ++g) {
    c->styles.push_back(group[g]);
    out[label[g]] = owners[g].release();
  }
  return WCT_OK;
}

extern "C" int wct_style_rows(wct_ctx* c, const wct_style* st, int level, int* n) {
  ARG_CHECK(c && n);
  TRY(style_live(c, st));
  if (level < 1 || level > 5 || !(st->level_set & (1u << level))) {
    wct_set_error("prepared style: relu%d_1 is not in the handle's level set", level);
    return WCT_ERR_ARG;
  }
  *n = style_rows(st, level);
  return WCT_OK;
}

extern "C" void wct_style_free(wct_ctx* c, wct_style* st) {
  if (!c || !st) return;
  auto it = std::find(c->styles.begin(), c->styles.end(), st);
  if (it == c->styles.end()) return;                      // not ours, or freed already
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);                        // frames in flight may still read its states
  c->styles.erase(it);
  delete st;
}

// The prelude of a content chain on prepared styles: the nc colour samples of the contents as fp32 in [0,1] (*img_c: uint8 ones
// converted into c->img_c), and c->umax with the content's row cleared (the row of wct_stylize_batch_dev)
static int content_prelude(wct_ctx* c, unsigned flags, const void* content, size_t nc, const float** img_c) {
  *img_c = (const float*)content;
  if (!(flags & WCT_FLAG_IMAGES_F32)) {
    TRY(ensure(c, c->img_c, nc * 4));
    ProfScope ps(c, 7, 0, (double)nc * 5);
    TRY(launch_u8_to_f32((const uint8_t*)content, (float*)c->img_c.p, nc, c->stream));
    *img_c = (const float*)c->img_c.p;
  }
  TRY(ensure(c, c->umax, 7 * UROW * sizeof(unsigned)));
  if (fuse_stats()) HIP_TRY(hipMemsetAsync(c->umax.p, 0, UROW * sizeof(unsigned), c->stream));
  return WCT_OK;
}

// stylize_levels' style_at of a chain on handles: no style features (style-swap alone asks for them)
static const float* no_style_at(int, int, int* hs, int* ws) { *hs = *ws = 0; return nullptr; }

// The states of K live handles for every level of `chain`, stamped with the running call (c->style_clock; the missing ones are
// computed, which blocks): style k serves the layout of (content, style k).  refs[i].state[k] is the state of level i, and
// ns[i * WCT_MIX_MAX + k] the rows of style k there (style_rows).
static int chain_states(wct_ctx* c, const Chain& chain, const wct_style* const* styles, int K, int kind, std::vector<WctStyleRef>* refs,
                        std::vector<int>* ns) {
  const int n_levels = (int)chain.lv.size();
  refs->assign(n_levels, WctStyleRef{});
  ns->assign((size_t)n_levels * WCT_MIX_MAX, 0);
  for (int k = 0; k < K; ++k) {
    wct_style* st = const_cast<wct_style*>(styles[k]);
    std::vector<StyleNeed> needs;
    for (int i = 0; i < n_levels; ++i) {
      const ChainLevel& g = chain.lv[i];
      const int rows = style_rows(st, g.l);
      (*ns)[(size_t)i * WCT_MIX_MAX + k] = rows;
      needs.push_back(StyleNeed{g.l, wct_style_key(g.C, g.h * g.w, rows)});
    }
    std::vector<const float*> bufs;
    TRY(style_states(c, k, st, kind, needs, &bufs));
    for (int i = 0; i < n_levels; ++i) (*refs)[i].state[k] = bufs[i];
  }
  return WCT_OK;
}

// The body of the wct_stylize_prepared* calls (their pointer and flag checks done): B contents [B][Hc][Wc][3] on the device, K
// handles; lambda null: one style for all B (K = 1), else the mix weights of K styles (B = 1).  Asynchronous unless a handle
// has to compute a state (style_fill), which happens before anything of the content chain is enqueued.
// smaps (one style): B strength maps [B][Hc][Wc] on the device, sampled by every level at its own stride.
static int stylize_prepared_dev(wct_ctx* c, const void* content, int Hc, int Wc, int B, const wct_style* const* styles, int K,
                                const float* lambda, const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out,
                                wct_warm* warm = nullptr /* with one style (lambda null): start the content solves from it */,
                                const uint8_t* smaps = nullptr) {
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
  TRY(check_levels(c, levels, n_levels, styles, K));
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));

  // the states of every level, before any launch of the content chain
  ++c->style_clock;
  std::vector<WctStyleRef> refs;
  std::vector<int> ns;
  TRY(chain_states(c, chain, styles, K, style_kind(flags), &refs, &ns));

  const float* img_c;
  TRY(content_prelude(c, flags, content, (size_t)B * Hc * Wc * 3, &img_c));
  if (warm && std::find(c->warm_used.begin(), c->warm_used.end(), warm) == c->warm_used.end()) c->warm_used.push_back(warm);
  return stylize_levels(c, img_c, content, B, chain, flags, UROW * sizeof(unsigned), 1, no_style_at,
                        [&](int i, const ChainLevel& g, const WctFeatStats& st) {
                          const int* Ns = &ns[(size_t)i * WCT_MIX_MAX];
                          if (lambda)
                            return run_transform_mix(c, (float*)c->feat_c.p, g.h * g.w, nullptr, Ns, K, lambda, g.C, alpha, flags, -1.f,
                                                     (half_t*)c->wct_out.p, nullptr, nullptr, &st, &refs[i]);
                          WctWarmRef wr = {};
                          if (warm) wr = {warm->basis[g.l], warm->valid[g.l] ? 1 : 0};
                          const WctStrength sm = {smaps, Hc, Wc, g.w, 1 << (g.l - 1)};
                          TRY(run_transform(c, (float*)c->feat_c.p, g.h * g.w, nullptr, Ns[0], g.C, B, alpha, flags, -1.f,
                                            (half_t*)c->wct_out.p, nullptr, nullptr, &st, &refs[i], warm ? &wr : nullptr,
                                            smaps ? &sm : nullptr));
                          if (warm) warm->valid[g.l] = true;     // (the basis of frame B - 1 is enqueued)
                          return (int)WCT_OK;
                        }, out);
}

// host content in, host frame out, around stylize_prepared_dev (B = 1)
static int stylize_prepared_host(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* const* styles, int K,
                                 const float* lambda, const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out,
                                 wct_warm* warm = nullptr) {
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    return stylize_prepared_dev(c, dc, Hc, Wc, 1, styles, K, lambda, levels, n_levels, alpha, flags, frame, warm);
  });
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

// ---------------------------------------------------------------------------
// guided upsampling (guided_up_rule.h): stylize at a working size, deliver at the content's own size.  B full contents
// [B][H][W][3] on the device -> resized to hc x wc (wct_resize_batch_dev; skipped at equal sizes) -> the prepared batch chain and
// its own quantisation -> upsampled against the full contents still resident -> with WCT_FLAG_CONTENT_COLORS recoloured at full
// size against them: the composition of the stand-alone calls, bit for bit.
// ---------------------------------------------------------------------------
static int upsampled_flags_ok(unsigned flags, bool resized) {
  TRY(style_flags_ok(flags));
  if (flags & WCT_FLAG_GUIDED) {
    wct_set_error("upsampled: WCT_FLAG_GUIDED is not served on this path (the upsampling is the guided filter of the frame)");
    return WCT_ERR_ARG;
  }
  if ((flags & WCT_FLAG_IMAGES_F32) && resized) {
    wct_set_error("upsampled: WCT_FLAG_IMAGES_F32 with H x W other than the working size hc x wc (the resize takes uint8 images)");
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

static int stylize_prepared_upsampled_dev(wct_ctx* c, const void* content, int H, int W, int B, int hc, int wc, const wct_style* style,
                                          const int* levels, int n_levels, float alpha, unsigned flags, int radius, int eps_q, int guide,
                                          uint8_t* out) {
  HIP_TRY(hipSetDevice(c->device));
  int h, w;
  TRY(wct_output_size(hc, wc, levels, n_levels, &h, &w));
  TRY(guided_up_check(B, h, w, hc, wc, H, W, radius, eps_q));
  TRY(guided_up_guide_check(guide));
  const bool resized = H != hc || W != wc;
  TRY(upsampled_flags_ok(flags, resized));
  const int f32 = (flags & WCT_FLAG_IMAGES_F32) ? 1 : 0;
  const void* small = content;
  if (resized) {
    TRY(ensure(c, c->up_c, (size_t)B * hc * wc * 3));
    TRY(wct_resize_batch_dev(c, (const uint8_t*)content, H, W, B, hc, wc, (uint8_t*)c->up_c.p));
    small = c->up_c.p;
  }
  TRY(ensure(c, c->up_s, (size_t)B * h * w * 3));
  TRY(stylize_prepared_dev(c, small, hc, wc, B, &style, 1, nullptr, levels, n_levels, alpha, flags & ~(unsigned)WCT_FLAG_CONTENT_COLORS,
                           (uint8_t*)c->up_s.p));
  TRY(run_guided_upsample(c, (const uint8_t*)c->up_s.p, small, content, f32, B, h, w, hc, wc, H, W, radius, eps_q, guide, out));
  if (!(flags & WCT_FLAG_CONTENT_COLORS)) return WCT_OK;
  ProfScope ps(c, 7, 0, (double)B * H * W * 3 * (2 + (f32 ? 4 : 1)));
  return launch_content_colors_u8_any(out, content, f32, B, H, W, H, W, out, c->stream);
}

extern "C" int wct_stylize_prepared_upsampled_guide_batch_dev(wct_ctx* c, const uint8_t* content, int H, int W, int B, int hc, int wc,
                                                              const wct_style* style, const int* levels, int n_levels, float alpha,
                                                              unsigned flags, int radius, int eps_q, int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!content || !out || !levels) { wct_set_error("upsampled: content_dev, out_dev or levels is a null pointer"); return WCT_ERR_ARG; }
  if (B < 1 || B > 32) { wct_set_error("upsampled: B = %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  ARG_CHECK(n_levels >= 1 && n_levels <= 16);
  const size_t n = (size_t)B * H * W * 3 * sample_bytes(flags);
  if (H >= 1 && W >= 1 && (const uint8_t*)content < out + (size_t)B * H * W * 3 && out < (const uint8_t*)content + n) {
    wct_set_error("upsampled: out_dev overlaps content_dev");
    return WCT_ERR_ARG;
  }
  return stylize_prepared_upsampled_dev(c, content, H, W, B, hc, wc, style, levels, n_levels, alpha, flags, radius, eps_q, guide, out);
}

extern "C" int wct_stylize_prepared_upsampled_batch_dev(wct_ctx* c, const uint8_t* content, int H, int W, int B, int hc, int wc,
                                                        const wct_style* style, const int* levels, int n_levels, float alpha,
                                                        unsigned flags, int radius, int eps_q, uint8_t* out) {
  return wct_stylize_prepared_upsampled_guide_batch_dev(c, content, H, W, B, hc, wc, style, levels, n_levels, alpha, flags, radius, eps_q,
                                                        WCT_GUIDE_GREY, out);
}

extern "C" int wct_stylize_prepared_upsampled_guide(wct_ctx* c, const uint8_t* content, int H, int W, int hc, int wc, const wct_style* style,
                                                    const int* levels, int n_levels, float alpha, unsigned flags, int radius, int eps_q,
                                                    int guide, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  if (!content || !out || !levels) { wct_set_error("upsampled: content, out or levels is a null pointer"); return WCT_ERR_ARG; }
  ARG_CHECK(n_levels >= 1 && n_levels <= 16);
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int h, w;
  TRY(wct_output_size(hc, wc, levels, n_levels, &h, &w));
  TRY(guided_up_check(1, h, w, hc, wc, H, W, radius, eps_q));                                  // (before the staging buffers are sized)
  TRY(guided_up_guide_check(guide));
  void* dc;
  TRY(stage_in(c, 0, content, (size_t)H * W * 3 * sample_bytes(flags), &dc));
  TRY(ensure(c, c->stage[2], (size_t)H * W * 3));
  TRY(stylize_prepared_upsampled_dev(c, dc, H, W, 1, hc, wc, style, levels, n_levels, alpha, flags, radius, eps_q, guide,
                                     (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)H * W * 3));
  return eig_status(c);
}

extern "C" int wct_stylize_prepared_upsampled(wct_ctx* c, const uint8_t* content, int H, int W, int hc, int wc, const wct_style* style,
                                              const int* levels, int n_levels, float alpha, unsigned flags, int radius, int eps_q,
                                              uint8_t* out) {
  return wct_stylize_prepared_upsampled_guide(c, content, H, W, hc, wc, style, levels, n_levels, alpha, flags, radius, eps_q, WCT_GUIDE_GREY,
                                              out);
}

// ---------------------------------------------------------------------------
// strength maps (strength_rule.h): the prepared-style calls with a per-pixel style strength -- the chain, the statistics and the
// matrices of every level are the plain call's, the blend of every feature row takes the strength of its pixel
// ---------------------------------------------------------------------------
// the refusals of a strength call before anything is staged: the flags of a prepared style, a map, a content whole-image calls take
static int strength_checks(const uint8_t* smaps, int Hc, int Wc, const int* levels, int n_levels, unsigned flags) {
  TRY(style_flags_ok(flags));
  if (!smaps) { wct_set_error("strength map: no map"); return WCT_ERR_ARG; }
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));
  int band_rows;
  TRY(band_rows_for(chain, &band_rows));
  if (band_rows) {
    wct_set_error("strength map: a %dx%d content passes the limit of one launch at these levels, and the banded call takes no map", Hc, Wc);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

extern "C" int wct_stylize_prepared_strength(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const uint8_t* smap, const wct_style* style,
                                             const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16);
  TRY(strength_checks(smap, Hc, Wc, levels, n_levels, flags));
  TRY(style_live(c, style));
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    TRY(ensure(c, c->mask_in, (size_t)Hc * Wc));
    HIP_TRY(hipMemcpyAsync(c->mask_in.p, smap, (size_t)Hc * Wc, hipMemcpyHostToDevice, c->stream));
    return stylize_prepared_dev(c, dc, Hc, Wc, 1, &style, 1, nullptr, levels, n_levels, alpha, flags, frame, nullptr,
                                (const uint8_t*)c->mask_in.p);
  });
}

// the body of the two batch calls: B maps on the device, asynchronous like wct_stylize_prepared_batch_dev
static int strength_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const uint8_t* smaps, const wct_style* style,
                              const int* levels, int n_levels, float alpha, unsigned flags, wct_warm* warm, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16);
  if (B < 1 || B > 32) { wct_set_error("strength map: a batch of %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  TRY(strength_checks(smaps, Hc, Wc, levels, n_levels, flags));
  return stylize_prepared_dev(c, content, Hc, Wc, B, &style, 1, nullptr, levels, n_levels, alpha, flags, out, warm, smaps);
}

extern "C" int wct_stylize_prepared_strength_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const uint8_t* smaps,
                                                       const wct_style* style, const int* levels, int n_levels, float alpha,
                                                       unsigned flags, uint8_t* out) {
  return strength_batch_dev(c, content, Hc, Wc, B, smaps, style, levels, n_levels, alpha, flags, nullptr, out);
}

extern "C" int wct_stylize_prepared_strength_batch_dev_warm(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const uint8_t* smaps,
                                                            const wct_style* style, const int* levels, int n_levels, float alpha,
                                                            unsigned flags, wct_warm* warm, uint8_t* out) {
  ARG_CHECK(c != nullptr);
  TRY(warm_live(c, warm));
  return strength_batch_dev(c, content, Hc, Wc, B, smaps, style, levels, n_levels, alpha, flags, warm, out);
}

// ---------------------------------------------------------------------------
// banded stylization (banded.hip): one content of any size on a prepared style -- every level encoded and decoded in bands of
// rows, its content statistics pooled over chunks of feature rows.  wct.py:70-106 runs each level over the whole image, as the
// calls above do; where they run, this one gives their frame.
// ---------------------------------------------------------------------------
static int banded_flags_ok(unsigned flags) {
  if (flags & WCT_FLAG_ADAIN) { wct_set_error("banded: WCT_FLAG_ADAIN is not served on this path (whiten-colour transforms only)"); return WCT_ERR_ARG; }
  if (flags & WCT_FLAG_GUIDED) { wct_set_error("banded: WCT_FLAG_GUIDED is not served on this path (filter the frame with wct_guided_filter)"); return WCT_ERR_ARG; }
  return style_flags_ok(flags);
}

static int stylize_prepared_banded_dev(wct_ctx* c, const void* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                       int n_levels, float alpha, unsigned flags, int band_rows, int stat_rows, uint8_t* out) {
  HIP_TRY(hipSetDevice(c->device));
  TRY(style_live(c, style));
  TRY(check_levels(c, levels, n_levels, &style, 1));
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));
  if (band_rows) TRY(band_rows_check(chain, band_rows));
  else {
    TRY(band_rows_for(chain, &band_rows));
    if (!band_rows)                                       // the whole-image call takes this content: one band per level
      for (const ChainLevel& g : chain.lv) band_rows = std::max(band_rows, (g.H + 15) / 16 * 16);
  }
  const int n = (int)chain.lv.size();
  std::vector<int> crows(n), cK(n);
  for (int i = 0; i < n; ++i) TRY(chunk_rule(chain.lv[i].h, chain.lv[i].w, chain.lv[i].C, stat_rows, &crows[i], &cK[i]));

  // the states of every level (the key of the whole-image call: the layout of the whole map against the style), before any launch
  ++c->style_clock;
  std::vector<WctStyleRef> refs;
  std::vector<int> ns;
  TRY(chain_states(c, chain, &style, 1, style_kind(flags), &refs, &ns));

  const float* cur;
  TRY(content_prelude(c, flags, content, (size_t)Hc * Wc * 3, &cur));
  for (int i = 0; i < n; ++i) {
    const ChainLevel& g = chain.lv[i];
    const size_t px = (size_t)g.h * g.w;
    TRY(ensure(c, c->band_f, px * g.C * 4));
    TRY(ensure(c, c->band_g, px * g.C * 2));
    DevBuf& dst = c->img_t[i & 1];
    TRY(ensure(c, dst, (size_t)(g.h << (g.l - 1)) * (g.w << (g.l - 1)) * 3 * 4));
    TRY(run_encoder_banded(c, cur, g.H, g.W, i > 0, g.l, band_rows, (float*)c->band_f.p));
    TRY(run_transform_chunked(c, (float*)c->band_f.p, px, crows[i] * g.w, cK[i], nullptr, ns[(size_t)i * WCT_MIX_MAX], g.C, alpha, flags,
                              -1.f, (half_t*)c->band_g.p, nullptr, nullptr, &refs[i]));
    TRY(run_decoder_banded(c, g.l, (half_t*)c->band_g.p, g.h, g.w, band_rows, (float*)dst.p));
    cur = (float*)dst.p;
  }
  const int H = chain.Ho, W = chain.Wo;
  if (flags & WCT_FLAG_CONTENT_COLORS) {
    const int f32 = (flags & WCT_FLAG_IMAGES_F32) ? 1 : 0;
    ProfScope ps(c, 7, 0, (double)H * W * 3 * 5 + (double)Hc * Wc * 3 * (f32 ? 4 : 1));
    return launch_content_colors_f32(cur, content, f32, 1, H, W, Hc, Wc, out, c->stream);
  }
  ProfScope ps(c, 7, 0, (double)H * W * 3 * 5);
  return launch_f32_to_u8(cur, out, (size_t)H * W * 3, c->stream);
}

extern "C" int wct_stylize_prepared_banded_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                               int n_levels, float alpha, unsigned flags, int band_rows, int stat_rows, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16 && band_rows >= 0 && stat_rows >= 0);
  TRY(banded_flags_ok(flags));
  return stylize_prepared_banded_dev(c, content, Hc, Wc, style, levels, n_levels, alpha, flags, band_rows, stat_rows, out);
}

extern "C" int wct_stylize_prepared_banded(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                           int n_levels, float alpha, unsigned flags, int band_rows, int stat_rows, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16 && band_rows >= 0 && stat_rows >= 0);
  TRY(banded_flags_ok(flags));
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    return stylize_prepared_banded_dev(c, dc, Hc, Wc, style, levels, n_levels, alpha, flags, band_rows, stat_rows, frame);
  });
}

// ---------------------------------------------------------------------------
// texture synthesis (Li et al. 2017, sec. 4.3; webcam.py:191-192 --noise, stylize.py:95-97): seeded noise made on the device,
// then `passes` runs of the prepared chain, each on the frames of the one before it
// ---------------------------------------------------------------------------
extern "C" int wct_texture_size(int H, int W, const int* levels, int n_levels, int passes, int* Ho, int* Wo) {
  ARG_CHECK(Ho && Wo && passes >= 1 && passes <= 16);
  for (int p = 0; p < passes; ++p) TRY(wct_output_size(H, W, levels, n_levels, &H, &W));
  *Ho = H; *Wo = W;
  return WCT_OK;
}

static int texture_flags_ok(unsigned flags) {
  TRY(style_flags_ok(flags));
  if (flags & WCT_FLAG_IMAGES_F32) { wct_set_error("texture: WCT_FLAG_IMAGES_F32 describes input images, and a texture has none"); return WCT_ERR_ARG; }
  if (flags & WCT_FLAG_CONTENT_COLORS) { wct_set_error("texture: WCT_FLAG_CONTENT_COLORS needs a content whose colours could be kept"); return WCT_ERR_ARG; }
  if (flags & WCT_FLAG_GUIDED) { wct_set_error("texture: WCT_FLAG_GUIDED needs a content to guide the filter, and a texture has none"); return WCT_ERR_ARG; }
  return WCT_OK;
}

extern "C" int wct_texture_prepared_batch_dev(wct_ctx* c, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                              const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                                              unsigned flags, uint8_t* out) {
  ARG_CHECK(c && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32 && passes >= 1 && passes <= 16);
  TRY(texture_flags_ok(flags));
  HIP_TRY(hipSetDevice(c->device));
  TRY(style_live(c, style));
  TRY(check_levels(c, levels, n_levels, &style, 1));
  const unsigned long long px = (unsigned long long)(H > 0 ? H : 0) * (unsigned long long)(W > 0 ? W : 0);
  if (px >= (1ull << 31) || px * 3ull * B >= (1ull << 31)) {               // (launch_texture_noise's bound, before its buffer is sized)
    wct_set_error("texture: the noise of %d images of %dx%dx3 passes 2^31 bytes in one call", B, H, W);
    return WCT_ERR_ARG;
  }
  // the two geometries the passes meet: the noise size, and the frame size of pass 1, which every later pass keeps (the deepest
  // level leaves a multiple of its stride, and no level changes such a size)
  Chain first, rest;
  TRY(chain_geometry(H, W, levels, n_levels, &first));
  TRY(chain_geometry(first.Ho, first.Wo, levels, n_levels, &rest));
  // their style states, before the first launch of the chain (one tick: neither geometry evicts the other's), and every buffer
  // of the call's own -- what may block is over when the noise is enqueued
  ++c->style_clock;
  std::vector<WctStyleRef> refs;
  std::vector<int> ns;
  TRY(chain_states(c, first, &style, 1, style_kind(flags), &refs, &ns));
  if (passes > 1) TRY(chain_states(c, rest, &style, 1, style_kind(flags), &refs, &ns));
  const size_t frames = (size_t)B * first.Ho * first.Wo * 3;
  TRY(ensure(c, c->tex_noise, (size_t)B * H * W * 3));
  for (int i = 0; i < 2 && i < passes - 1; ++i) TRY(ensure(c, c->tex[i], frames));
  {
    ProfScope ps(c, 7, 0, (double)B * H * W * 3);
    TRY(launch_texture_noise((uint8_t*)c->tex_noise.p, B, H, W, seed, first_sample, smooth, c->stream));
  }
  const uint8_t* in = (const uint8_t*)c->tex_noise.p;
  for (int p = 0; p < passes; ++p) {
    uint8_t* dst = p == passes - 1 ? out : (uint8_t*)c->tex[p & 1].p;
    TRY(stylize_prepared_dev(c, in, p ? first.Ho : H, p ? first.Wo : W, B, &style, 1, nullptr, levels, n_levels, alpha, flags, dst));
    in = dst;
  }
  return WCT_OK;
}

// host frame out: the B = 1 case of the batch call, blocking
extern "C" int wct_texture_prepared(wct_ctx* c, int H, int W, unsigned seed, unsigned sample, int smooth, const wct_style* style,
                                    const int* levels, int n_levels, int passes, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && out && levels && n_levels >= 1 && n_levels <= 16 && passes >= 1 && passes <= 16);
  TRY(texture_flags_ok(flags));
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  int Ho, Wo;
  TRY(wct_texture_size(H, W, levels, n_levels, passes, &Ho, &Wo));
  TRY(ensure(c, c->stage[2], (size_t)Ho * Wo * 3));
  TRY(wct_texture_prepared_batch_dev(c, H, W, 1, seed, sample, smooth, style, levels, n_levels, passes, alpha, flags,
                                     (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)Ho * Wo * 3));
  return eig_status(c);
}

// ---------------------------------------------------------------------------
// periodic (tileable) stylization and synthesis: every encoder and decoder of the chain runs on the map extended by a halo of its
// own pixels modulo its size (wrap.hip; the halos and the argument in banded.hip), the transform on the tile alone.  The
// reference reflect-pads every conv (model.py:135-139, 245-304) and so cannot make a tile; this is that network on a torus.
// ---------------------------------------------------------------------------
static int wrap_flags_ok(unsigned flags) {
  if (flags & WCT_FLAG_CONTENT_COLORS) {
    wct_set_error("wrap: WCT_FLAG_CONTENT_COLORS is not served on the periodic path");
    return WCT_ERR_ARG;
  }
  if (flags & WCT_FLAG_SWAP5) { wct_set_error("wrap: WCT_FLAG_SWAP5 (style-swap) is not served on the periodic path"); return WCT_ERR_ARG; }
  if (flags & WCT_FLAG_GUIDED) { wct_set_error("wrap: WCT_FLAG_GUIDED is not served on the periodic path (its window stops at the border)"); return WCT_ERR_ARG; }
  return style_flags_ok(flags);
}

// The body of the wrap calls (their pointer and flag checks done): B tiles [B][Hc][Wc][3] on the device (uint8, or fp32 with
// WCT_FLAG_IMAGES_F32), frames of the same size.  Asynchronous unless the handle has to compute a state or a buffer grows, both of
// which happen before the first launch.
static int stylize_prepared_wrap_dev(wct_ctx* c, const void* content, int Hc, int Wc, int B, const wct_style* style, const int* levels,
                                     int n_levels, float alpha, unsigned flags, uint8_t* out) {
  HIP_TRY(hipSetDevice(c->device));
  TRY(style_live(c, style));
  TRY(check_levels(c, levels, n_levels, &style, 1));
  Chain chain;
  TRY(wrap_chain_check(Hc, Wc, levels, n_levels, &chain));

  // the states of every level under the key of the unpadded map (the transform never sees the halo), and every buffer of the call
  ++c->style_clock;
  std::vector<WctStyleRef> refs;
  std::vector<int> ns;
  TRY(chain_states(c, chain, &style, 1, style_kind(flags), &refs, &ns));
  for (const ChainLevel& g : chain.lv) {
    TRY(wrap_encoder_buffers(c, B, g.H, g.W, g.l));
    TRY(wrap_decoder_buffers(c, B, g.h, g.w, g.l));
    TRY(ensure(c, c->wrap_f, (size_t)B * g.h * g.w * g.C * 4));
    TRY(ensure(c, c->wct_out, (size_t)B * g.h * g.w * g.C * 2));
  }
  for (int i = 0; i < 2 && i < (int)chain.lv.size(); ++i) TRY(ensure(c, c->img_t[i], (size_t)B * Hc * Wc * 3 * 4));

  const float* cur;
  TRY(content_prelude(c, flags, content, (size_t)B * Hc * Wc * 3, &cur));
  for (int i = 0; i < (int)chain.lv.size(); ++i) {
    const ChainLevel& g = chain.lv[i];
    // level i>0 encodes clip(previous decoded, 0, 1) (model.py:86): the clamp is in the conv1_1 loader, as in stylize_levels
    TRY(run_encoder_wrap(c, cur, B, g.H, g.W, i > 0, g.l, (float*)c->wrap_f.p));
    TRY(run_transform(c, (float*)c->wrap_f.p, g.h * g.w, nullptr, ns[(size_t)i * WCT_MIX_MAX], g.C, B, alpha, flags, -1.f,
                      (half_t*)c->wct_out.p, nullptr, nullptr, nullptr, &refs[i]));
    float* dst = (float*)c->img_t[i & 1].p;
    TRY(run_decoder_wrap(c, g.l, (half_t*)c->wct_out.p, B, g.h, g.w, dst));
    cur = dst;
  }
  ProfScope ps(c, 7, 0, (double)B * Hc * Wc * 3 * 5);
  return launch_f32_to_u8(cur, out, (size_t)B * Hc * Wc * 3, c->stream);
}

extern "C" int wct_stylize_prepared_wrap_batch_dev(wct_ctx* c, const uint8_t* content, int Hc, int Wc, int B, const wct_style* style,
                                                   const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32);
  TRY(wrap_flags_ok(flags));
  return stylize_prepared_wrap_dev(c, content, Hc, Wc, B, style, levels, n_levels, alpha, flags, out);
}

extern "C" int wct_stylize_prepared_wrap(wct_ctx* c, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                         int n_levels, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && content && out && levels && n_levels >= 1 && n_levels <= 16);
  TRY(wrap_flags_ok(flags));
  Chain chain;
  TRY(wrap_chain_check(Hc, Wc, levels, n_levels, &chain));    // (the size rule, before the content is staged)
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    return stylize_prepared_wrap_dev(c, dc, Hc, Wc, 1, style, levels, n_levels, alpha, flags, frame);
  });
}

// seamless textures: the noise of wct_texture_prepared_batch_dev, then `passes` runs of the wrap chain, each on the frames of the
// one before it; the tile keeps its size through every pass
extern "C" int wct_texture_prepared_wrap_batch_dev(wct_ctx* c, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                                   const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                                                   unsigned flags, uint8_t* out) {
  ARG_CHECK(c && out && levels && n_levels >= 1 && n_levels <= 16 && B >= 1 && B <= 32 && passes >= 1 && passes <= 16);
  TRY(texture_flags_ok(flags));
  HIP_TRY(hipSetDevice(c->device));
  TRY(style_live(c, style));
  TRY(check_levels(c, levels, n_levels, &style, 1));
  Chain chain;
  TRY(wrap_chain_check(H, W, levels, n_levels, &chain));      // (its launch limits keep B * H * W * 3 far below 2^31)
  const size_t frames = (size_t)B * H * W * 3;
  TRY(ensure(c, c->tex_noise, frames));
  for (int i = 0; i < 2 && i < passes - 1; ++i) TRY(ensure(c, c->tex[i], frames));
  {
    ProfScope ps(c, 7, 0, (double)frames);
    TRY(launch_texture_noise((uint8_t*)c->tex_noise.p, B, H, W, seed, first_sample, smooth, c->stream));
  }
  const uint8_t* in = (const uint8_t*)c->tex_noise.p;
  for (int p = 0; p < passes; ++p) {
    uint8_t* dst = p == passes - 1 ? out : (uint8_t*)c->tex[p & 1].p;
    TRY(stylize_prepared_wrap_dev(c, in, H, W, B, style, levels, n_levels, alpha, flags, dst));
    in = dst;
  }
  return WCT_OK;
}

extern "C" int wct_texture_prepared_wrap(wct_ctx* c, int H, int W, unsigned seed, unsigned sample, int smooth, const wct_style* style,
                                         const int* levels, int n_levels, int passes, float alpha, unsigned flags, uint8_t* out) {
  ARG_CHECK(c && out && levels && n_levels >= 1 && n_levels <= 16 && passes >= 1 && passes <= 16);
  TRY(texture_flags_ok(flags));
  Chain chain;
  TRY(wrap_chain_check(H, W, levels, n_levels, &chain));
  HIP_TRY(hipSetDevice(c->device));
  TRY(eig_stale(c));
  TRY(ensure(c, c->stage[2], (size_t)H * W * 3));
  TRY(wct_texture_prepared_wrap_batch_dev(c, H, W, 1, seed, sample, smooth, style, levels, n_levels, passes, alpha, flags,
                                          (uint8_t*)c->stage[2].p));
  TRY(fetch(c, out, c->stage[2].p, (size_t)H * W * 3));
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
  TRY(check_levels(c, levels, n_levels, styles, K));
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));

  // the labels of every level and frame, counted on the host: nk [level][frame][WCT_MIX_MAX]
  const size_t fstride = (size_t)B * WCT_MIX_MAX;
  std::vector<int> nk((size_t)n_levels * fstride), ns((size_t)n_levels * WCT_MIX_MAX);
  for (int i = 0; i < n_levels; ++i) {
    const ChainLevel& g = chain.lv[i];
    for (int f = 0; f < B; ++f)
      mask_counts(masks + (size_t)f * Hc * Wc, Hc, Wc, g.h, g.w, 1 << (g.l - 1), K, &nk[i * fstride + (size_t)f * WCT_MIX_MAX]);
    for (int k = 0; k < K; ++k) ns[(size_t)i * WCT_MIX_MAX + k] = style_rows(styles[k], g.l);
  }

  // the states of every live (level, frame, region), before any launch of the content chain
  const int kind = style_kind(flags);
  ++c->style_clock;
  std::vector<const float*> states((size_t)n_levels * fstride, nullptr), bufs;
  for (int k = 0; k < K; ++k) {
    std::vector<StyleNeed> needs;
    std::vector<size_t> slot;                            // need j is the state of pair slot[j]
    for (int i = 0; i < n_levels; ++i)
      for (int f = 0; f < B; ++f) {
        const size_t at = i * fstride + (size_t)f * WCT_MIX_MAX + k;
        if (nk[at] < 2) continue;
        needs.push_back(StyleNeed{levels[i], wct_style_key(chain.lv[i].C, nk[at], ns[(size_t)i * WCT_MIX_MAX + k])});
        slot.push_back(at);
      }
    TRY(style_states(c, k, const_cast<wct_style*>(styles[k]), kind, needs, &bufs));
    for (size_t j = 0; j < slot.size(); ++j) states[slot[j]] = bufs[j];
  }

  TRY(ensure(c, c->mask_in, (size_t)B * Hc * Wc));
  HIP_TRY(hipMemcpyAsync(c->mask_in.p, masks, (size_t)B * Hc * Wc, hipMemcpyHostToDevice, c->stream));
  const float* img_c;
  TRY(content_prelude(c, flags, content, (size_t)B * Hc * Wc * 3, &img_c));
  return stylize_levels(c, img_c, content, B, chain, flags, UROW * sizeof(unsigned), 1, no_style_at,
                        [&](int i, const ChainLevel& lv, const WctFeatStats&) {
                          const int l = lv.l, C = lv.C, w = lv.w, Nc = lv.h * lv.w;
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
                            TRY(run_stages(c, wct_masked_batch_workspace_bytes(C, Nc, G, gnk, Ns, K), flags, cost, [&](WctCall r) {
                              r.alpha = alpha; r.eps = r.stages ? -1.f : 1e-5f; r.out16 = o16;
                              if (!r.stages) return launch_adain_masked_batch(fc, Nc, G, g, gnk, Ns, K, C, r, slots);
                              return launch_wct_masked_batch(fc, Nc, G, g, gnk, Ns, K, C, r, slots);
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
  return host_frame(c, content, Hc, Wc, levels, n_levels, flags, out, [&](void* dc, uint8_t* frame) {
    return stylize_prepared_masked_dev(c, dc, Hc, Wc, 1, mask, styles, K, levels, n_levels, alpha, flags, frame);
  });
}
