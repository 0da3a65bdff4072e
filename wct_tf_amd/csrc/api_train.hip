// Decoder training (model.py:123-223, train.py:129-196): one optimiser step, and its data-parallel halves.
#include "api.h"

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
    float* p[4] = {};
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
  // operands, exact products); tests/test_gpu_backward.py rebuilds the saved state layer by layer with that kernel and holds every
  // gradient element to a derived bound, tests/test_gpu_train.py holds the whole chain to 1e-3 .. 1e-2 against autograd
  struct DirectOnly { wct_ctx* c; DirectOnly(wct_ctx* x) : c(x) { c->no_wino = true; } ~DirectOnly() { c->no_wino = false; } } direct_only(c);
  Decoder& d = c->dec[level];
  if (!d.loaded) { wct_set_error("decoder weights for relu%d_1 not set (wct_set_decoder)", level); return WCT_ERR_STATE; }
  const int scale = 1 << (level - 1);
  ARG_CHECK(H % scale == 0 && W % scale == 0 && H / scale >= 2 && W / scale >= 2);   // the decoder returns exactly H x W
  hipStream_t s = c->stream;
  const int C = LEVEL_C[level];
  const int h = H / scale, w = W / scale;
  const int nconv = (int)d.w32.size();
  int tap_idx = -1;
  for (int i = 0; i < 12 && level > 1; ++i) if (ENC_TAP[i] == level) tap_idx = i;

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
        if (ENC_POOL_AFTER[i] && i != tap_idx) {
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
    float* taps[6] = {};
    taps[level] = F;
    TRY(run_encoder(c, X, B, H, W, 0, level, taps));                       // content features (the target of the feature loss)
  }
  TRY(launch_f32_to_f16(F, A0, (size_t)B * h * w * C, s));
  for (auto& ds : dec_steps) {
    if (d.cout[ds.conv] == 3) {
      ConvLastArgs a;
      a.x = ds.in; a.wfrag = d.last_w; a.bias = d.last_b; a.y = D; a.B = B; a.H = ds.h; a.W = ds.w;
      TRY(launch_conv_last(a, s));
    } else {
      TRY(run_conv(c, d.convs[ds.conv], ds.in, ds.out, nullptr, B, ds.h, ds.w, ds.up, 1));
    }
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
