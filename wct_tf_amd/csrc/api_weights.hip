// Weight packing and upload: the encoder and decoder filters as the MFMA fragments the conv kernels fetch.
#include "api.h"

int upload(wct_ctx* c, const void* host, size_t bytes, void** dev) {
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
int pack_conv(wct_ctx* c, const float* w_hwio, const float* b, int cin, int cout, ConvLayer* out) {
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
