// Banded stylization: contents past the limits of one launch.  The conv kernels address one image's activations with 32-bit
// byte offsets and the transform one feature map the same way, so the whole-image calls refuse a map of 2^31 bytes.  Here a level
// runs in pieces that each stay inside those limits, on the unchanged kernels:
//   the encoder and the decoder band by band -- a band of rows with a halo of real rows reproduces a convolution exactly --,
//   the transform chunk by chunk -- its content side needs a mean and a covariance, which pool exactly over chunks of rows
//   (pool_rule.h); the eigensolve, the spectral tail and the blend then run once, the apply per chunk.
// This unit holds the band plan, the pooling kernels and the band / chunk drivers; the entry points are in api_ops.hip
// (wct_encode_banded, wct_decode_banded, wct_transform_chunked) and api_stylize.hip (wct_stylize_prepared_banded*).
// It also holds the wrap plan and the wrap drivers of periodic synthesis (wrap.hip's kernels): the same halo tables and the same
// argument, the halo filled with the tile's own pixels modulo its size.
#include "api.h"
#include "wct_stages.h"
#include "pool_rule.h"

// ---------------------------------------------------------------------------
// the band plan
// ---------------------------------------------------------------------------
// The halo of a level.  Walk the layer list backwards from one feature row: a 3x3 conv widens the row interval by 1 on both
// sides, a ceil-mode 2x2 pool maps [lo, hi) to [2 lo, 2 hi), a x2 upsample [lo, hi) to [lo / 2, (hi + 1) / 2).
// Encoder (image rows before / after a feature row's first image row): 1 / 1, 4 / 5, 10 / 13, 30 / 37, 70 / 85 for relu1_1 ..
// relu5_1; BAND_RE is that rounded up to a multiple of 16, so that a span starts where the whole-image pass has a pooling
// window, an upsampled pair and a Winograd row pair start.  Decoder (feature rows on either side): 2, 2, 3, 4, 5; a span's first
// row is moved down to an even one for the same reason.  tests/test_banded_cpu.py checks both on the oracle network.
static const int BAND_RE[6] = {0, 16, 16, 16, 48, 96};
static const int BAND_RD[6] = {0, 2, 2, 3, 4, 5};
// The automatic band height is at most this.  Measured on a 4000 x 3000 content at five levels (profiles/banded_bench.json): 84.0,
// 76.7 and 74.1 ms per frame at 512, 1024 and 2048 rows -- the halo rows are a smaller share of a taller band -- with spreads
// below 1 %; nothing taller was measured, and a band's activations grow with it.
constexpr int BAND_ROWS_CAP = 2048;
constexpr size_t LAUNCH_BYTES = WCT_LAUNCH_BYTES; // one map of one launch stays below this (launch_map_fits, common.h)

struct Band { int e0, e1, y0, y1, d0, d1, f0, f1; };   // encoder span, interior (image rows); decoder span, interior (feature rows)

static void band_list(int H, int level, int band_rows, std::vector<Band>* out) {
  const int s = 1 << (level - 1), h = (H + s - 1) / s, Re = BAND_RE[level], Rd = BAND_RD[level];
  out->clear();
  for (long long y = 0; y < H; y += band_rows) {
    Band b;
    b.y0 = (int)y; b.y1 = (int)std::min<long long>(H, y + band_rows);
    b.e0 = std::max(0, b.y0 - Re); b.e1 = (int)std::min<long long>(H, (long long)b.y1 + Re);
    b.f0 = b.y0 / s; b.f1 = b.y1 == H ? h : b.y1 / s;
    b.d0 = std::max(0, b.f0 - Rd) & ~1; b.d1 = std::min(h, b.f1 + Rd);
    out->push_back(b);
  }
}

// does an encoder pass to relu<level>_1 over rows x W pixels stay inside the launch limits (launch_conv3x3's and the
// transform's: the 64-channel full-resolution map -- fp32 where relu1_1 is the tap -- and the fp32 tap)?
static bool enc_fits(long long rows, long long W, int level) {
  const size_t px = (size_t)rows * (size_t)W;
  if (level == 1) return launch_map_fits(px * 64, 4);
  int h, w;
  level_dims((int)rows, (int)W, level, &h, &w);
  return launch_map_fits(px * 64, 2) && launch_map_fits((size_t)h * w * LEVEL_C[level], 4);
}
// the same of a decoder pass from rows x w feature pixels: its 64-channel fp16 maps at the output resolution, and its input
static bool dec_fits(long long rows, long long w, int level) {
  const size_t s = (size_t)1 << (level - 1);
  return launch_map_fits((size_t)rows * s * (size_t)w * s * 64, 2) && launch_map_fits((size_t)rows * (size_t)w * LEVEL_C[level], 2);
}

// "The whole-image call takes this level": what launch_conv3x3, launch_conv3x3_wino and launch_wct check launch by launch with
// the same launch_map_fits, for the largest maps of the H x W input of a level whose feature map is h x w
bool whole_level_fits(int H, int W, int level, int h, int w) {
  return enc_fits(H, W, level) && launch_map_fits((size_t)h * w * LEVEL_C[level], 4) && dec_fits(h, w, level);
}

// does every span of a level's bands fit?
static bool band_fits(int H, int W, int level, int band_rows) {
  const int s = 1 << (level - 1), w = (W + s - 1) / s;
  std::vector<Band> bands;
  band_list(H, level, band_rows, &bands);
  for (const Band& b : bands)
    if (!enc_fits(b.e1 - b.e0, W, level) || !dec_fits(b.d1 - b.d0, w, level)) return false;
  return true;
}

// the automatic band height of a chain: the largest multiple of 16 up to the cap at which every span of every level fits (0: none)
static int auto_band_rows(const Chain& chain) {
  for (int rows = BAND_ROWS_CAP; rows >= 16; rows -= 16) {
    bool ok = true;
    for (const ChainLevel& g : chain.lv) ok = ok && band_fits(g.H, g.W, g.l, rows);
    if (ok) return rows;
  }
  return 0;
}

int band_rows_for(const Chain& chain, int* band_rows) {
  bool whole = true;
  for (const ChainLevel& g : chain.lv) whole = whole && whole_level_fits(g.H, g.W, g.l, g.h, g.w);
  *band_rows = 0;
  if (whole) return WCT_OK;
  *band_rows = auto_band_rows(chain);
  if (*band_rows) return WCT_OK;
  // the widest input whose smallest band -- 16 rows and both halos at full resolution, 64 channels -- still fits one launch
  size_t limit = LAUNCH_BYTES;
  for (const ChainLevel& g : chain.lv)
    limit = std::min(limit, (LAUNCH_BYTES - 1) / ((size_t)(16 + 2 * BAND_RE[g.l]) * 64 * (g.l == 1 ? 4 : 2)));
  wct_set_error("a %dx%d content is too wide for the smallest band of these levels: the width limit is %d pixels", chain.lv[0].H,
                chain.lv[0].W, (int)limit);
  return WCT_ERR_ARG;
}

int band_rows_check(const Chain& chain, int band_rows) {
  if (band_rows < 16 || band_rows % 16) { wct_set_error("band_rows = %d: must be a positive multiple of 16 (or 0: automatic)", band_rows); return WCT_ERR_ARG; }
  for (const ChainLevel& g : chain.lv)
    if (!band_fits(g.H, g.W, g.l, band_rows)) {
      wct_set_error("band_rows = %d: a band of the %dx%d input of relu%d_1 passes 2^31 bytes in one launch", band_rows, g.H, g.W, g.l);
      return WCT_ERR_ARG;
    }
  return WCT_OK;
}

extern "C" int wct_band_rows(int Hc, int Wc, const int* levels, int n_levels, int* band_rows) {
  ARG_CHECK(band_rows != nullptr);
  Chain chain;
  TRY(chain_geometry(Hc, Wc, levels, n_levels, &chain));
  return band_rows_for(chain, band_rows);
}

extern "C" int wct_band_plan(int H, int W, int level, int band_rows, int max_bands, int* n_bands, int* rows) {
  ARG_CHECK(n_bands && level >= 1 && level <= 5 && H >= 2 && W >= 2 && max_bands >= 0 && (rows || !max_bands));
  TRY(check_min_size("image", H, W, level));
  if (band_rows == 0) {
    TRY(wct_band_rows(H, W, &level, 1, &band_rows));
    if (band_rows == 0) band_rows = (H + 15) / 16 * 16;       // the whole-image call takes it: one band
  }
  if (band_rows < 16 || band_rows % 16) { wct_set_error("band_rows = %d: must be a positive multiple of 16 (or 0: automatic)", band_rows); return WCT_ERR_ARG; }
  std::vector<Band> bands;
  band_list(H, level, band_rows, &bands);
  *n_bands = (int)bands.size();
  if ((int)bands.size() > max_bands) {
    if (!max_bands) return WCT_OK;                             // (a query of the count alone)
    wct_set_error("band plan: %d bands, room for %d", (int)bands.size(), max_bands);
    return WCT_ERR_ARG;
  }
  for (size_t k = 0; k < bands.size(); ++k) {
    const Band& b = bands[k];
    const int r[6] = {b.e0, b.e1, b.y0, b.y1, b.d0, b.d1};
    for (int j = 0; j < 6; ++j) rows[k * 6 + j] = r[j];
  }
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// the wrap plan: the same halos around a TILE, filled with the tile's own pixels modulo its size (wrap.hip) -- every layer then
// sees a torus, and the interior of the pass is the periodic network's output
// ---------------------------------------------------------------------------
// Encoder: BAND_RE image pixels on all four sides.  Decoder: BAND_RD feature pixels behind the tile, and BAND_RD rounded up to
// even in front of it, where a band moves its first row down to an even one.  tests/test_wrap_cpu.py checks both on the oracle.
void wrap_halo(int level, int* enc, int* dec_before, int* dec_after) {
  *enc = BAND_RE[level];
  *dec_before = (BAND_RD[level] + 1) & ~1;
  *dec_after = BAND_RD[level];
}

extern "C" int wct_wrap_halo(int level, int* enc, int* dec_before, int* dec_after) {
  ARG_CHECK(enc && dec_before && dec_after && level >= 1 && level <= 5);
  wrap_halo(level, enc, dec_before, dec_after);
  return WCT_OK;
}

// The tile of a wrap chain: every side a multiple of the deepest level's stride (ceil-mode pooling of an odd size is not
// periodic), large enough for that level, and every padded map of every level inside the limits of one launch
int wrap_chain_check(int H, int W, const int* levels, int n_levels, Chain* chain) {
  ARG_CHECK(levels && n_levels >= 1);
  int deepest = 0;
  for (int i = 0; i < n_levels; ++i) { ARG_CHECK(levels[i] >= 1 && levels[i] <= 5); deepest = std::max(deepest, levels[i]); }
  const int m = 1 << (deepest - 1);
  if (H < 1 || W < 1 || H % m || W % m) {
    wct_set_error("wrap: a %dx%d tile with relu%d_1 in the chain: both sides must be multiples of %d (ceil-mode pooling of an odd "
                  "size is not periodic)", H, W, deepest, m);
    return WCT_ERR_ARG;
  }
  TRY(chain_geometry(H, W, levels, n_levels, chain));
  for (const ChainLevel& g : chain->lv) {
    int Re, d0, d1;
    wrap_halo(g.l, &Re, &d0, &d1);
    const long long Hp = (long long)g.H + 2 * Re, Wp = (long long)g.W + 2 * Re;
    if (Hp > 0x7fffffff || Wp > 0x7fffffff || !enc_fits(Hp, Wp, g.l) || !launch_map_fits((size_t)g.h * g.w * g.C, 4) ||
        !dec_fits((long long)g.h + d0 + d1, (long long)g.w + d0 + d1, g.l)) {
      wct_set_error("wrap: a %dx%d tile with its halo of relu%d_1 (%lldx%lld) passes 2^31 bytes in one launch", g.H, g.W, g.l, Hp, Wp);
      return WCT_ERR_ARG;
    }
  }
  return WCT_OK;
}

extern "C" int wct_wrap_check(int H, int W, const int* levels, int n_levels) {
  Chain chain;
  return wrap_chain_check(H, W, levels, n_levels, &chain);
}

// ---------------------------------------------------------------------------
// the band drivers: slices of the full maps through run_encoder / run_decoder, interiors copied device to device
// ---------------------------------------------------------------------------
static int copy_rows(wct_ctx* c, void* dst, const void* src, size_t bytes) {
  ProfScope ps(c, 7, 0, 2.0 * (double)bytes);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
  return WCT_OK;
}

int run_encoder_banded(wct_ctx* c, const float* img, int H, int W, int clamp01, int level, int band_rows, float* F) {
  ARG_CHECK(level >= 1 && level <= 5 && band_rows >= 16 && band_rows % 16 == 0);
  const int s = 1 << (level - 1), C = LEVEL_C[level];
  int h, w;
  level_dims(H, W, level, &h, &w);
  std::vector<Band> bands;
  band_list(H, level, band_rows, &bands);
  size_t tap_bytes = 0;
  for (const Band& b : bands) tap_bytes = std::max(tap_bytes, (size_t)((b.e1 - b.e0 + s - 1) / s) * w * C * 4);
  TRY(ensure(c, c->feat_c, tap_bytes));
  float* taps[6] = {};
  taps[level] = (float*)c->feat_c.p;
  for (const Band& b : bands) {
    ARG_CHECK(enc_fits(b.e1 - b.e0, W, level));
    // a span is a contiguous slice of [H][W][3]: an edge that is the image's gets the image's own reflect pad, an inner one real rows
    TRY(run_encoder(c, img + (size_t)b.e0 * W * 3, 1, b.e1 - b.e0, W, clamp01, level, taps));
    const size_t row = (size_t)w * C;
    TRY(copy_rows(c, F + (size_t)b.f0 * row, taps[level] + (size_t)(b.f0 - b.e0 / s) * row, (size_t)(b.f1 - b.f0) * row * 4));
  }
  return WCT_OK;
}

int run_decoder_banded(wct_ctx* c, int level, const half_t* G, int h, int w, int band_rows, float* img_out) {
  ARG_CHECK(level >= 1 && level <= 5 && band_rows >= 16 && band_rows % 16 == 0 && h >= 2 && w >= 2);
  const int s = 1 << (level - 1), C = LEVEL_C[level];
  std::vector<Band> bands;
  band_list(h * s, level, band_rows, &bands);     // (the bands of an input of h * s rows own the feature rows of any input with h)
  size_t img_bytes = 0;
  for (const Band& b : bands) img_bytes = std::max(img_bytes, (size_t)(b.d1 - b.d0) * s * w * s * 3 * 4);
  TRY(ensure(c, c->band_img, img_bytes));
  for (const Band& b : bands) {
    ARG_CHECK(dec_fits(b.d1 - b.d0, w, level) && b.d1 - b.d0 >= 2);
    TRY(run_decoder(c, level, G + (size_t)b.d0 * w * C, 1, b.d1 - b.d0, w, (float*)c->band_img.p));
    const size_t row = (size_t)w * s * 3;         // floats per image row
    TRY(copy_rows(c, img_out + (size_t)b.f0 * s * row, (float*)c->band_img.p + (size_t)(b.f0 - b.d0) * s * row,
                  (size_t)(b.f1 - b.f0) * s * row * 4));
  }
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// the wrap drivers: B tiles with their wrap-around halos through run_encoder / run_decoder, the interiors cropped out
// ---------------------------------------------------------------------------
int wrap_encoder_buffers(wct_ctx* c, int B, int H, int W, int level) {
  ARG_CHECK(level >= 1 && level <= 5 && B >= 1 && H >= 1 && W >= 1);
  const int Re = BAND_RE[level];
  const size_t Hp = (size_t)H + 2 * Re, Wp = (size_t)W + 2 * Re;
  TRY(ensure(c, c->wrap_img, (size_t)B * Hp * Wp * 3 * 4));
  return ensure(c, c->feat_c, (size_t)B * (Hp >> (level - 1)) * (Wp >> (level - 1)) * LEVEL_C[level] * 4);
}

int wrap_decoder_buffers(wct_ctx* c, int B, int h, int w, int level) {
  ARG_CHECK(level >= 1 && level <= 5 && B >= 1 && h >= 1 && w >= 1);
  int Re, d0, d1;
  wrap_halo(level, &Re, &d0, &d1);
  const size_t hp = (size_t)h + d0 + d1, wp = (size_t)w + d0 + d1;
  TRY(ensure(c, c->wrap_g, (size_t)B * hp * wp * LEVEL_C[level] * 2));
  return ensure(c, c->wrap_img, (size_t)B * (hp << (level - 1)) * (wp << (level - 1)) * 3 * 4);
}

int run_encoder_wrap(wct_ctx* c, const float* img, int B, int H, int W, int clamp01, int level, float* tap) {
  ARG_CHECK(level >= 1 && level <= 5);
  const int s = 1 << (level - 1), C = LEVEL_C[level], Re = BAND_RE[level];
  ARG_CHECK(H >= s && W >= s && H % s == 0 && W % s == 0);
  const int Hp = H + 2 * Re, Wp = W + 2 * Re;
  ARG_CHECK(enc_fits(Hp, Wp, level));
  TRY(wrap_encoder_buffers(c, B, H, W, level));
  {
    ProfScope ps(c, 7, 0, 2.0 * B * Hp * Wp * 3 * 4);
    TRY(launch_wrap_pad(img, c->wrap_img.p, B, H, W, 3, 4, Re, Re, Re, Re, c->stream));
  }
  float* taps[6] = {};
  taps[level] = (float*)c->feat_c.p;
  TRY(run_encoder(c, (const float*)c->wrap_img.p, B, Hp, Wp, clamp01, level, taps));
  ProfScope ps(c, 7, 0, 2.0 * B * (H / s) * (W / s) * C * 4);
  return launch_wrap_crop(c->feat_c.p, tap, B, Hp / s, Wp / s, C, 4, Re / s, Re / s, H / s, W / s, c->stream);
}

int run_decoder_wrap(wct_ctx* c, int level, const half_t* G, int B, int h, int w, float* img_out) {
  ARG_CHECK(level >= 1 && level <= 5 && h >= 1 && w >= 1);
  const int s = 1 << (level - 1), C = LEVEL_C[level];
  int Re, d0, d1;
  wrap_halo(level, &Re, &d0, &d1);
  const int hp = h + d0 + d1, wp = w + d0 + d1;
  ARG_CHECK(dec_fits(hp, wp, level));
  TRY(wrap_decoder_buffers(c, B, h, w, level));
  {
    ProfScope ps(c, 7, 0, 2.0 * B * hp * wp * C * 2);
    TRY(launch_wrap_pad(G, c->wrap_g.p, B, h, w, C, 2, d0, d1, d0, d1, c->stream));
  }
  TRY(run_decoder(c, level, (const half_t*)c->wrap_g.p, B, hp, wp, (float*)c->wrap_img.p));
  ProfScope ps(c, 7, 0, 2.0 * B * h * s * w * s * 3 * 4);
  return launch_wrap_crop(c->wrap_img.p, img_out, B, hp * s, wp * s, 3, 4, d0 * s, d0 * s, h * s, w * s, c->stream);
}

// ---------------------------------------------------------------------------
// the chunked transform
// ---------------------------------------------------------------------------
// The chunks of an h x w map of C channels: whole feature rows, `rows` of them per chunk (the last chunk: what is left).
// stat_rows = 0: the fewest chunks that keep every launch inside its limit, of equal heights -- one chunk when the map fits;
// stat_rows > 0: that many rows per chunk.  Depends on (h, w, C, stat_rows) alone, never on the bands.
int chunk_rule(int h, int w, int C, int stat_rows, int* rows, int* K) {
  ARG_CHECK(h >= 1 && w >= 2 && stat_rows >= 0);
  const long long rows_max = (long long)((LAUNCH_BYTES - 1) / ((size_t)w * C * 4));
  ARG_CHECK(rows_max >= 1);
  if (stat_rows == 0) {
    *K = (int)((h + rows_max - 1) / rows_max);
    *rows = (h + *K - 1) / *K;
  } else {
    *rows = std::min(stat_rows, h);
    if (*rows > rows_max) { wct_set_error("stat_rows = %d: a chunk of a %d-pixel-wide map of %d channels passes 2^31 bytes (at most %lld rows)", stat_rows, w, C, rows_max); return WCT_ERR_ARG; }
  }
  *K = (h + *rows - 1) / *rows;
  return WCT_OK;
}

// running sums: acc [C][C] (double) takes the chunks of one group -- their covariances cov [G][C][C], eps = 0, normalised by
// n - 1 -- in order.  One block per matrix row, one thread per column.
__global__ __launch_bounds__(512) void pool_within_kernel(double* acc, const float* cov, const int* n, int G, int C, int first) {
  const int i = blockIdx.x, j = threadIdx.x;
  if (j >= C) return;
  const size_t e = (size_t)i * C + j, cc = (size_t)C * C;
  double a = first ? 0.0 : acc[e];
  for (int g = 0; g < G; ++g) a = wct_pool_within(a, cov[g * cc + e], n[g]);
  acc[e] = a;
}

// the pooled statistics into the content slot of a P = 1 carve: mean [C], the covariance (eps on its diagonal) into A and A0,
// and the fp16 scale that covers every chunk -- the smallest of theirs: each is 2^k for its own largest value
__global__ __launch_bounds__(512) void pool_finish_kernel(const double* acc, const float* means, const float* scales, const int* n, int K,
                                                          int C, float eps, float* mean, float* A, float* A0, float* scale) {
  const int i = blockIdx.x, j = threadIdx.x;
  if (j >= C) return;
  const double mi = wct_pool_mean(means, n, K, C, i), mj = wct_pool_mean(means, n, K, C, j);
  const size_t e = (size_t)i * C + j;
  float v = (float)wct_pool_cov(acc[e], means, n, K, C, i, j, mi, mj);
  if (i == j) v += eps;
  A[e] = v;
  A0[e] = v;
  if (i == 0) {
    mean[j] = (float)mj;
    if (j == 0) {
      float sc = scales[0];
      for (int k = 1; k < K; ++k) sc = fminf(sc, scales[k]);
      *scale = sc;
    }
  }
}

constexpr int CHUNKS_MAX = 4096;                 // chunks per map

// n [K]: the rows of every chunk
__global__ void chunk_rows_kernel(int* n, int K, int n_full, int n_last) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < K) n[k] = k == K - 1 ? n_last : n_full;
}
// What a chunked transform of K chunks (n_full rows each, the last n_last) lays out in its workspace: the tail plan (P = 1: the
// pooled content in slot 0; the style in slot 1, computed or loaded from a prepared state), the plan of one group of at most
// WCT_PLAN_PAIRS chunks (chunk g of the group in slot g, with the layout of its own rows), and what persists across the groups
struct ChunkedPlan {
  SlotPlan tail, group;
  double* acc; float* means; float* scales; int* n;
  size_t total;
};

static void chunked_plan(ChunkedPlan* cp, void* base, int C, int n_full, int n_last, int K, const float* style, int Ns, bool prepared) {
  const int Nc = (int)std::min<long long>((long long)n_full * (K - 1) + n_last, 0x7fffffff);
  char* b = (char*)base;
  size_t off = 0;
  cp->tail = SlotPlan{};
  cp->tail.P = 1; cp->tail.skip = prepared ? WCT_SKIP_STYLE : WCT_SKIP_NONE; cp->tail.nwhite = 1;
  if (!prepared) cp->tail.slot[1] = {style, Ns, pair_layout(C, Nc, Ns)};
  plan_carve(&cp->tail, b, C);
  off += align_up(cp->tail.total);
  const int G = std::min(K, WCT_PLAN_PAIRS);
  cp->group = SlotPlan{};
  cp->group.P = (G + 1) / 2;
  // (its partial buffers: room for the layout of a full chunk and for that of the last one, neither of which bounds the other)
  const PairLayout lf = pair_layout(C, n_full, n_full), ll = pair_layout(C, n_last, n_last);
  for (int g = 0; g < G; ++g) cp->group.slot[g] = {nullptr, n_full, lf};
  cp->group.slot[0].lay = PairLayout{std::max(lf.nslab, ll.nslab), std::max(lf.nsplit, ll.nsplit), lf.ksplit};
  plan_carve(&cp->group, b ? b + off : nullptr, C);
  off += align_up(cp->group.total);
  auto take = [&](size_t bytes) { void* p = b ? b + off : nullptr; off += align_up(bytes); return p; };
  cp->acc = (double*)take((size_t)C * C * sizeof(double));
  cp->means = (float*)take((size_t)K * C * sizeof(float));
  cp->scales = (float*)take((size_t)K * sizeof(float));
  cp->n = (int*)take((size_t)K * sizeof(int));
  cp->total = off;
}

// K >= 2 chunks of content [Nc][C] (Nc = n_full (K - 1) + n_last rows, any size) against one style -- `style` [Ns][C], or a
// prepared state -- in the stages of launch_wct
static int launch_wct_chunked(const float* content, int n_full, int n_last, int K, const float* style, int Ns, int C, const WctCall& r,
                              const WctStyleRef* prep) {
  const int mode = r.mode, stages = r.stages; hipStream_t s = r.stream;
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 512 && K >= 2 && K <= CHUNKS_MAX && n_full >= 2 && n_last >= 2 && Ns >= 2 && (style || prep));
  ARG_CHECK(mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  ChunkedPlan cp;
  chunked_plan(&cp, r.workspace, C, n_full, n_last, K, style, Ns, prep != nullptr);
  ARG_CHECK(r.workspace_bytes >= cp.total);
  ARG_CHECK(launch_map_fits((size_t)std::max(n_full, n_last) * C, 4) && plan_fits(cp.tail, C));
  const WctCarve& w = cp.tail.w;
  int rc;
  if (stages & WCT_STAGE_COV) {
    if (!prep && (rc = launch_plan_stats(cp.tail, C, false, true, cov_eps(mode, r.eps), s))) return rc;
    hipLaunchKernelGGL(chunk_rows_kernel, dim3(cdiv(K, 256)), dim3(256), 0, s, cp.n, K, n_full, n_last);
    HIP_TRY(hipGetLastError());
    for (int k0 = 0; k0 < K; k0 += WCT_PLAN_PAIRS) {
      const int G = std::min(K - k0, WCT_PLAN_PAIRS);
      SlotPlan gp = cp.group;
      gp.P = (G + 1) / 2;
      for (int g = 0; g < 2 * WCT_PLAN_PAIRS; ++g) {
        if (g >= G) { gp.slot[g].n = 0; continue; }
        const int n = k0 + g == K - 1 ? n_last : n_full;
        gp.slot[g] = {content + (size_t)(k0 + g) * n_full * C, n, pair_layout(C, n, n)};
      }
      if ((rc = launch_plan_stats(gp, C, false, true, 0.f, s))) return rc;
      hipLaunchKernelGGL(pool_within_kernel, dim3(C), dim3(C), 0, s, cp.acc, (const float*)gp.w.A0, (const int*)(cp.n + k0), G, C, k0 == 0);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(cp.means + (size_t)k0 * C, gp.w.mean, (size_t)G * C * sizeof(float), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(cp.scales + k0, gp.w.scale, (size_t)G * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(pool_finish_kernel, dim3(C), dim3(C), 0, s, (const double*)cp.acc, (const float*)cp.means, (const float*)cp.scales,
                       (const int*)cp.n, K, C, cov_eps(mode, r.eps), w.mean, w.A, w.A0, w.scale);
    HIP_TRY(hipGetLastError());
  }
  if ((stages & WCT_STAGE_EIG) && (rc = launch_eig_stage(w, C, 1, cp.tail.skip, 1, r.sweeps_dev, r.eig_fail, s))) return rc;
  if (!(stages & WCT_STAGE_APPLY)) return WCT_OK;
  if (prep) {
    WctStyleSlots slots = {};
    slots.state[0] = prep->state[0];
    if ((rc = launch_style_load_slots(slots, 1, w, C, true, s))) return rc;
  }
  if ((rc = launch_spectral_tail(w, C, 1, r.alpha, mode, r.eps, cp.tail.skip, 1, s))) return rc;
  if ((rc = launch_blend(w, C, 1, r.alpha, cp.tail.skip, s))) return rc;
  for (int k = 0; k < K; ++k) {
    const size_t at = (size_t)k * n_full * C;
    if ((rc = launch_apply(w, content + at, k == K - 1 ? n_last : n_full, C, 1, r.out16 ? r.out16 + at : nullptr, r.out32 ? r.out32 + at : nullptr, s)))
      return rc;
  }
  return WCT_OK;
}

// The transform of content [Nc][C] in K chunks of n_full rows (the last: what is left), device pointers.  One chunk IS
// run_transform -- the same layout, the same eps placement, no pooling arithmetic.  sweeps_dev [2] or null.
int run_transform_chunked(wct_ctx* c, const float* fc, size_t Nc, int n_full, int K, const float* fs, int Ns, int C, float alpha,
                          unsigned flags, float eps, half_t* out16, float* out32, int* sweeps_dev, const WctStyleRef* prep) {
  ARG_CHECK(K >= 1 && n_full >= 1 && Nc > (size_t)n_full * (K - 1) && Nc < LAUNCH_BYTES);
  if (flags & WCT_FLAG_ADAIN) { wct_set_error("a chunked transform is a whiten-colour transform: WCT_FLAG_ADAIN is not served"); return WCT_ERR_ARG; }
  if (K == 1) return run_transform(c, fc, (int)Nc, fs, Ns, C, 1, alpha, flags, eps, out16, out32, sweeps_dev, nullptr, prep);
  if (K > CHUNKS_MAX) { wct_set_error("%d chunks: at most %d per map", K, CHUNKS_MAX); return WCT_ERR_ARG; }
  const int n_last = (int)(Nc - (size_t)n_full * (K - 1));
  ChunkedPlan cp;
  chunked_plan(&cp, nullptr, std::max(C, 32), n_full, n_last, K, nullptr, Ns, prep != nullptr);
  const double rows = (double)Nc;
  const StageCost cost = {2.0 * C * C * (rows + (prep ? 0 : Ns)), 2.0 * (rows + (prep ? 0 : Ns)) * C * 4, 2.0 * C * C * rows + 6.0 * C * C * C,
                          rows * C * (4 + (out16 ? 2 : 0) + (out32 ? 4 : 0)), 0};
  return run_stages(c, cp.total, flags, cost, [&](WctCall r) {
    r.alpha = alpha; r.eps = eps; r.out16 = out16; r.out32 = out32; r.sweeps_dev = sweeps_dev;
    return launch_wct_chunked(fc, n_full, n_last, K, fs, Ns, C, r, prep);
  });
}
