// Guided smoothing with the colour guide (guided_color_rule.h; He, Sun, Tang, "Guided Image Filtering", eqs. 19-21): the stylized
// frames filtered with the three channels of their content as guide -- the two launches and the tiling of guided.hip
// (guided_tile.h), for up to 32 frames.
//   pass 1: s [B][H][W][3] uint8 + c [B][Hc][Wc][3] (uint8, or fp32 in [0,1] quantised by wct_quantise_u8) -> ab [B][H][W][12]
//           int32: a_q[i][p] at 3 i + p, b_q[p] at 9 + p (48 B per pixel, three 16-byte stores)
//   pass 2: ab + c -> out [B][H][W][3] uint8; out may be s (pass 1 has consumed s before pass 2 writes)
// Pass 1 keeps the 21 window sums of the rule per column, mod 2^32: every term is <= 65025, so the true sums stay below 2^31 and
// the prefixes of a row (256 columns x 129 rows x 65025 < 2^31) too, as in guided.hip.  Pass 2 keeps 12 int64 sums
// (window_sums_ab12 of guided_tile.h, which the means pass of guided_up_color.hip shares); launch_guided_color_ab is pass 1 alone,
// for guided_up_color.hip.  The 27
// 64-bit divisions of a pixel and its 3 x 3 solve are the rule's own (plain C++); halo threads leave the row before them.
#include "guided_tile.h"
#include "guided_color_rule.h"

namespace {
constexpr int KS = WCT_GUIDED_COLOR_SUMS, KC = WCT_GUIDED_COLOR_COEFFS;

template <typename CT>
__global__ __launch_bounds__(NT) void guided_color_ab_kernel(const uint8_t* s, const CT* c, int32_t* ab, int H, int W, int Hc, int Wc, int r,
                                                             int eps_q, int strips, int segs) {
  __shared__ unsigned P[KS][NT];
  __shared__ unsigned tot[KS][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x;
  const uint8_t* sb = s + (size_t)pl.b * H * W * 3;
  const CT* cb = c + (size_t)pl.b * Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  unsigned v[KS];                                           // the column's window sums: true values below 2^31, kept mod 2^32
#pragma unroll
  for (int k = 0; k < KS; ++k) v[k] = 0;
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const uint8_t* sp = sb + ((size_t)y * W + x) * 3;
    const CT* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    const int I[3] = {sample(cp), sample(cp + 1), sample(cp + 2)}, p[3] = {sp[0], sp[1], sp[2]};
    unsigned d[KS];
    wct_guided_color_terms(I, p, d);
#pragma unroll
    for (int k = 0; k < KS; ++k) v[k] += add ? d[k] : 0u - d[k];
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);    // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    unsigned w[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) w[k] = v[k];
    block_prefix<unsigned, KS>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) S[k] = (int64_t)(P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0u));
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    int32_t o[KC];
    wct_guided_color_ab(n, S, eps_q, o, nullptr);
    int4* op = reinterpret_cast<int4*>(ab + (((size_t)pl.b * H + y) * W + x) * KC);          // 48 B per pixel: 16-byte aligned
#pragma unroll
    for (int k = 0; k < KC / 4; ++k) op[k] = make_int4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
  }
}

template <typename CT>
__global__ __launch_bounds__(NT) void guided_color_out_kernel(const int32_t* ab, const CT* c, uint8_t* out, int H, int W, int Hc, int Wc,
                                                              int r, int strips, int segs) {
  __shared__ long long P[KC][NT];
  __shared__ long long tot[KC][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int x = pl.x;
  const CT* cb = c + (size_t)pl.b * Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  window_sums_ab12(ab + (size_t)pl.b * H * W * KC, pl, H, W, r, P, tot, [&](int y, auto win) {
    const CT* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    const int I[3] = {sample(cp), sample(cp + 1), sample(cp + 2)};
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    uint8_t* op = out + (((size_t)pl.b * H + y) * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t SA[3] = {win(ch), win(3 + ch), win(6 + ch)};
      op[ch] = wct_guided_color_out(n, SA, win(9 + ch), I);
    }
  });
}

template <typename CT>
int launch_ab(const uint8_t* s, const CT* c, int32_t* ab, int B, int H, int W, int Hc, int Wc, int r, int eps_q, hipStream_t st) {
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const dim3 grid((unsigned)B * strips * segs);
  hipLaunchKernelGGL((guided_color_ab_kernel<CT>), grid, dim3(NT), 0, st, s, c, ab, H, W, Hc, Wc, r, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

template <typename CT>
int launch_out(const int32_t* ab, const CT* c, int B, int H, int W, int Hc, int Wc, int r, uint8_t* out, hipStream_t st) {
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const dim3 grid((unsigned)B * strips * segs);
  hipLaunchKernelGGL((guided_color_out_kernel<CT>), grid, dim3(NT), 0, st, ab, c, out, H, W, Hc, Wc, r, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

int launch_guided_color_ab(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                           int eps_q, void* ab, hipStream_t s) {
  ARG_CHECK(stylized && content && ab);
  if (((uintptr_t)ab & 15) != 0) { wct_set_error("guided filter: the colour guide's workspace must be 16-byte aligned"); return WCT_ERR_ARG; }
  int rc = guided_check(B, Ho, Wo, Hc, Wc, radius, eps_q, GUIDE_COLOR);
  if (rc) return rc;
  if (content_f32) return launch_ab(stylized, (const float*)content, (int32_t*)ab, B, Ho, Wo, Hc, Wc, radius, eps_q, s);
  return launch_ab(stylized, (const uint8_t*)content, (int32_t*)ab, B, Ho, Wo, Hc, Wc, radius, eps_q, s);
}

int launch_guided_color(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                        int eps_q, void* workspace, uint8_t* out, hipStream_t s) {
  ARG_CHECK(stylized && content && workspace && out);
  int rc = launch_guided_color_ab(stylized, content, content_f32, B, Ho, Wo, Hc, Wc, radius, eps_q, workspace, s);
  if (rc) return rc;
  const int32_t* ab = (const int32_t*)workspace;
  if (content_f32) return launch_out(ab, (const float*)content, B, Ho, Wo, Hc, Wc, radius, out, s);
  return launch_out(ab, (const uint8_t*)content, B, Ho, Wo, Hc, Wc, radius, out, s);
}
