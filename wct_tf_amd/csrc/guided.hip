// Guided smoothing (guided_rule.h; He, Sun, Tang, "Guided Image Filtering"): the stylized frames filtered with their grey content
// as guide -- two launches for up to 32 frames.
//   pass 1: s [B][H][W][3] uint8 + c [B][Hc][Wc][3] (uint8, or fp32 in [0,1] quantised by wct_quantise_u8) -> ab [B][H][W][3][2]
//           int32, the (a_q, b_q) of every pixel and channel
//   pass 2: ab + c -> out [B][H][W][3] uint8; out may be s (pass 1 has consumed s before pass 2 writes)
// Output pixel (y, x) takes content pixel (min(y, Hc - 1), min(x, Wc - 1)): the clamp of colors.hip.
// Both passes are box sums over the (2r + 1)^2 window cut at the frame's border, and the rule's integers make them exact in any
// order, so the work of a pixel does not grow with r.  A block of NT = 256 threads owns SEG = 64 rows of a strip of NT - 2r
// columns of one frame; thread t owns column x0 - r + t of the strip with its halo (a column outside the frame holds zeros) and
// keeps that column's vertical window sums in registers: per row it adds the entering row y + r and subtracts the leaving row
// y - r - 1.  A segment warms up over the 2r rows in front of its first window.  Per row the column sums become inclusive prefix
// sums across the block (a shuffle scan per wave, the wave totals through LDS), and the window sum of column t is
// P[t + r] - P[t - r - 1].  Pass 1's sums are below 2^31 per window, and its prefixes (256 columns x 129 rows x 65025 < 2^31)
// are kept mod 2^32; pass 2's are int64 (window_sums_ab of guided_tile.h, which the means pass of guided_up.hip shares).  The nine
// 64-bit divisions of a pixel are the rule's own (plain C++).  launch_guided_ab is pass 1 alone, for guided_up.hip.
#include "guided_tile.h"
#include "guided_rule.h"

namespace {
template <typename CT>
__global__ __launch_bounds__(NT) void guided_ab_kernel(const uint8_t* s, const CT* c, int32_t* ab, int H, int W, int Hc, int Wc, int r,
                                                       int eps_q, int strips, int segs) {
  __shared__ unsigned P[8][NT];
  __shared__ unsigned tot[8][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x;
  const uint8_t* sb = s + (size_t)pl.b * H * W * 3;
  const CT* cb = c + (size_t)pl.b * Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  // the column's window sums SI, SII, Sp[3], SIp[3]: true values below 2^31, kept mod 2^32
  unsigned v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const uint8_t* sp = sb + ((size_t)y * W + x) * 3;
    const CT* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    const unsigned I = (unsigned)wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
    unsigned d[8] = {I, I * I, sp[0], sp[1], sp[2], I * sp[0], I * sp[1], I * sp[2]};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += add ? d[k] : 0u - d[k];
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);    // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    unsigned w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = v[k];
    block_prefix<unsigned, 8>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = (int64_t)(P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0u));
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    int32_t o[6];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) wct_guided_ab(n, S[0], S[1], S[2 + ch], S[5 + ch], eps_q, &o[2 * ch], &o[2 * ch + 1]);
    int32_t* op = ab + (((size_t)pl.b * H + y) * W + x) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) op[k] = o[k];
  }
}

template <typename CT>
__global__ __launch_bounds__(NT) void guided_out_kernel(const int32_t* ab, const CT* c, uint8_t* out, int H, int W, int Hc, int Wc, int r,
                                                        int strips, int segs) {
  __shared__ long long P[6][NT];
  __shared__ long long tot[6][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int x = pl.x;
  const CT* cb = c + (size_t)pl.b * Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  window_sums_ab(ab + (size_t)pl.b * H * W * 6, pl, H, W, r, P, tot, [&](int y, const int64_t (&S)[6]) {
    const CT* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    const int I = wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    uint8_t* op = out + (((size_t)pl.b * H + y) * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) op[ch] = wct_guided_out(n, S[2 * ch], S[2 * ch + 1], I);
  });
}

template <typename CT>
int launch_ab(const uint8_t* s, const CT* c, int32_t* ab, int B, int H, int W, int Hc, int Wc, int r, int eps_q, hipStream_t st) {
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const dim3 grid((unsigned)B * strips * segs);
  hipLaunchKernelGGL((guided_ab_kernel<CT>), grid, dim3(NT), 0, st, s, c, ab, H, W, Hc, Wc, r, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

template <typename CT>
int launch(const uint8_t* s, const CT* c, int32_t* ab, int B, int H, int W, int Hc, int Wc, int r, int eps_q, uint8_t* out,
           hipStream_t st) {
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const dim3 grid((unsigned)B * strips * segs);
  int rc = launch_ab(s, c, ab, B, H, W, Hc, Wc, r, eps_q, st);
  if (rc) return rc;
  hipLaunchKernelGGL((guided_out_kernel<CT>), grid, dim3(NT), 0, st, (const int32_t*)ab, c, out, H, W, Hc, Wc, r, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

int guided_check(int B, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int guide) {
  if (B < 1 || B > 32) { wct_set_error("guided filter: B = %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (Hc < 1 || Wc < 1 || Ho < Hc || Wo < Wc) {
    wct_set_error("guided filter: a %dx%d stylized frame for a %dx%d content (the frame is never the smaller one)", Ho, Wo, Hc, Wc);
    return WCT_ERR_ARG;
  }
  if (!wct_guided_params_ok(radius, eps_q)) {
    wct_set_error("guided filter: radius %d, eps_q %d; the radius is 1 .. %d and eps_q 1 .. %d (grey levels squared)", radius, eps_q,
                  WCT_GUIDED_MAX_RADIUS, WCT_GUIDED_MAX_EPS);
    return WCT_ERR_ARG;
  }
  if (guide != GUIDE_GREY && guide != GUIDE_COLOR) {
    wct_set_error("guided filter: guide %d, must be WCT_GUIDE_GREY (%d) or WCT_GUIDE_COLOR (%d)", guide, GUIDE_GREY, GUIDE_COLOR);
    return WCT_ERR_ARG;
  }
  if ((unsigned long long)B * (unsigned long long)Ho * (unsigned long long)Wo * 3ull >= (1ull << 31)) {
    wct_set_error("guided filter: %d frames of %dx%dx3 pass 2^31 bytes in one call", B, Ho, Wo);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

size_t guided_workspace_bytes(int B, int Ho, int Wo, int guide) {
  return (size_t)B * Ho * Wo * (guide == GUIDE_COLOR ? 12 : 6) * sizeof(int32_t);
}

int launch_guided_ab(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                     int eps_q, void* ab, hipStream_t s) {
  ARG_CHECK(stylized && content && ab);
  int rc = guided_check(B, Ho, Wo, Hc, Wc, radius, eps_q, GUIDE_GREY);
  if (rc) return rc;
  if (content_f32) return launch_ab(stylized, (const float*)content, (int32_t*)ab, B, Ho, Wo, Hc, Wc, radius, eps_q, s);
  return launch_ab(stylized, (const uint8_t*)content, (int32_t*)ab, B, Ho, Wo, Hc, Wc, radius, eps_q, s);
}

int launch_guided_filter(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                         int eps_q, int guide, void* workspace, uint8_t* out, hipStream_t s) {
  ARG_CHECK(stylized && content && workspace && out);
  int rc = guided_check(B, Ho, Wo, Hc, Wc, radius, eps_q, guide);
  if (rc) return rc;
  if (guide == GUIDE_COLOR) return launch_guided_color(stylized, content, content_f32, B, Ho, Wo, Hc, Wc, radius, eps_q, workspace, out, s);
  if (content_f32) return launch(stylized, (const float*)content, (int32_t*)workspace, B, Ho, Wo, Hc, Wc, radius, eps_q, out, s);
  return launch(stylized, (const uint8_t*)content, (int32_t*)workspace, B, Ho, Wo, Hc, Wc, radius, eps_q, out, s);
}
