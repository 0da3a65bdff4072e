// Guided upsampling (He, Sun, "Fast Guided Filter", 2015): the guided filter's output is a I + b, a linear function of the guide
// per pixel whose coefficients are smooth.  So the coefficients of a SMALL stylized frame against its small content are computed
// at the small size, interpolated, and evaluated against the FULL content: every edge of the full content comes back at full
// sharpness, whatever the ratio.  Integers only, one rule for the kernels of guided_up.hip and any host program (plain C++).
//   s [h][w][3] uint8 the small stylized frame, c [hc][wc][3] the small content (hc <= h, wc <= w, the clamp of guided_rule.h),
//   C [H][W][3] the full content, H >= hc, W >= wc; radius r and eps_q as in guided_rule.h, in pixels of the small frame
//   1. coefficients  a_q, b_q on h x w: pass 1 of guided_rule.h, unchanged (wct_guided_ab)
//   2. means         per small pixel and channel, n, SA, SB the window count and sums of pass 2 of guided_rule.h:
//                    am = rdiv(SA, n), bm = rdiv(SB, n)  in 2^-12 units; only rows < hc and columns < wc are read afterwards
//   3. interpolation per axis (N the full length, m the small CONTENT length hc or wc -- the rows and columns of s beyond the
//                    content are padding --, P the full coordinate), half-pixel centres:
//                      t = clamp((2P + 1) m - N, 0, 2N (m - 1)),  p0 = t div 2N,  f = rdiv((t - p0 2N) 256, 2N)  (0 .. 256),
//                      p1 = min(p0 + 1, m - 1);  the two weights of the axis are 256 - f and f
//                    I = wct_guided_guide(C[Y][X]);  v = sum over the four neighbours k of w_k (am_k I + bm_k), w_k the products
//                    of the axis weights (they sum to 65536);  out = clamp((v + 2^27) >> 28, 0, 255), >> arithmetic: rdiv by 2^28
// A constant small frame gives a_q = 0 and b_q = 2^12 times the constant everywhere: it comes back as that constant at every full
// size.
// At H = hc, W = wc every f is 0 and the result is clamp(rdiv(am I + bm, 2^12)): wct_guided_filter with SA / n and SB / n rounded
// once more before the product.  It is NOT bit-equal to wct_guided_filter; it differs by at most 1 grey level (the extra error is
// (255 * 0.5 + 0.5) 2^-12 = 0.03125 of a level in front of a rounding to nearest).
// Distance from the float64 fast guided filter (same guide, box, eps and half-pixel bilinear map), before the clamp:
//   |rule - float64| <= 0.5 + 256 2^-12 + D 2^-8,   D = max - min of the pixel's four (am_k I + bm_k) 2^-12
//   * 0.5: the final rounding.
//   * a_q = a 2^12 + da, |da| <= 0.5; b_q rounds (Sp 2^12 - a_q SI) / n, so b_q = 2^12 (mp - a mI) - da mI + db, |db| <= 0.5, and
//     a_q I + b_q = 2^12 (a I + b) + da (I - mI) + db: off by at most 255 * 0.5 + 0.5 = 128 units of 2^-12.  Window means keep
//     that bound; am and bm add |dam| I + |dbm| <= 128 more: 256 2^-12 together.  A convex combination (exact weights) keeps it.
//   * the weights: f / 256 is within 2^-9 of the exact fraction on each axis.  Moving one axis' fraction by e moves a bilinear
//     value by at most e times the spread of its four corners: 2 * 2^-9 D = D 2^-8.
// (8-bit weights are kept: on smooth coefficients D is a fraction of a grey level, and the product w_k (am_k I + bm_k) then stays
// where the 2^-12 coefficient roundings already are; finer weights buy nothing the 0.5 of the last rounding does not hide.)
// Left out: down-scaling (H < hc or W < wc), full contents of 2^31 bytes and more.  (The colour guide under upsampling is
// guided_up_color_rule.h, on this header's axis taps and final shift; the temporal box under upsampling is guided_up_time_rule.h.)
#pragma once
#include "guided_rule.h"

#define WCT_GUIDED_UP_WBITS 8                               // weight bits per axis
#define WCT_GUIDED_UP_ONE (1 << WCT_GUIDED_UP_WBITS)

// step 2 of one small pixel and channel: |SA| < 16641 * 2^18, |SB| < 16641 * 6.8e7 = 1.2e12 (guided_rule.h); doubled in rdiv
// plus n: < 2^63.  |am| < 2^18 and |bm| < 6.8e7, the bounds of a_q and b_q: a mean of values within a bound, rounded to nearest.
WCT_GUIDED_HD inline void wct_guided_up_mean(int64_t n, int64_t SA, int64_t SB, int32_t* am, int32_t* bm) {
  *am = (int32_t)wct_guided_rdiv(SA, n);
  *bm = (int32_t)wct_guided_rdiv(SB, n);
}

// step 3 along one axis: full coordinate P of N onto the small content axis of m, 1 <= m <= N < 2^31.
// (2P + 1) m < 2 N m < 2^63; the remainder is below 2N, times 256 below 2^41.
WCT_GUIDED_HD inline void wct_guided_up_axis(int P, int N, int m, int* p0, int* p1, int* f) {
  const int64_t N2 = 2 * (int64_t)N, hi = N2 * (m - 1);
  int64_t t = (2 * (int64_t)P + 1) * m - N;
  t = t < 0 ? 0 : (t > hi ? hi : t);
  const int64_t q = t / N2;                                  // t >= 0: C's division is the floor
  *p0 = (int)q;                                              // <= m - 1
  *f = (int)wct_guided_rdiv((t - q * N2) * WCT_GUIDED_UP_ONE, N2);
  *p1 = q + 1 < m ? (int)q + 1 : m - 1;
}

// the same in 32-bit unsigned arithmetic, for the kernels: needs wct_guided_up_axis32_ok(N, m), which keeps t (< 2 N m) below
// 2^31 and the numerator of f, rem 256 + N with rem < 2N, below 2^32.  rdiv(rem 256, 2N) = floor((rem 256 + N) / 2N).
WCT_GUIDED_HD inline bool wct_guided_up_axis32_ok(int N, int m) {
  return N <= (1 << 22) && 2 * (int64_t)N * m < ((int64_t)1 << 31);
}
WCT_GUIDED_HD inline void wct_guided_up_axis32(int P, int N, int m, int* p0, int* p1, int* f) {
  const uint32_t N2 = 2u * (uint32_t)N, hi = N2 * (uint32_t)(m - 1);
  const int32_t ts = (int32_t)((2u * (uint32_t)P + 1u) * (uint32_t)m) - N;     // (2P + 1) m < 2^31
  const uint32_t t = ts < 0 ? 0u : ((uint32_t)ts > hi ? hi : (uint32_t)ts);
  const uint32_t q = t / N2;
  *p0 = (int)q;
  *f = (int)(((t - q * N2) * (uint32_t)WCT_GUIDED_UP_ONE + (uint32_t)N) / N2);
  *p1 = (int)q + 1 < m ? (int)q + 1 : m - 1;
}

// step 3 of one pixel and channel before the clamp: am[k], bm[k] of the neighbours (y0, x0), (y0, x1), (y1, x0), (y1, x1), the
// axis fractions fy, fx in 0 .. 256, the pixel's guide I.  |am I + bm| < 2^18 * 255 + 6.8e7 < 1.35e8, the weights sum to 65536:
// |v| < 8.9e12.  The kernels form the same integer in another order (integer addition and multiplication are exact).
WCT_GUIDED_HD inline int64_t wct_guided_up_sum(const int32_t am[4], const int32_t bm[4], int fy, int fx, int I) {
  const int64_t wy[2] = {WCT_GUIDED_UP_ONE - fy, fy}, wx[2] = {WCT_GUIDED_UP_ONE - fx, fx};
  int64_t v = 0;
  for (int k = 0; k < 4; ++k) v += wy[k >> 1] * wx[k & 1] * ((int64_t)am[k] * I + bm[k]);
  return v;
}

// the byte of a sum: rdiv(v, 2^28) as an arithmetic shift, |v + 2^27| < 2^44
WCT_GUIDED_HD inline int64_t wct_guided_up_round(int64_t v) {
  return (v + ((int64_t)1 << (WCT_GUIDED_SHIFT + 2 * WCT_GUIDED_UP_WBITS - 1))) >> (WCT_GUIDED_SHIFT + 2 * WCT_GUIDED_UP_WBITS);
}
WCT_GUIDED_HD inline uint8_t wct_guided_up_out(int64_t v) {
  const int64_t o = wct_guided_up_round(v);
  return (uint8_t)(o < 0 ? 0 : (o > 255 ? 255 : o));
}
