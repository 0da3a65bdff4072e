// Guided smoothing (He, Sun, Tang, "Guided Image Filtering", ECCV 2010 / TPAMI 2013; the post-step of the fast variant of Li et
// al. 2018, "A Closed-form Solution to Photorealistic Image Stylization"): the stylized frame s filtered with the grey CONTENT as
// guide, so the frame keeps an edge wherever the content has one and is averaged wherever the content is flat.  Integers only:
// with 8-bit inputs every window sum is an exact integer, so the filter is one rule shared by the kernels of guided.hip and by
// any host program (plain C++: nothing of HIP is needed to include this file), and integer addition being associative the
// kernels may form the sums in any order (running sums, prefix differences).
//   s [H][W][3] uint8, c [Hc][Wc][3] uint8, Hc <= H, Wc <= W; output pixel (y, x) reads content pixel (min(y, Hc - 1),
//   min(x, Wc - 1)): the clamp of colors.hip (a frame can be larger than its content, wct_output_size)
//   radius r in 1 .. 64, eps_q in 1 .. 65025 (grey levels squared: eps of the [0,1]^2 convention x 255^2)
//   rdiv(a, b) = floor((2a + b) / (2b)), b > 0: a / b rounded to nearest, halves up, for either sign of a
//   guide   I = (wct_luma256(c) + 128) >> 8                              0 .. 255, never clamps (the weights sum to 256)
//   window  W(y, x) = rows max(0, y - r) .. min(H - 1, y + r) x columns max(0, x - r) .. min(W - 1, x + r), n pixels
//           (the border-normalised box of He et al.'s reference code); n <= 129^2 = 16641
//   pass 1, per pixel and channel p of s:
//     SI = sum I, SII = sum I^2, Sp = sum p, SIp = sum I p over the window        each <= 16641 * 65025 < 2^31
//     cov = n SIp - SI Sp, var = n SII - SI^2 (>= 0, Cauchy-Schwarz), den = var + eps_q n^2
//     a_q = rdiv(cov 2^12, den), b_q = rdiv(Sp 2^12 - a_q SI, n)
//   pass 2: SA = sum a_q, SB = sum b_q over the window; out = clamp(rdiv(SA I + SB, n 2^12), 0, 255)
// Left out: radii above 64.  The colour (3-channel) guide is guided_color_rule.h, the subsampled "fast guided filter"
// guided_up_rule.h.
#pragma once
#include <stdint.h>
#include "colors_rule.h"

#if defined(__HIPCC__)
#define WCT_GUIDED_HD __host__ __device__
#else
#define WCT_GUIDED_HD
#endif

#define WCT_GUIDED_MAX_RADIUS 64
#define WCT_GUIDED_MAX_EPS 65025
#define WCT_GUIDED_SHIFT 12

WCT_GUIDED_HD inline bool wct_guided_params_ok(int radius, int eps_q) {
  return radius >= 1 && radius <= WCT_GUIDED_MAX_RADIUS && eps_q >= 1 && eps_q <= WCT_GUIDED_MAX_EPS;
}

// floor((2a + b) / (2b)), b > 0.  C's / truncates towards zero: one less where a negative numerator leaves a remainder.
// |2a + b| stays below 2^63 for every caller below (their bounds are beside each call).
WCT_GUIDED_HD inline int64_t wct_guided_rdiv(int64_t a, int64_t b) {
  const int64_t num = 2 * a + b, den = 2 * b;
  const int64_t q = num / den;
  return (num % den < 0) ? q - 1 : q;
}

// the guide of one content pixel: 77 r + 150 g + 29 b <= 256 * 255, so (.. + 128) >> 8 <= 255
WCT_GUIDED_HD inline int wct_guided_guide(int r, int g, int b) { return (wct_luma256(r, g, b) + 128) >> 8; }

// the pixels of the window along one axis: position p of an axis of `size`
WCT_GUIDED_HD inline int wct_guided_extent(int p, int size, int radius) {
  const int lo = p - radius < 0 ? 0 : p - radius, hi = p + radius > size - 1 ? size - 1 : p + radius;
  return hi - lo + 1;
}

// pass 1 of one pixel and channel from its window sums (n pixels)
WCT_GUIDED_HD inline void wct_guided_ab(int64_t n, int64_t SI, int64_t SII, int64_t Sp, int64_t SIp, int eps_q, int32_t* a_q,
                                        int32_t* b_q) {
  // n <= 16641, SI, Sp <= n * 255, SII, SIp <= n * 65025: every product below is < 16641^2 * 65025 = 1.81e13
  const int64_t cov = n * SIp - SI * Sp;                       // |cov| <= n^2 * 255^2 / 4 (a covariance of two 0 .. 255 values)
  const int64_t var = n * SII - SI * SI;                       // 0 .. n^2 * 255^2 / 4
  const int64_t den = var + (int64_t)eps_q * n * n;            // n^2 .. n^2 * (16256.25 + 65025) < 2.26e13
  // |cov| 2^12 <= 16641^2 * 16256.25 * 4096 = 1.85e16; doubled in rdiv, plus den: < 3.8e16 < 2^63
  const int64_t a = wct_guided_rdiv(cov * (1 << WCT_GUIDED_SHIFT), den);
  // |cov| / den <= sigma_I sigma_p / (sigma_I^2 + eps_q) <= sigma_p / (2 sqrt(eps_q)) <= 63.75: |a| <= 63.75 * 4096 + 1 < 2^18
  // Sp 2^12 <= 16641 * 255 * 4096 = 1.74e10, |a SI| < 2^18 * 16641 * 255 = 1.12e12; the quotient is below 6.8e7: int32
  const int64_t b = wct_guided_rdiv(Sp * (1 << WCT_GUIDED_SHIFT) - a * SI, n);
  *a_q = (int32_t)a;
  *b_q = (int32_t)b;
}

// pass 2 of one pixel and channel before the clamp: SA, SB the window sums (n pixels) of a_q, b_q, I the pixel's guide
WCT_GUIDED_HD inline int64_t wct_guided_value(int64_t n, int64_t SA, int64_t SB, int I) {
  // |SA| < 16641 * 2^18 = 4.4e9, |SB| < 16641 * 6.8e7 = 1.2e12: |SA I + SB| < 2.3e12; the divisor n 2^12 <= 6.9e7
  return wct_guided_rdiv(SA * I + SB, n * (1 << WCT_GUIDED_SHIFT));
}

WCT_GUIDED_HD inline uint8_t wct_guided_out(int64_t n, int64_t SA, int64_t SB, int I) {
  const int64_t v = wct_guided_value(n, SA, SB, I);
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
