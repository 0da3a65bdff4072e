// Guided upsampling under the colour guide: the rule of guided_up_rule.h (He, Sun, "Fast Guided Filter", 2015) with the
// coefficients of guided_color_rule.h (He, Sun, Tang, "Guided Image Filtering", eqs. 19-21).  The output is sum_i a_i I_i + b per
// channel, linear in the three channels of the guide with smooth coefficients: they are computed on the SMALL pair, interpolated,
// and evaluated against the FULL content, so an edge between two colours of equal luminance comes back at full sharpness, whatever
// the ratio.  Integers only, nothing wider than int64; one rule for the kernels of guided_up_color.hip and any host program
// (plain C++).  Both parents are included unchanged.
//   s [h][w][3] uint8 the small stylized frame, c [hc][wc][3] the small content (hc <= h, wc <= w, the clamp of guided_rule.h),
//   C [H][W][3] the full content, H >= hc, W >= wc; radius r and eps_q as in guided_rule.h, in pixels of the small frame
//   1. coefficients  a_q[i][p], b_q[p] on h x w: pass 1 of guided_color_rule.h, unchanged (wct_guided_color_ab; 12 int32 per small
//                    pixel, a_q[i][p] at 3 i + p, b_q[p] at 9 + p)
//   2. means         per small pixel, n, SA_ip, SB_p the window count and sums of pass 2 of guided_color_rule.h:
//                    am[i][p] = rdiv(SA_ip, n), bm[p] = rdiv(SB_p, n)  in 2^-12 units, in the layout of step 1; only rows < hc and
//                    columns < wc are read afterwards
//   3. interpolation per axis wct_guided_up_axis of guided_up_rule.h, unchanged (the same taps and 8-bit weights;
//                    wct_guided_up_axis32 under the same condition).  I_i the three channels of C[Y][X]:
//                      v_p = sum over the four neighbours k of w_k (sum_i am_k[i][p] I_i + bm_k[p]),  the w_k sum to 65536
//                      out_p = clamp((v_p + 2^27) >> 28, 0, 255), >> arithmetic: wct_guided_up_out
// Bounds.  am and bm are means of values within +-WCT_GUIDED_COLOR_MAX_A (288400) and +-WCT_GUIDED_COLOR_MAX_B (2.22e8), rounded to
// nearest: they stay within them.  |sum_i am_i I_i + bm| <= 3 * 288400 * 255 + 2.22e8 = 4.43e8, and
//   |v| <= 65536 (3 * 288400 * 255 + 2.22e8) < 2.91e13 < 2^45.
// No division at full size.
// A constant small frame gives a_q = 0 and b_q = 2^12 times the constant everywhere (every c_ip is 0, so every u_ip is): it comes
// back as that constant at every full size.
// At H = hc, W = wc every f is 0 and the result is clamp(rdiv(sum_i am_i I_i + bm, 2^12)): wct_guided_filter_guide(...,
// WCT_GUIDE_COLOR) with SA / n and SB / n rounded once more before the products.  It is NOT bit-equal to it; it differs by at most
// 1 grey level (the extra error is (3 * 255 * 0.5 + 0.5) 2^-12 = 0.094 of a level in front of a rounding to nearest).
// Distance from the float64 fast guided filter with the colour guide (np.linalg.solve on the small pair's window covariances,
// window means, half-pixel bilinear interpolation, evaluation against the full content), before the clamp:
//   |rule - float64| <= 0.5 + 766 2^-12 + 765 2^-35 + D 2^-8 + E(eps_q),
//   D = max - min of the pixel's four (sum_i am_k[i] I_i + bm_k) 2^-12,
//   E(eps_q) = 255 sqrt(3) h (sqrt(3) + 191.25 / sqrt(eps_q)) / (eps_q - 3h),  h = 2^-(F+1) = 2^-5
//   * 0.5: the final rounding.
//   * with a^ = M^-1 c the solve of pass 1 in exact arithmetic, a_q = 2^12 a^ + da with |da_i| <= 0.5 + (1 + A) 2^-30 (the rounding
//     and the shift by k, guided_color_rule.h); b_q rounds (S_p 2^12 - sum_i a_q_i S_i) / n, so b_q = 2^12 (mp - a^ . mI) - da . mI
//     + db, |db| <= 0.5, and  a_q . I + b_q = 2^12 (a^ . (I - mI) + mp) + da . (I - mI) + db: off by at most 3 * 255 * 0.5 + 0.5 =
//     383 units of 2^-12, and 765 2^-35 of a level for the shift.  I is the FULL content's pixel here, mI the window's mean of the
//     small content: |I_i - mI_i| <= 255 all the same.  Window means keep that; am and bm add sum_i |dam_i| I_i + |dbm| <= 383
//     more: 766 2^-12 together.  A convex combination (exact weights) keeps it.
//   * the weights: D 2^-8, as in guided_up_rule.h.
//   * E: a^ against the exact a* = (Sigma + eps U)^-1 kappa_p, eq. (1) of guided_color_rule.h, |a^ - a*|_2 <= h (sqrt(3) + 3 sigma_p
//     / (2 sqrt(eps))) / (eps - 3h), met by |I - mI|_2 <= 255 sqrt(3); a bound per window, so window means and the convex
//     combination keep it.
//   E is 0.0005 at eps_q = 65025, 0.2 at 650, 5.4 at 65, 148 at 7 and 2940 at 1: a worst case over every guide, and from eps_q of
//   a few hundred downwards not a useful bound.  Measured: at most 0.55 on every case with eps_q >= 7, with no pixel
//   above the first four terms; at eps_q = 1, r = 1 up to 0.78, and one pixel of a smooth case above the first four terms -- E is
//   needed there.  As in guided_color_rule.h, small eps on nearly flat guides is where this rule is least exact.
// Left out: the temporal box under upsampling, down-scaling (H < hc or W < wc), full contents of 2^31 bytes and more.
#pragma once
#include "guided_color_rule.h"
#include "guided_up_rule.h"

// the header's bound of |v| (tests/emul/guided_up_color_rule_check.cpp holds the extremes against it and the two of the means)
#define WCT_GUIDED_UP_COLOR_MAX_V 29100000000000LL

// step 2 of one small pixel: S[k] the window sums of the twelve coefficients in their stored order, |S| < 16641 * 2.22e8 = 3.7e12;
// doubled in rdiv plus n: < 2^43.  m[k] in the same order.
WCT_GUIDED_HD inline void wct_guided_up_color_mean(int64_t n, const int64_t S[WCT_GUIDED_COLOR_COEFFS], int32_t m[WCT_GUIDED_COLOR_COEFFS]) {
  for (int k = 0; k < WCT_GUIDED_COLOR_COEFFS; ++k) m[k] = (int32_t)wct_guided_rdiv(S[k], n);
}

// step 3 of one pixel and channel p before the clamp: m[k] the twelve means of the neighbours (y0, x0), (y0, x1), (y1, x0),
// (y1, x1), the axis fractions fy, fx in 0 .. 256, the pixel's guide I[3].  Every inner value is within 4.43e8, the weights sum to
// 65536: |v| < 2.91e13.  The kernels form the same integer in another order (integer addition and multiplication are exact).
WCT_GUIDED_HD inline int64_t wct_guided_up_color_sum(const int32_t* const m[4], int p, int fy, int fx, const int I[3]) {
  const int64_t wy[2] = {WCT_GUIDED_UP_ONE - fy, fy}, wx[2] = {WCT_GUIDED_UP_ONE - fx, fx};
  int64_t v = 0;
  for (int k = 0; k < 4; ++k)
    v += wy[k >> 1] * wx[k & 1] * ((int64_t)m[k][p] * I[0] + (int64_t)m[k][3 + p] * I[1] + (int64_t)m[k][6 + p] * I[2] + m[k][9 + p]);
  return v;
}
