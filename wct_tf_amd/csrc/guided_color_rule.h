// Guided smoothing with a colour guide (He, Sun, Tang, "Guided Image Filtering", TPAMI 2013, eqs. 19-21): the stylized frame s
// filtered with the three CONTENT channels as guide, so the frame keeps an edge between two colours of equal luminance, which the
// grey guide of guided_rule.h cannot see.  Where the grey rule divides once per pixel and channel, this one solves a 3 x 3 system.
// Integers only, nothing wider than int64; one rule shared by the kernels of guided_color.hip and by any host program (plain C++).
// Frame, content clamp, window, n, rdiv, WCT_GUIDED_SHIFT and the parameter ranges are those of guided_rule.h.
//   guide   I = (c.R, c.G, c.B) of content pixel (min(y, Hc - 1), min(x, Wc - 1)), each 0 .. 255; i, j index its channels, p those of s
//   F = WCT_GUIDED_COLOR_F = 4: covariances are kept in units of 2^-F grey levels squared; U the 3 x 3 unit matrix
//   pass 1, per pixel: the 21 window sums S_i, S_ij (i <= j), S_p, S_ip                      each <= 16641 * 65025 < 2^31
//     V_ij  = rdiv(2^F (n S_ij - S_i S_j), n^2)           M = V + 2^F eps_q U           c_ip = rdiv(2^F (n S_ip - S_i S_p), n^2)
//     adj   = the symmetric adjugate of M (six entries),  det = sum_j M_0j adj_0j > 0,  u_ip = sum_j adj_ij c_jp
//     k     = max(0, bitlength(det) - 43)                 (so that det >> k < 2^43)
//     a_q[i][p] = rdiv((u_ip >> k) 2^12, det >> k)        >> the arithmetic shift (a floor for either sign)
//     b_q[p]    = rdiv(S_p 2^12 - sum_i a_q[i][p] S_i, n)
//   pass 2: SA_ip = sum a_q[i][p], SB_p = sum b_q[p] over the window (int64);
//           out_p = clamp(rdiv(sum_i SA_ip I_i + SB_p, n 2^12), 0, 255)
//
// Bounds.  Write D = 255^2 / 4 = 16256.25 (the largest variance, and covariance, of values in 0 .. 255), h = 2^-(F+1) (half a unit
// of V, in grey levels squared), eps = eps_q, sigma_p <= 127.5 the window's standard deviation of channel p.
//   V is the exact covariance matrix (positive semi-definite) times 2^F, each entry moved by at most 1/2: a symmetric
//   perturbation of spectral norm <= 3/2 (its Frobenius norm).  So M is positive definite, lambda_min(M) >= 2^F eps - 3/2 >= 14.5,
//   |M_ij| <= sqrt(M_ii M_jj) <= Dm = 2^F (D + 65025) + 1/2 = 1300500.5, off the diagonal |M_ij| = |V_ij| <= Do = 2^F D + 1/2 =
//   260100.5, and |c_ip| <= Do.  det <= M_00 M_11 M_22 (Hadamard) <= Dm^3 = 2.2e18 < 2^61.
//   F stops at 4: with F = 5, Dm^3 = 1.76e19 passes 2^63 at eps_q = 65025.
//   The exact coefficients a* = (Sigma + eps U)^-1 kappa_p (Sigma the guide's covariance, kappa_p = cov(I, p)) satisfy
//   |a*|_2 <= sigma_p / (2 sqrt(eps)): kappa_p = Sigma^(1/2) w with |w|_2 <= sigma_p (the joint covariance of (I, p) is positive
//   semi-definite), and sqrt(l) / (l + eps) <= 1 / (2 sqrt(eps)) for every eigenvalue l >= 0.
//   The rule solves a^ = M^-1 c with M = 2^F (Sigma + eps U + E), c = 2^F (kappa_p + e), |E|_2 <= 3h, |e|_2 <= sqrt(3) h:
//     a^ - a* = (Sigma + eps U + E)^-1 (e - E a*),    |a^ - a*|_2 <= h (sqrt(3) + 3 sigma_p / (2 sqrt(eps))) / (eps - 3h)    (1)
//   At eps = 1, F = 4 this is 6.65, so |u_ip / det| = |a^_i| <= 63.75 + 6.65 = 70.4 =: A -- above the 63.75 of the grey rule, which
//   is why det is brought below 2^43 and not 2^44 (70.4 * 2^44 * 2^13 passes 2^63).  For larger eps both terms shrink.
//   |a_q| <= A 2^12 + 1 < 288400 < 2^19;  |b_q| <= 255 * 2^12 + 3 * 288400 * 255 + 1 < 2.22e8 < 2^28: both int32.
//
// Distance from the float64 filter (np.linalg.solve on the window covariances, the same box), before the clamp.  With
// A_k = a_q / 2^12 and B_k = b_q / 2^12 of window k, B_k = mean_p - A_k . mean_I + beta_k with |beta_k| <= 2^-13, and
//   value - exact = mean_k[(A_k - a*_k) . (I - mean_I,k)] + mean_k[beta_k] + rho,   |rho| <= 1/2 (the last rounding).
//   A_k - a*_k = alpha_k + (a^_k - a*_k): each entry of alpha is at most 2^-13 (the rounding of a_q) + (1 + A) 2^-42 (the shift by k:
//   (u >> k) / (det >> k) differs from u / det by at most (1 + |u / det|) / (det >> k), and det >> k >= 2^42 when k > 0); with
//   |I_i - mean_i| <= 255 the first part gives 3 * 255 * (2^-13 + 2^-35), and (1) with |I - mean_I|_2 <= 255 sqrt(3) the second:
//   distance(eps_q, F) = 1/2 + 2^-13 + 765 (2^-13 + 2^-35) + 255 sqrt(3) h (sqrt(3) + 191.25 / sqrt(eps_q)) / (eps_q - 3h),  h = 2^-(F+1)
//   At F = 4: 0.594 at eps_q = 65025, 0.79 at 650, 6.0 at 65, 2940 at 1.  The last term is a worst case over every guide (a
//   perturbation of the smallest eigenvalue met by a pixel 255 sqrt(3) from the window's mean); measured distances are in
//   DESIGN 4.19 (at most 0.52 but for the two-greys guide at eps_q = 1, where the 2^-F quantisation of a variance of 1 grey level
//   squared shows: up to 1.22).  The bound at eps_q = 1 is above one grey level and F cannot be raised (above), so small eps on nearly flat guides is
//   where this rule is least exact.
// Left out: the subsampled "fast guided filter", radii above 64, a guide other than the content.
#pragma once
#include "guided_rule.h"

#define WCT_GUIDED_COLOR_F 4
#define WCT_GUIDED_COLOR_DET_BITS 43
// the header's bounds of the stored coefficients (tests/emul/guided_color_rule_check.cpp holds the extremes against them)
#define WCT_GUIDED_COLOR_MAX_A 288400
#define WCT_GUIDED_COLOR_MAX_B 222000000
#define WCT_GUIDED_COLOR_SUMS 21     // the window sums of pass 1, in the order of wct_guided_color_terms
#define WCT_GUIDED_COLOR_COEFFS 12   // int32 per pixel between the passes: a_q[i][p] at 3 * i + p, b_q[p] at 9 + p

// the 21 terms a pixel adds to the window sums: I_0..2, then I_i I_j for (i, j) = 00 01 02 11 12 22, then p_0..2, then I_i p at
// 12 + 3 * i + p.  Each <= 65025.
WCT_GUIDED_HD inline void wct_guided_color_terms(const int I[3], const int p[3], unsigned d[WCT_GUIDED_COLOR_SUMS]) {
  d[0] = I[0]; d[1] = I[1]; d[2] = I[2];
  d[3] = I[0] * I[0]; d[4] = I[0] * I[1]; d[5] = I[0] * I[2]; d[6] = I[1] * I[1]; d[7] = I[1] * I[2]; d[8] = I[2] * I[2];
  d[9] = p[0]; d[10] = p[1]; d[11] = p[2];
  for (int i = 0; i < 3; ++i)
    for (int ch = 0; ch < 3; ++ch) d[12 + 3 * i + ch] = I[i] * p[ch];
}

// the bits of det > 0
WCT_GUIDED_HD inline int wct_guided_color_bitlength(int64_t v) { return 64 - __builtin_clzll((unsigned long long)v); }

// pass 1 of one pixel from its 21 window sums (n pixels): o[3 * i + p] = a_q[i][p], o[9 + p] = b_q[p].  *det_bits: bitlength(det)
WCT_GUIDED_HD inline void wct_guided_color_ab(int64_t n, const int64_t S[WCT_GUIDED_COLOR_SUMS], int eps_q,
                                              int32_t o[WCT_GUIDED_COLOR_COEFFS], int* det_bits) {
  const int64_t n2 = n * n, one = (int64_t)1 << WCT_GUIDED_COLOR_F;            // n2 <= 16641^2 = 2.77e8
  // n S_ij, S_i S_j <= 16641^2 * 65025 = 1.81e13, their difference within +-n^2 D = 4.51e12; times 2^F: 7.3e13; rdiv: < 1.5e14
  const int64_t V00 = wct_guided_rdiv(one * (n * S[3] - S[0] * S[0]), n2), V01 = wct_guided_rdiv(one * (n * S[4] - S[0] * S[1]), n2);
  const int64_t V02 = wct_guided_rdiv(one * (n * S[5] - S[0] * S[2]), n2), V11 = wct_guided_rdiv(one * (n * S[6] - S[1] * S[1]), n2);
  const int64_t V12 = wct_guided_rdiv(one * (n * S[7] - S[1] * S[2]), n2), V22 = wct_guided_rdiv(one * (n * S[8] - S[2] * S[2]), n2);
  const int64_t e = one * eps_q;                                               // <= 1040400
  const int64_t M00 = V00 + e, M11 = V11 + e, M22 = V22 + e;                   // 14.5 .. Dm = 1300500.5; |V01|, |V02|, |V12| <= Do = 260100.5
  // the adjugate: every product <= Dm^2 = 1.69e12, every entry within +-2 Dm^2
  const int64_t a00 = M11 * M22 - V12 * V12, a01 = V02 * V12 - V01 * M22, a02 = V01 * V12 - V02 * M11;
  const int64_t a11 = M00 * M22 - V02 * V02, a12 = V01 * V02 - V12 * M00, a22 = M00 * M11 - V01 * V01;
  // M_00 adj_00 <= Dm^3 = 2.2e18; |V_0j adj_0j| <= Do (Do^2 + Do Dm) = 1.06e17 each: every partial sum below 2.42e18 < 2^63 = 9.22e18
  const int64_t det = M00 * a00 + V01 * a01 + V02 * a02;                       // > 0 (M is positive definite), <= Dm^3 < 2^61
  const int bits = wct_guided_color_bitlength(det);
  const int k = bits > WCT_GUIDED_COLOR_DET_BITS ? bits - WCT_GUIDED_COLOR_DET_BITS : 0;
  const int64_t dk = det >> k;                                                 // 2^42 <= dk < 2^43 when k > 0, det itself otherwise
  if (det_bits) *det_bits = bits;
  for (int ch = 0; ch < 3; ++ch) {
    const int64_t c0 = wct_guided_rdiv(one * (n * S[12 + ch] - S[0] * S[9 + ch]), n2);     // |c_i| <= Do
    const int64_t c1 = wct_guided_rdiv(one * (n * S[15 + ch] - S[1] * S[9 + ch]), n2);
    const int64_t c2 = wct_guided_rdiv(one * (n * S[18 + ch] - S[2] * S[9 + ch]), n2);
    // |adj_ii c_i| <= Dm^2 Do = 4.4e17, |adj_ij c_j| <= (Do^2 + Do Dm) Do = 1.06e17: every partial sum below 6.6e17
    const int64_t u[3] = {a00 * c0 + a01 * c1 + a02 * c2, a01 * c0 + a11 * c1 + a12 * c2, a02 * c0 + a12 * c1 + a22 * c2};
    int64_t acc = S[9 + ch] * ((int64_t)1 << WCT_GUIDED_SHIFT);                // S_p 2^12 <= 1.74e10
    for (int i = 0; i < 3; ++i) {
      // |u| <= A det with A = 70.4 (the header): |u >> k| <= A (dk + 1) + 1 < 70.4 * 2^43; times 2^12, doubled in rdiv, plus dk:
      // < 70.4 * 2^56 + 2^43 < 2^62.2
      const int64_t a = wct_guided_rdiv((u[i] >> k) * ((int64_t)1 << WCT_GUIDED_SHIFT), dk);
      o[3 * i + ch] = (int32_t)a;                                              // |a| < 288400
      acc -= a * S[i];                                                         // |a S_i| < 288400 * 16641 * 255 = 1.23e12
    }
    o[9 + ch] = (int32_t)wct_guided_rdiv(acc, n);                              // |acc| < 3.7e12; the quotient below 2.22e8
  }
}

// pass 2 of one pixel and channel before the clamp: SA[i] the window sums of a_q[i][p], SB that of b_q[p], I the pixel's guide
WCT_GUIDED_HD inline int64_t wct_guided_color_value(int64_t n, const int64_t SA[3], int64_t SB, const int I[3]) {
  // |SA| < 16641 * 288400 = 4.8e9, |SB| < 16641 * 2.22e8 = 3.7e12: |sum SA I + SB| < 7.4e12; the divisor n 2^12 <= 6.9e7
  return wct_guided_rdiv(SA[0] * I[0] + SA[1] * I[1] + SA[2] * I[2] + SB, n * (1 << WCT_GUIDED_SHIFT));
}

WCT_GUIDED_HD inline uint8_t wct_guided_color_out(int64_t n, const int64_t SA[3], int64_t SB, const int I[3]) {
  const int64_t v = wct_guided_color_value(n, SA, SB, I);
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
