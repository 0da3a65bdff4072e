// Temporal guided upsampling: guided upsampling (guided_up_rule.h) with the temporal box of guided_time_rule.h, optionally along
// camera motion (guided_motion_rule.h), where the coefficients are formed -- on the SMALL frames.  The full-size step needs frame
// f's own interpolated means and frame f's full content, nothing else.  Integers only, plain C++ on top of the two headers, which
// are included unchanged: shared by the kernels of guided_up_time.hip and by any host program.
//   a clip of F frames: s [F][h][w][3] uint8 small stylized frames, c [F][hc][wc][3] small contents (hc <= h, wc <= w), C
//   [.][H][W][3] full contents (H >= hc, W >= wc); T = frames on each side, 0 .. 3; radius r and eps_q as in guided_rule.h, in
//   pixels of the small frame; pos [F][2] int32 positions in pixels of the small frame, or NULL: equal positions
//   1. coefficients  a_q, b_q of (f, y, x) on F x h x w: pass 1 of guided_motion_rule.h, unchanged -- wct_guided_ab on the sums
//                    of the shifted 3-D window, n = wct_guided_motion_n.  With equal positions that is pass 1 of
//                    guided_time_rule.h by construction (wct_guided_up_time_n below returns wct_guided_time_n then).
//   2. means         am = rdiv(SA, n), bm = rdiv(SB, n) (wct_guided_up_mean), SA, SB the sums of a_q, b_q and n the count over
//                    the SAME 3-D window of (f, y, x)
//   3. interpolation step 3 of guided_up_rule.h on frame f's own (am, bm) and frame f's full content, unchanged
//                    (wct_guided_up_axis, wct_guided_up_sum, wct_guided_up_out).  No other frame is read at full size.
// Bounds.  The window holds 1 <= n <= (2r + 1)^2 (2T + 1) <= 33025 pixels under wct_guided_time_params_ok (r <= 64 / 51 / 40 / 33
// at T = 0 / 1 / 2 / 3; the own frame, unshifted, always gives n >= 1), so every bound of pass 1 in guided_time_rule.h holds:
// |a_q| < 2^18, |b_q| < 6.8e7.  Then
//   |SA| < 33025 * 2^18 = 8.7e9,  |SB| < 33025 * 6.8e7 = 2.25e12 < 2.3e12;  rdiv doubles the numerator and adds n:
//   2 * 2.3e12 + 33025 < 4.7e12 < 2^63 = 9.2e18
//   |am| < 2^18 and |bm| < 6.8e7: a mean of values within a bound, rounded to nearest, stays within the bound (the bounds are
//   integers).  These are the bounds guided_up_rule.h states for its own means, so every bound of its step 3 (|A| < 2^26,
//   |am I + bm| < 1.35e8, |v| < 8.9e12, the 32-bit axis taps) holds unchanged.
// Identities.
//   * T = 0, or F = 1 at any T: the window is the 2-D box of the own frame (D = 0, n = extent x extent) in steps 1 and 2, so the
//     bytes are those of wct_guided_upsample.
//   * A constant clip (every small stylized pixel the same value v) gives Sp = n v and SIp = v SI, so a_q = 0 and b_q = 2^12 v
//     everywhere, am = 0 and bm = 2^12 v, and the result is v at every full size, whatever the contents and positions.
//   * At H = hc, W = wc every fraction is 0 and the result is clamp(rdiv(am I + bm, 2^12)): wct_guided_filter_time / _motion with
//     SA / n and SB / n rounded once more in front of the product, within 1 grey level of it (the extra error is at most
//     (255 * 0.5 + 0.5) 2^-12 = 0.03125 of a level in front of a rounding to nearest).
//   * Frame f depends on the small frames up to 2T away (step 2 reads coefficients T frames away, each made from frames T further)
//     and on ONE full content, its own: the halo of a chunked clip is 2T SMALL frames.  A halo of T does not give the bytes.
// Distance from the float64 filter (the fast guided filter with the same guide, 3-D shifted window, eps and half-pixel bilinear
// map), before the clamp -- the formula of guided_up_rule.h, whose derivation never uses the window's shape; restated for this one:
//   |rule - float64| <= 0.5 + 256 2^-12 + D 2^-8,   D = max - min of the pixel's four (am_k I + bm_k) 2^-12
//   * 0.5: the final rounding.
//   * a_q = a 2^12 + da, |da| <= 0.5, whatever set of pixels the sums run over.  b_q rounds (Sp 2^12 - a_q SI) / n, so
//     b_q = 2^12 (mp - a mI) - da mI + db, |db| <= 0.5, with mp, mI the means over the window, and for ANY guide value J in 0 .. 255
//     a_q J + b_q = 2^12 (a J + b) + da (J - mI) + db: off by at most 255 * 0.5 + 0.5 = 128 units of 2^-12 (mI is a mean of guide
//     values, so |J - mI| <= 255).  A mean of such values over any window -- 2-D or 3-D, shifted or cut -- keeps the bound; the
//     roundings of am and bm add |dam| J + |dbm| <= 128 more: 256 2^-12 together.  A convex combination with exact weights (they sum
//     to 65536) keeps it.
//   * the weights: f / 256 is within 2^-9 of the exact fraction on each axis; moving one axis' fraction by e moves a bilinear value
//     by at most e times the spread of its four corners: 2 * 2^-9 D = D 2^-8.
// Left out: the colour guide along time, T above 3, per-block, sub-pixel or non-translational motion, fp32 contents, down-scaling.
#pragma once
#include "guided_up_rule.h"
#include "guided_motion_rule.h"

// the parameters of the rule: those of the temporal filter (the radius limit depends on T)
WCT_GUIDED_HD inline bool wct_guided_up_time_params_ok(int radius, int eps_q, int frames_t) {
  return wct_guided_time_params_ok(radius, eps_q, frames_t);
}

// n of (f, y, x) on the small frames: wct_guided_motion_n under positions, wct_guided_time_n (the same number) without
WCT_GUIDED_HD inline int64_t wct_guided_up_time_n(const int32_t* pos, int f, int F, int frames_t, int y, int h, int x, int w, int radius) {
  return pos ? wct_guided_motion_n(pos, f, F, frames_t, y, h, x, w, radius) : wct_guided_time_n(f, F, frames_t, y, h, x, w, radius);
}

// the box of frame g that belongs to the window of (f, y, x): rows [*ya, *yb] and columns [*xa, *xb] of frame g, empty when
// *ya > *yb or *xa > *xb.  What a host program walks; the kernels tile the same sums.
WCT_GUIDED_HD inline void wct_guided_up_time_box(const int32_t* pos, int f, int g, int y, int h, int x, int w, int radius, int* ya,
                                                 int* yb, int* xa, int* xb) {
  const int cy = y + (pos ? pos[2 * g] - pos[2 * f] : 0), cx = x + (pos ? pos[2 * g + 1] - pos[2 * f + 1] : 0);
  *ya = cy - radius < 0 ? 0 : cy - radius;
  *yb = cy + radius > h - 1 ? h - 1 : cy + radius;
  *xa = cx - radius < 0 ? 0 : cx - radius;
  *xb = cx + radius > w - 1 ? w - 1 : cx + radius;
}
