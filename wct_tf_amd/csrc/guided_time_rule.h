// Temporal guided smoothing: the guided filter of guided_rule.h with its box extended along time, so that a stylized clip is
// averaged over neighbouring frames wherever its CONTENT does not change between them (the flicker of per-frame stylization on
// flat, static areas) and follows the content wherever it moves, as the 2-D filter follows it at a spatial edge.  Integers only,
// the same rule with a 3-D window: plain C++, shared by the kernels of guided_time.hip and by any host program.
//   a clip of F frames: s [F][H][W][3] uint8, c [F][Hc][Wc][3] uint8, Hc <= H, Wc <= W; the guide of frame f at (y, x) is
//   wct_guided_guide of content pixel (f, min(y, Hc - 1), min(x, Wc - 1))
//   T = frames on each side, 0 .. 3; radius r and eps_q as in guided_rule.h
//   window  W(f, y, x) = the box of guided_rule.h at (y, x) in each frame of max(0, f - T) .. min(F - 1, f + T): cut at the
//           clip's ends as it is cut at the image's borders,
//           n = extent(y, H, r) extent(x, W, r) extent(f, F, T) <= (2r + 1)^2 (2T + 1)
//   pass 1: SI, SII, Sp, SIp over W(f, y, x), then wct_guided_ab(n, ..) -> the (a_q, b_q) of (f, y, x)
//   pass 2: SA, SB over the same window, then wct_guided_out(n, SA, SB, I(f, y, x))
// T = 0 is the rule of guided_rule.h.  Box sums are associative: the 3-D sum is the sum over the window's frames of the 2-D sums.
// The limit: (2r + 1)^2 (2T + 1) <= 33025 = floor(2^31 / 65025), so that every pass-1 sum stays below 2^31 (SII, SIp <=
// n * 65025 <= 33025 * 65025 = 2147450625 < 2^31 = 2147483648) and prefix sums kept mod 2^32 give it exactly.  That is
// r <= 64 / 51 / 40 / 33 at T = 0 / 1 / 2 / 3: 129^2 = 16641; 3 * 103^2 = 31827 (3 * 105^2 = 33075 is over); 5 * 81^2 = 32805
// (5 * 83^2 = 34445); 7 * 67^2 = 31423 (7 * 69^2 = 33327).
// What wct_guided_ab and wct_guided_value hold for n <= 33025 (their own comments are for n <= 16641):
//   every product n SIp, SI Sp, n SII, SI^2 <= 33025^2 * 65025 = 7.1e13
//   |cov| <= n^2 255^2 / 4 <= 33025^2 * 16256.25 = 1.78e13; |cov| 2^12 <= 7.3e16
//   den <= n^2 (16256.25 + 65025) = 8.9e13; rdiv's numerator 2 |cov| 2^12 + den < 1.5e17 < 2^63 = 9.2e18
//   |a_q| <= 63.75 * 4096 + 1 < 2^18: a ratio, no n in it
//   Sp 2^12 <= 33025 * 255 * 4096 = 3.5e10, |a_q SI| < 2^18 * 33025 * 255 = 2.2e12; the doubled numerator plus n is < 4.5e12
//   |b_q| <= (255 * 4096 + 2^18 * 255) + 1 < 6.8e7: both terms are per-pixel means, no n in them; int32
//   pass 2: |SA| < 33025 * 2^18 = 8.7e9, |SA I| < 2.21e12, |SB| < 33025 * 6.8e7 = 2.25e12: |SA I + SB| < 4.5e12;
//           the divisor n 2^12 <= 1.36e8, doubled in rdiv: every term far below 2^63
// Left out: T above 3, any motion compensation (guided_motion_rule.h).  The colour guide along time: guided_color_time_rule.h.
#pragma once
#include "guided_rule.h"

#define WCT_GUIDED_TIME_MAX_FRAMES 3
#define WCT_GUIDED_TIME_MAX_WINDOW 33025        // floor(2^31 / 65025)

// the pixels of a full window: (2r + 1)^2 (2T + 1) for r <= 64, T <= 3: at most 129^2 * 7 = 116487
WCT_GUIDED_HD inline int wct_guided_time_window(int radius, int frames_t) {
  return (2 * radius + 1) * (2 * radius + 1) * (2 * frames_t + 1);
}

// the largest radius of `frames_t` frames on each side: 64 / 51 / 40 / 33; 0 for a frames_t outside 0 .. 3
WCT_GUIDED_HD inline int wct_guided_time_radius_limit(int frames_t) {
  if (frames_t < 0 || frames_t > WCT_GUIDED_TIME_MAX_FRAMES) return 0;
  int r = WCT_GUIDED_MAX_RADIUS;
  while (wct_guided_time_window(r, frames_t) > WCT_GUIDED_TIME_MAX_WINDOW) --r;
  return r;
}

WCT_GUIDED_HD inline bool wct_guided_time_params_ok(int radius, int eps_q, int frames_t) {
  return wct_guided_params_ok(radius, eps_q) && frames_t >= 0 && frames_t <= WCT_GUIDED_TIME_MAX_FRAMES &&
         wct_guided_time_window(radius, frames_t) <= WCT_GUIDED_TIME_MAX_WINDOW;
}

// n of (f, y, x): at most WCT_GUIDED_TIME_MAX_WINDOW under wct_guided_time_params_ok
WCT_GUIDED_HD inline int64_t wct_guided_time_n(int f, int F, int frames_t, int y, int H, int x, int W, int radius) {
  return (int64_t)wct_guided_extent(y, H, radius) * wct_guided_extent(x, W, radius) * wct_guided_extent(f, F, frames_t);
}
