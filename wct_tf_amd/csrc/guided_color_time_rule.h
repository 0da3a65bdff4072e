// Temporal guided smoothing with the colour guide: the 3 x 3 rule of guided_color_rule.h over the 3-D, optionally shifted, window
// of guided_motion_rule.h, so that a clip keeps an edge between two colours of equal luminance AND stops flickering on its flat,
// static areas.  No new arithmetic: both headers are included unchanged; plain C++, shared by the kernels of
// guided_color_time.hip and by any host program.
//   a clip of F frames: s [F][H][W][3] uint8, c [F][Hc][Wc][3] uint8, Hc <= H, Wc <= W; the guide of frame f at (y, x) is
//   I = (c.R, c.G, c.B) of content pixel (f, min(y, Hc - 1), min(x, Wc - 1))
//   T = frames on each side, 0 .. 3; radius r and eps_q as in guided_rule.h; positions pos [F][2] as in guided_motion_rule.h
//   window  of (f, y, x): that of guided_motion_rule.h -- in each frame g of max(0, f - T) .. min(F - 1, f + T) the (2r + 1)^2
//           box centred at the shifted pixel (y + Dy, x + Dx), cut at the borders, possibly empty; n = wct_guided_motion_n.
//           Equal positions, or no positions (all zero), give the window and the n of guided_time_rule.h.
//   pass 1: the 21 sums of wct_guided_color_terms over that window, then wct_guided_color_ab(n, S, eps_q, ..) -> the twelve
//           coefficients a_q[i][p], b_q[p] of (f, y, x)
//   pass 2: the 12 coefficient sums SA_ip, SB_p over the same window, then wct_guided_color_out(n, SA, SB, I(f, y, x))
// T = 0, or a clip of one frame, is the rule of guided_color_rule.h.  A frame depends on no frame further than 2T away.
// Limits: those of the grey temporal rule -- wct_guided_time_params_ok, so (2r + 1)^2 (2T + 1) <= 33025 and r <= 64 / 51 / 40 / 33
// at T = 0 .. 3; positions are those wct_motion_bad_step accepts.
//
// What wct_guided_color_ab and wct_guided_color_value hold for n <= 33025 (their own comments are for n <= 16641):
//   every pass-1 sum <= n * 65025 <= 33025 * 65025 = 2147450625 < 2^31: kept mod 2^32, a window sum is exact
//   n S_ij, S_i S_j <= 33025^2 * 65025 = 7.1e13; their difference within +-n^2 D = 33025^2 * 16256.25 = 1.78e13; times 2^F:
//   2.9e14; doubled in rdiv, plus n^2 = 1.1e9: < 5.7e14 < 2^63
//   V, M, c, the adjugate, det, u and a_q are ratios with no n in them: Dm, Do, det < 2^61, k, |u >> k| and |a_q| < 288400 stand
//   S_p 2^12 <= 33025 * 255 * 4096 = 3.5e10; |a_q S_i| < 288400 * 33025 * 255 = 2.43e12; |acc| < 7.4e12, doubled in rdiv < 2^63
//   |b_q| <= 255 * 2^12 + 3 * 288400 * 255 + 1 < 2.22e8: per-pixel means, no n in them; int32
//   pass 2: |SA| < 33025 * 288400 = 9.6e9, |SB| < 33025 * 2.22e8 = 7.4e12: |sum SA I + SB| < 1.5e13; the divisor n 2^12 <=
//           1.36e8, doubled in rdiv: every term far below 2^63
// The distance from the float64 filter (np.linalg.solve on the covariances of the same 3-D shifted box), distance(eps_q, F) of
// guided_color_rule.h, has no n in it and holds unchanged: 0.594 at eps_q = 65025, 0.79 at 650.
// Left out: the colour guide along time under upsampling, fp32 contents, T above 3, per-block or sub-pixel motion, a motion
// estimator on colour (the positions come from the grey guide or from the caller).
#pragma once
#include "guided_color_rule.h"
#include "guided_motion_rule.h"
