// Temporal guided smoothing along camera motion: the rule of guided_time_rule.h with the window of every neighbouring frame shifted
// by one global integer translation per frame, so that a clip that pans is averaged along the motion, not across it.  Integers
// only, plain C++ on top of guided_time_rule.h: shared by the kernels of guided_motion.hip and by any host program.
//   positions  pos [F][2] int32 (py, px); pos[0] is arbitrary, only differences are used.  The scene point at pixel (y, x) of
//              frame f is at pixel (y + pos[g][0] - pos[f][0], x + pos[g][1] - pos[f][1]) of frame g.  Valid when
//              |pos[f + 1] - pos[f]| <= WCT_MOTION_MAX_RANGE (16) on both axes for every f.
//   window     of (f, y, x): in each frame g of max(0, f - T) .. min(F - 1, f + T) the (2r + 1)^2 box centred at the shifted
//              pixel (y + Dy, x + Dx), cut at the image's borders -- it may be empty:
//              ext(c, L, r) = max(0, min(L - 1, c + r) - max(0, c - r) + 1),  n = sum_g ext(y + Dy, H, r) ext(x + Dx, W, r)
//   pass 1:    SI, SII, Sp, SIp over that window, then wct_guided_ab(n, ..) -> the (a_q, b_q) of (f, y, x)
//   pass 2:    SA, SB over the same window, then wct_guided_out(n, SA, SB, I(f, y, x))
// Equal positions are the rule of guided_time_rule.h by construction (every D is 0, and the sum of equal extents is their product
// with the number of frames).  A frame still depends on no frame further than 2T away: the halo of a chunked clip stays 2T.
// Bounds: the own frame (D = 0) gives n >= 1; each frame gives at most (2r + 1)^2, so n <= (2r + 1)^2 (2T + 1).  A shifted window
// is a subset of a full one: wct_guided_time_params_ok, the 33025 limit and every bound derived in guided_time_rule.h for
// n <= 33025 (the pass-1 sums below 2^31, the products of wct_guided_ab, |a_q| < 2^18, |b_q| < 6.8e7, pass 2) hold unchanged.
// |D| <= 16 T <= 48 on each axis; y + Dy and x + Dx are far inside int.
//
// The estimator, wct_motion_*: one translation per pair of consecutive content frames, by exhaustive integer search.
//   I_f = the grey guide (wct_guided_guide) of content frame f at content size [Hc][Wc]
//   search range R in 1 .. 16; needs Hc, Wc >= 4R (every candidate keeps samples) and Hc Wc <= 2^28
//   candidate d = (dy, dx), |dy|, |dx| <= R: the samples are the (y, x) with both coordinates even inside frame f whose
//              (y + dy, x + dx) is inside frame f + 1;  SAD(d) = sum |I_f(y, x) - I_{f+1}(y + dy, x + dx)|, cnt(d) their number
//   d wins over d' when SAD(d) cnt(d') < SAD(d') cnt(d): the smaller mean, compared without a division.  cnt <= ceil(Hc / 2)
//              ceil(Wc / 2) <= (Hc + 1)(Wc + 1) / 4 < 2^26.1 and SAD <= 255 cnt, so a product is < 255 * 2^52.2 < 2^61 < 2^63: int64
//   at equality the smaller (dy^2 + dx^2, dy, dx) wins, so a flat or an unchanged pair gives (0, 0)
//   pos[0] = (0, 0), pos[f + 1] = pos[f] + d_f
// Left out: per-block or dense motion, sub-pixel shifts, rotation and zoom.  The colour guide along time and along motion:
// guided_color_time_rule.h.
#pragma once
#include "guided_time_rule.h"

#define WCT_MOTION_MAX_RANGE 16                  // the largest step between two frames, and the largest search range
#define WCT_MOTION_MAX_PIXELS (1 << 28)          // Hc Wc of the estimator

// ext of the header: the pixels of a window centred at c (any integer) along an axis of `size`; 0 when it lies outside
WCT_GUIDED_HD inline int wct_motion_extent(int c, int size, int radius) {
  const int lo = c - radius < 0 ? 0 : c - radius, hi = c + radius > size - 1 ? size - 1 : c + radius;
  return hi >= lo ? hi - lo + 1 : 0;
}

// every step of pos [F][2] within WCT_MOTION_MAX_RANGE: -1, or the first f whose step to f + 1 is not
WCT_GUIDED_HD inline int wct_motion_bad_step(const int32_t* pos, int F) {
  for (int f = 0; f + 1 < F; ++f)
    for (int k = 0; k < 2; ++k) {
      const int64_t d = (int64_t)pos[2 * (f + 1) + k] - pos[2 * f + k];
      if (d > WCT_MOTION_MAX_RANGE || d < -WCT_MOTION_MAX_RANGE) return f;
    }
  return -1;
}

// n of (f, y, x) under positions pos [F][2]: 1 .. WCT_GUIDED_TIME_MAX_WINDOW under wct_guided_time_params_ok
WCT_GUIDED_HD inline int64_t wct_guided_motion_n(const int32_t* pos, int f, int F, int frames_t, int y, int H, int x, int W, int radius) {
  const int lo = f - frames_t < 0 ? 0 : f - frames_t, hi = f + frames_t > F - 1 ? F - 1 : f + frames_t;
  int64_t n = 0;
  for (int g = lo; g <= hi; ++g)
    n += (int64_t)wct_motion_extent(y + (pos[2 * g] - pos[2 * f]), H, radius) *
         wct_motion_extent(x + (pos[2 * g + 1] - pos[2 * f + 1]), W, radius);
  return n;
}

WCT_GUIDED_HD inline bool wct_motion_search_ok(int range, int Hc, int Wc) {
  return range >= 1 && range <= WCT_MOTION_MAX_RANGE && Hc >= 4 * range && Wc >= 4 * range &&
         (int64_t)Hc * Wc <= WCT_MOTION_MAX_PIXELS;
}

// the even c in [0, size) with c + d in [0, size): at least one for |d| <= size / 4
WCT_GUIDED_HD inline int wct_motion_samples(int d, int size) {
  const int lo = d < 0 ? -d : 0, hi = d > 0 ? size - 1 - d : size - 1;
  return hi >= lo ? hi / 2 - (lo + 1) / 2 + 1 : 0;
}

// cnt(d) of the header
WCT_GUIDED_HD inline int64_t wct_motion_count(int dy, int dx, int Hc, int Wc) {
  return (int64_t)wct_motion_samples(dy, Hc) * wct_motion_samples(dx, Wc);
}

// does candidate (dy, dx) with (sad, cnt) win over (dy2, dx2) with (sad2, cnt2)?  Both counts positive; products < 2^61
WCT_GUIDED_HD inline bool wct_motion_better(int64_t sad, int64_t cnt, int dy, int dx, int64_t sad2, int64_t cnt2, int dy2, int dx2) {
  const int64_t a = sad * cnt2, b = sad2 * cnt;
  if (a != b) return a < b;
  const int q = dy * dy + dx * dx, q2 = dy2 * dy2 + dx2 * dx2;
  if (q != q2) return q < q2;
  if (dy != dy2) return dy < dy2;
  return dx < dx2;
}

// SAD(d) of guide planes I0, I1 [Hc][Wc]
WCT_GUIDED_HD inline int64_t wct_motion_sad(const uint8_t* I0, const uint8_t* I1, int Hc, int Wc, int dy, int dx) {
  int64_t sad = 0;
  for (int y = 0; y < Hc; y += 2) {
    if (y + dy < 0 || y + dy >= Hc) continue;
    for (int x = 0; x < Wc; x += 2) {
      if (x + dx < 0 || x + dx >= Wc) continue;
      const int v = (int)I0[(size_t)y * Wc + x] - (int)I1[(size_t)(y + dy) * Wc + x + dx];
      sad += v < 0 ? -v : v;
    }
  }
  return sad;
}

// the step of one pair by the whole rule, candidate by candidate (the kernels tile the same sums)
WCT_GUIDED_HD inline void wct_motion_pair(const uint8_t* I0, const uint8_t* I1, int Hc, int Wc, int range, int32_t* d) {
  int by = 0, bx = 0;
  int64_t bs = wct_motion_sad(I0, I1, Hc, Wc, 0, 0), bc = wct_motion_count(0, 0, Hc, Wc);
  for (int dy = -range; dy <= range; ++dy)
    for (int dx = -range; dx <= range; ++dx) {
      const int64_t s = wct_motion_sad(I0, I1, Hc, Wc, dy, dx), n = wct_motion_count(dy, dx, Hc, Wc);
      if (wct_motion_better(s, n, dy, dx, bs, bc, by, bx)) { bs = s; bc = n; by = dy; bx = dx; }
    }
  d[0] = by; d[1] = bx;
}
