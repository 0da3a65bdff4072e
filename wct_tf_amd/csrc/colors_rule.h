// Luminance-only colour preservation (Gatys et al. 2016, "Preserving Color in Neural Artistic Style Transfer", the post-hoc
// luminance transfer; jcjohnson/neural-style's -original_colors): the rule of one pixel, integers only, shared by the kernels
// of colors.hip and by any host program (plain C++: nothing of HIP is needed to include this file).
//   Y(q)   = 77 q.R + 150 q.G + 29 q.B               BT.601 weights x 256 (they sum to 256)
//   d      = Y(s) - Y(p)                             s the stylized pixel, p the content pixel
//   out.ch = clamp((256 p.ch + d + 128) >> 8, 0, 255)   for ch in R, G, B (arithmetic shift = floor)
// Adding one luminance difference to all three channels is "Y from s, U and V from p" for any luma-weighted YUV.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WCT_COLORS_HD __host__ __device__
#else
#define WCT_COLORS_HD
#endif

WCT_COLORS_HD inline int wct_luma256(int r, int g, int b) { return 77 * r + 150 * g + 29 * b; }

// the three output channels of one pixel: s = stylized (R, G, B), p = content (R, G, B), all in 0 .. 255
WCT_COLORS_HD inline void wct_content_colors_px(int sr, int sg, int sb, int pr, int pg, int pb, uint8_t out[3]) {
  const int d = wct_luma256(sr, sg, sb) - wct_luma256(pr, pg, pb) + 128;
  const int p[3] = {pr, pg, pb};
  for (int ch = 0; ch < 3; ++ch) {
    int v = (256 * p[ch] + d) >> 8;               // |256 p + d| < 2^17: no overflow; >> of a negative int floors
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    out[ch] = (uint8_t)v;
  }
}

// the output rule of the stylize chain (f32_to_u8_kernel, wct.py:66-68): uint8(clip(x, 0, 1) * 255.f), truncating; NaN -> 0
WCT_COLORS_HD inline uint8_t wct_quantise_u8(float x) {
  const float v = fminf(fmaxf(x, 0.f), 1.f) * 255.f;
  return (uint8_t)v;
}
