// The strength map's rule, shared by the apply kernels of wct.hip and by any host program (plain C++: nothing of
// HIP is needed to include this file).  A strength map is a uint8 image of the content's size: 255 is the call's alpha, 0 keeps
// the content features.  Per feature row with the map byte v of its pixel, the content features x and the level's transform at
// alpha = 1, y (ops.py:83,133,293 with alpha replaced by a):
//   a   = alpha * (float(v) / 255.f)
//   out = a * y + (1.f - a) * x
// float32 throughout, every operation rounded once and none fused, the division correctly rounded: a kernel, a host program and
// NumPy (np.float32(alpha) * (np.float32(v) / np.float32(255)), then a * y + (np.float32(1) - a) * x) give the same bits.
// Two ends follow: v = 0 gives a = 0 and out = 0 y + 1 x = x (finite y), and v = 255 with alpha = 1 gives a = 1 and
// out = 1 y + 0 x = y (finite x).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WCT_STRENGTH_HD __host__ __device__
#else
#define WCT_STRENGTH_HD
#endif

// the map byte of feature pixel (i, j) at stride s = 2^(level - 1) of an Hm x Wm map: the rule label maps use; the
// clamp covers the later levels of a chain, whose maps can be larger than the content
WCT_STRENGTH_HD inline size_t wct_strength_index(int i, int j, int stride, int Hm, int Wm) {
  const int y = i * stride < Hm - 1 ? i * stride : Hm - 1, x = j * stride < Wm - 1 ? j * stride : Wm - 1;
  return (size_t)y * Wm + x;
}

WCT_STRENGTH_HD inline float wct_strength_a(float alpha, uint8_t v) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  const float q = __fdiv_rn((float)v, 255.f);      // (the IEEE quotient whatever division the unit is compiled with)
#else
  const float q = (float)v / 255.f;
#endif
  return alpha * q;
}

WCT_STRENGTH_HD inline float wct_strength_blend(float a, float y, float x) {
#pragma clang fp contract(off)
  const float ay = a * y;
  const float keep = 1.f - a;
  const float kx = keep * x;
  return ay + kx;
}
