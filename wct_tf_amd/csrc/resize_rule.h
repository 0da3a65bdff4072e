// Bilinear resize of 8-bit images as Pillow's Image.resize(.., Image.BILINEAR) does it (the resampler behind this project's
// resize_to -- the reference's utils.py:55-67, behind --content-size, stylize_video.py:29; webcam.py:163,189 resizes every frame
// by --scale): an integer rule, shared by the kernel of resize.hip and by any host program (plain C++: nothing of HIP is needed
// to include this file).
// Per axis, `in` the input length and `out` the output length; everything up to the integer taps is IEEE double in this order:
//   scale = in / out;  fs = max(scale, 1.0);  support = fs;  ksize = (int)ceil(support) * 2 + 1
//   for xx in 0 .. out-1:
//     center = (xx + 0.5) * scale
//     xmin = max((int)(center - support + 0.5), 0)                       (int): truncation
//     n    = min((int)(center + support + 0.5), in) - xmin
//     w[x] = tri((x + xmin - center + 0.5) * (1.0 / fs)),  x in 0 .. n-1,   tri(t) = |t| < 1 ? 1 - |t| : 0
//     ww = sum w[x] in order;  if ww != 0: w[x] /= ww
//     k[x] = (int)(0.5 + w[x] * 4194304.0)                               (22 bits; bilinear taps are never negative)
//   byte = clamp((2097152 + sum_x k[x] * src[xmin + x]) >> 22, 0, 255)   int32 throughout
// The image is resized along x first, into a uint8 intermediate of H x w, which is then resized along y.  An axis whose length
// does not change has the taps 2^22, 0 and reproduces its bytes.
// The tap tables are host work, once per geometry (wct_resize_taps: no floating-point contraction, or a fused multiply-add
// moves a tap by one); the byte of one output element is wct_resize_byte, host and device.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define WCT_RESIZE_HD __host__ __device__
#else
#define WCT_RESIZE_HD
#endif

constexpr int WCT_RESIZE_BITS = 22;

// taps per output index of an axis in -> out (the row length of the tap table); in, out >= 1
inline int wct_resize_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(fs) * 2 + 1;
}

// The tables of one axis: bounds [out][2] = (xmin, n) and taps [out][ksize] (zero past n); w: scratch of ksize doubles.
inline void wct_resize_taps(int in, int out, int* bounds, int* taps, double* w) {
#pragma clang fp contract(off)
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / fs;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    int* k = taps + (size_t)xx * ksize;
    for (int x = 0; x < n; ++x) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = (int)(0.5 + w[x] * 4194304.0);
    }
    for (int x = n; x < ksize; ++x) k[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
}

// one output byte: n taps k on the bytes src[0], src[stride], ..  (int32: n taps sum to 2^22 +- ksize, times 255, plus 2^21)
template <typename Src>
WCT_RESIZE_HD inline uint8_t wct_resize_byte(const int* k, int n, Src src, int stride) {
  int acc = 1 << (WCT_RESIZE_BITS - 1);
  for (int x = 0; x < n; ++x) acc += k[x] * (int)src[x * stride];
  acc >>= WCT_RESIZE_BITS;
  return (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}
