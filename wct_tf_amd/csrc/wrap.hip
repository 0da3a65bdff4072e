// Wrap-around halos for periodic (tileable) synthesis: a map [B][H][W][E] extended periodically on the device, and the interior
// of an extended map copied back out.  The conv kernels reflect-pad whatever they are given; a map that carries a halo of its
// own pixels taken modulo its size makes every layer see a torus, and the interior of the pass over it is exact (banded.hip has
// the argument and the halo tables; the drivers are in api_ops.hip and api_stylize.hip).
// Byte movers.  A map is an array of UNITS, U per pixel: one float of an fp32 image (E = 3: pixels are 12 bytes, no 16-byte
// alignment survives a row), or one 16-byte group of a pixel's channels (fp16 feature maps, fp32 taps: E * sizeof a multiple of
// 16).  One lane per OUTPUT unit, so the stores of a wave are consecutive; the loads are consecutive wherever the source row
// does not wrap.  Grid (tiles, B); the indices inside one image are 32-bit, which the launchers make true by refusing what
// launch_map_fits refuses.
#include "common.h"

namespace {
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the mathematically non-negative remainder, n >= 1: a halo may be several periods wide
__device__ __forceinline__ int wrap_mod(int a, int n) {
  const int m = a % n;
  return m < 0 ? m + n : m;
}

// out [B][Hp][Wp][U] <- in [B][H][W][U]: out(y, x) = in((y - t) mod H, (x - l) mod W)
template <typename T>
__global__ __launch_bounds__(256) void wrap_pad_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int U, int t, int l,
                                                       int Hp, int Wp) {
  const unsigned row = (unsigned)Wp * (unsigned)U, n = (unsigned)Hp * row;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned yo = i / row, r = i - yo * row, xo = r / (unsigned)U, u = r - xo * (unsigned)U;
  const int ys = wrap_mod((int)yo - t, H), xs = wrap_mod((int)xo - l, W);
  const size_t b = blockIdx.y;
  out[b * n + i] = in[b * ((size_t)H * W * U) + ((unsigned)ys * (unsigned)W + (unsigned)xs) * (unsigned)U + u];
}

// out [B][h][w][U] <- the interior of in [B][Hp][Wp][U] at (t, l)
template <typename T>
__global__ __launch_bounds__(256) void wrap_crop_kernel(const T* __restrict__ in, T* __restrict__ out, int Hp, int Wp, int U, int t, int l,
                                                        int h, int w) {
  const unsigned row = (unsigned)w * (unsigned)U, n = (unsigned)h * row;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned y = i / row, r = i - y * row;
  const size_t b = blockIdx.y;
  out[b * n + i] = in[b * ((size_t)Hp * Wp * U) + ((y + (unsigned)t) * (unsigned)Wp + (unsigned)l) * (unsigned)U + r];
}

// the units of a pixel of E elements of `bytes` each: 16-byte groups where a pixel is a whole number of them (*wide), else elements
int pixel_units(int E, int bytes, bool* wide) {
  *wide = ((size_t)E * bytes) % 16 == 0;
  return *wide ? (int)((size_t)E * bytes / 16) : E;
}
}  // namespace

int launch_wrap_pad(const void* in, void* out, int B, int H, int W, int E, int elem_bytes, int t, int b, int l, int r, hipStream_t s) {
  ARG_CHECK(in && out && B >= 1 && B <= 65535 && H >= 1 && W >= 1 && E >= 1 && t >= 0 && b >= 0 && l >= 0 && r >= 0);
  ARG_CHECK(elem_bytes == 2 || elem_bytes == 4);
  const long long Hp = (long long)t + H + b, Wp = (long long)l + W + r;
  if (Hp > 0x7fffffff || Wp > 0x7fffffff || !launch_map_fits((size_t)Hp * (size_t)Wp * (size_t)E, (size_t)elem_bytes)) {
    wct_set_error("wrap pad: the %lldx%lld map of %d channels that a %dx%d tile makes with its halo passes 2^31 bytes in one launch",
                  Hp, Wp, E, H, W);
    return WCT_ERR_ARG;
  }
  bool wide;
  const int U = pixel_units(E, elem_bytes, &wide);
  ARG_CHECK(wide || elem_bytes == 4);                      // (fp16 maps come in whole 16-byte groups: C a multiple of 8)
  ARG_CHECK(!wide || (((uintptr_t)in | (uintptr_t)out) & 15) == 0);
  const unsigned n = (unsigned)((size_t)Hp * Wp * U);
  const dim3 grid((n + 255) / 256, B);
  if (wide) hipLaunchKernelGGL(wrap_pad_kernel<u32x4>, grid, dim3(256), 0, s, (const u32x4*)in, (u32x4*)out, H, W, U, t, l, (int)Hp, (int)Wp);
  else hipLaunchKernelGGL(wrap_pad_kernel<float>, grid, dim3(256), 0, s, (const float*)in, (float*)out, H, W, U, t, l, (int)Hp, (int)Wp);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_wrap_crop(const void* in, void* out, int B, int Hp, int Wp, int E, int elem_bytes, int t, int l, int h, int w, hipStream_t s) {
  ARG_CHECK(in && out && B >= 1 && B <= 65535 && Hp >= 1 && Wp >= 1 && E >= 1 && t >= 0 && l >= 0 && h >= 1 && w >= 1);
  ARG_CHECK((long long)t + h <= Hp && (long long)l + w <= Wp && (elem_bytes == 2 || elem_bytes == 4));
  if (!launch_map_fits((size_t)Hp * (size_t)Wp * (size_t)E, (size_t)elem_bytes)) {
    wct_set_error("wrap crop: the %dx%d map of %d channels passes 2^31 bytes in one launch", Hp, Wp, E);
    return WCT_ERR_ARG;
  }
  bool wide;
  const int U = pixel_units(E, elem_bytes, &wide);
  ARG_CHECK(wide || elem_bytes == 4);
  ARG_CHECK(!wide || (((uintptr_t)in | (uintptr_t)out) & 15) == 0);
  const unsigned n = (unsigned)((size_t)h * w * U);
  const dim3 grid((n + 255) / 256, B);
  if (wide) hipLaunchKernelGGL(wrap_crop_kernel<u32x4>, grid, dim3(256), 0, s, (const u32x4*)in, (u32x4*)out, Hp, Wp, U, t, l, h, w);
  else hipLaunchKernelGGL(wrap_crop_kernel<float>, grid, dim3(256), 0, s, (const float*)in, (float*)out, Hp, Wp, U, t, l, h, w);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
