// What the 3x3 conv kernels of conv.hip and conv_wino.hip share: the tile constants behind the patch layout in LDS and the packed
// weight fragments (the two files read the same layouts, so they must agree on these), the packed register types and the padding rule.
#pragma once
#include "common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
constexpr int TW = 16;          // tile width in pixels (one MFMA B-fragment = 2 rows x 16)
constexpr int PITCH = 20;       // patch row pitch in pixels (18 used; multiple of 4 keeps the swizzle aligned)
constexpr int BK = 32;          // input channels per K-chunk

__device__ __forceinline__ int reflect_idx(int i, int n) {
  // 1-px REFLECT padding (edge not repeated): -1 -> 1, n -> n-2
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  // ragged tiles can run further out; clamp (those lanes are masked at the store)
  i = i < 0 ? 0 : i;
  return i >= n ? n - 1 : i;
}
