// What the kernels of guided.hip and guided_color.hip share: the tiling (a block of NT threads owns SEG rows of a strip of
// NT - 2r columns of one frame, thread t owns column x0 - r + t with the halo), the block-wide prefix sums of a row, and the read
// of a content sample.  Included inside each unit, so every name is local to it.
#pragma once
#include "common.h"
#include "colors_rule.h"

namespace {
constexpr int NT = 256;               // threads of a block = columns of a strip with both halos
constexpr int NW = NT / 64;           // waves
constexpr int SEG = 64;               // output rows of a block

__device__ __forceinline__ int sample(const uint8_t* p) { return *p; }
__device__ __forceinline__ int sample(const float* p) { return wct_quantise_u8(*p); }

// Inclusive prefix sums of K values per thread across the block, into P[k][t].  tot [K][NW] is scratch.  Two barriers; the
// caller's reads of P and the next call's writes are separated by the first barrier of that call.
template <typename T, int K>
__device__ __forceinline__ void block_prefix(T (&v)[K], T (*P)[NT], T (*tot)[NW]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T x = v[k];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T up = __shfl_up(x, d, 64);
      if (lane >= d) x += up;
    }
    v[k] = x;
    if (lane == 63) tot[k][wave] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T base = 0;
    for (int w = 0; w < wave; ++w) base += tot[k][w];
    P[k][t] = v[k] + base;
  }
  __syncthreads();
}

// the block's place: strip and row segment of frame b
struct Place { int b, x, y0, y1; bool col, owner; };
__device__ __forceinline__ Place place(int H, int W, int r, int strips, int segs) {
  const int TW = NT - 2 * r, t = threadIdx.x;
  int id = blockIdx.x;
  const int strip = id % strips; id /= strips;
  const int seg = id % segs;
  Place p;
  p.b = id / segs;
  p.x = strip * TW - r + t;
  p.col = p.x >= 0 && p.x < W;                              // a column of the frame
  p.owner = p.col && t >= r && t < r + TW;                  // ... that this block writes
  p.y0 = seg * SEG;
  p.y1 = p.y0 + SEG < H ? p.y0 + SEG : H;
  return p;
}
}  // namespace
