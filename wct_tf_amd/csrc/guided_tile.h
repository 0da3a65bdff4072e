// What the kernels of guided.hip, guided_color.hip, guided_up.hip and guided_up_color.hip share: the tiling (a block of NT threads owns SEG rows of a strip of
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

// The window sums of the grey guide's coefficient map abb [H][W][6] int32 (one frame) over the block's place: the column's
// running vertical sums in registers, per row the block-wide prefix, and emit(y, S) for every pixel (y, pl.x) the block owns, S[6]
// its window sums (a_q, b_q per channel).  What pass 2 of guided.hip and the means pass of guided_up.hip share.
template <typename Emit>
__device__ __forceinline__ void window_sums_ab(const int32_t* abb, const Place& pl, int H, int W, int r, long long (*P)[NT],
                                               long long (*tot)[NW], Emit&& emit) {
  const int t = threadIdx.x, x = pl.x;
  long long v[6] = {0, 0, 0, 0, 0, 0};                      // the column's window sums of (a_q, b_q) per channel
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const int32_t* p = abb + ((size_t)y * W + x) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += add ? (long long)p[k] : -(long long)p[k];
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    long long w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = v[k];
    block_prefix<long long, 6>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0);
    emit(y, S);
  }
}

// The same for the colour guide's coefficient map abb [H][W][12] int32 (one frame; 48 B per pixel from a 16-byte aligned base,
// read as three int4): emit(y, win) for every pixel (y, pl.x) the block owns, win(k) the window sum of coefficient k.  What pass 2
// of guided_color.hip and the means pass of guided_up_color.hip share.  P [12][NT] and tot [12][NW] are the block's.
template <typename Emit>
__device__ __forceinline__ void window_sums_ab12(const int32_t* abb, const Place& pl, int H, int W, int r, long long (*P)[NT],
                                                 long long (*tot)[NW], Emit&& emit) {
  constexpr int K = 12;
  const int t = threadIdx.x, x = pl.x;
  long long v[K];                                           // the column's window sums of the twelve coefficients
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0;
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const int4* p = reinterpret_cast<const int4*>(abb + ((size_t)y * W + x) * K);
#pragma unroll
    for (int k = 0; k < K / 4; ++k) {
      const int4 q = p[k];
      const int e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] += add ? (long long)e[j] : -(long long)e[j];
    }
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    long long w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = v[k];
    block_prefix<long long, K>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    emit(y, [&](int k) -> int64_t { return P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0); });
  }
}
}  // namespace
