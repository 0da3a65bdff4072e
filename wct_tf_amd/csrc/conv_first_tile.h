// conv1_1's arithmetic on one MFMA pixel tile (32 pixels x 64 channels), in ONE copy: conv_first_kernel (conv.hip) and the
// kernels that compute relu1_1 where it is read instead of loading a stored map (cov_image_kernel, stats_gemm.hip;
// apply_image_kernel, wct.hip) call these functions, so that what they compute is what conv_first_kernel stores, bit for bit.
//   the patch value     conv1_fetch: clip(x, 0, 1) where the pass asks for it (model.py:86), applied when the value is fetched
//   the products        conv1_tile: every patch value v is split into fp16 hi = fp16(v) and lo = fp16(v - hi); k = ky * 9 + kx * 3 + c
//                       runs over two k-steps of 16 (k = 27..31 are padding: the value is 0); per k-step and tile of 32 output
//                       channels the three products wl.bh, wh.bl, wh.bh go into one fp32 accumulator in that order
//   the activation      conv1_act: the bias is added last, then max(., 0)
#pragma once
#include "common.h"

__device__ __forceinline__ float conv1_fetch(float v, int clamp01) { return clamp01 ? fminf(fmaxf(v, 0.f), 1.f) : v; }

// value(ks, j): the patch value of this lane's pixel (lane & 31) at k = ks * 16 + (lane >> 5) * 8 + j, 0.f for k >= 27.
// wh / wl [cout tile][k-step]: the weight fragments of ConvFirstArgs::wfrag, hi and lo.
// acc[nt] comes out in the MFMA D layout.  PIXEL_ROWS = false: the weights are the A operand -- register r of a lane is channel
// nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) of pixel lane & 31 (4 consecutive channels of one pixel).  PIXEL_ROWS = true: the
// operands change places -- register r is pixel (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) of channel nt * 32 + (lane & 31) (4
// consecutive pixels of one channel); every output is the same sum of the same products in the same order of k.
template <bool PIXEL_ROWS = false, typename Value>
__device__ __forceinline__ void conv1_tile(const half8 (&wh)[2][2], const half8 (&wl)[2][2], Value value, f32x16 (&acc)[2]) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    half8 bh, bl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = value(ks, j);
      bh[j] = (half_t)v;
      bl[j] = (half_t)(v - (float)bh[j]);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if constexpr (PIXEL_ROWS) {
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wl[nt][ks], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, wh[nt][ks], acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wh[nt][ks], acc[nt], 0, 0, 0);
      } else {
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[nt][ks], bh, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[nt][ks], bl, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[nt][ks], bh, acc[nt], 0, 0, 0);
      }
    }
  }
}

__device__ __forceinline__ float conv1_act(float acc, float bias) { return fmaxf(acc + bias, 0.f); }

// the weight fragments of a lane: [cout tile][k-step][hi/lo][lane][8] (ConvFirstArgs::wfrag), 8 coalesced 1-KiB loads
__device__ __forceinline__ void conv1_weights(const half_t* wfrag, int lane, half8 (&wh)[2][2], half8 (&wl)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      wh[t][ks] = *reinterpret_cast<const half8*>(wfrag + (((t * 2 + ks) * 2 + 0) * 64 + lane) * 8);
      wl[t][ks] = *reinterpret_cast<const half8*>(wfrag + (((t * 2 + ks) * 2 + 1) * 64 + lane) * 8);
    }
}

// A lane that fetches its pixel's patch straight from the image (no LDS patch; the readers of relu1_1, one pixel a lane):
// pre[ks][j] = the image value at k = ks * 16 + kgrp * 8 + j of pixel (y, px), 0 <= y < H, 0 <= px < W, of x [H][W][3]; k >= 27
// reads a valid address and is zeroed by conv1_patch_values.  The borders are conv_first_kernel's: with the pixel inside the
// image, reflect_idx(y - 1, H) = |y - 1| and reflect_idx(y + 1, H) = min(y + 1, 2 H - 3 - y), and so along x.
__device__ __forceinline__ void conv1_patch_load(const float* x, int y, int px, int H, int W, int kgrp, float (&pre)[2][8]) {
  const int ry[3] = {abs(y - 1), y, min(y + 1, 2 * H - 3 - y)};
  const int rx[3] = {abs(px - 1) * 3, px * 3, min(px + 1, 2 * W - 3 - px) * 3};
  int t[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) t[ky][kx] = ry[ky] * (W * 3) + rx[kx];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ka = ks * 16 + j, kb = ks * 16 + 8 + j < 27 ? ks * 16 + 8 + j : ka;    // (compile-time after unrolling)
      const int oa = t[ka / 9][(ka % 9) / 3] + ka % 3, ob = t[kb / 9][(kb % 9) / 3] + kb % 3;
      pre[ks][j] = x[kgrp ? ob : oa];
    }
}
// the values conv1_tile takes, out of what conv1_patch_load fetched: the padded k zeroed, the clamp (uniform) applied
__device__ __forceinline__ void conv1_patch_values(const float (&pre)[2][8], int kgrp, int clamp01, float (&cur)[2][8]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) cur[ks][j] = ks * 16 + 8 + j < 27 ? pre[ks][j] : (kgrp ? 0.f : pre[ks][j]);
  if (clamp01)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) cur[ks][j] = conv1_fetch(cur[ks][j], 1);
}
