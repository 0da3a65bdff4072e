// Whiten-colour transform (and AdaIN) for gfx950, replacing ops.py:24-140,282-294.
//
// Feature maps stay pixel-major (NHWC flattened: X[n][c], fp32) so none of the
// reference's four transposes exist.  Per transform:
//   K3  colstats      per-channel mean (two-stage, deterministic)
//   K4  cov           C x C covariance of the centred features, split-K; operands split into fp16
//                     hi+lo pairs (22 bits) on v_mfma_f32_32x32x16_f16, mean subtracted at load
//   K5  jacobi        batched two-sided block-Jacobi eigensolver (content+style together)
//   K6  tbuild        T = E_s f_s(L_s) E_s^T . E_c f_c(L_c) E_c^T with the 1e-5 cut-off
//   K7  apply         out = (x - mc) M^T + b,  M = alpha T + (1-alpha) I  (one GEMM,
//                     blend and re-centring folded into M and b)
// One translation unit per stage: K3, K4 and the fp32 GEMM behind the products of every stage in stats_gemm.hip, K5 in
// eigh.hip, K6 in spectral.hip; this file holds K7, the workspace carve, the slot plans and the transforms themselves (launch_wct, the
// style mix, AdaIN); spatial control is mask.hip, style-swap style_swap.hip.  What the units share: wct_stages.h.
#include "wct_stages.h"
#include "jacobi_dev.h"   // (JacobiState: carve() sizes the solver's state words)
#include "strength_rule.h"
#include "conv_first_tile.h"   // conv1_1 on one pixel tile (apply_image_kernel)
#include <algorithm>
#include <type_traits>

// (the blend M = alpha T + (1 - alpha) I, max |M| and the bias vector: gemm_f32_kernel's blend epilogue and
// spectral_open_all_kernel since round 5)

// ---------------------------------------------------------------------------
// K7: apply  out[n][j] = sum_k (x[n][k] - mc[k]) M[j][k] + b[j]   (ops.py:73-83 with the blend folded into M, b)
// Same split-operand scheme as the covariance: (x - mc) s_x and M s_M are split into fp16 hi + lo and
// multiplied by three v_mfma_f32_32x32x16_f16 with fp32 accumulation; s_x, s_M are powers of two.
// D[channel][pixel] (A = M rows, B = pixels) so that a lane ends up with 4 consecutive channels of one
// pixel, as in the conv epilogue.  Block = BC channels x BP pixels, 256 threads = 2x2 waves, K-stage 32.
// ---------------------------------------------------------------------------

template <int BC, int BP, typename Args = ApplyArgs>
__global__ __launch_bounds__(256, 2) void apply_f16x2_kernel(Args p) {
  constexpr bool SEGB = std::is_same<Args, ApplySegBatchArgs>::value;   // a masked batch: per-frame seg_off / perm / rows
  constexpr bool SEG = std::is_same<Args, ApplySegArgs>::value || SEGB;  // (ApplyArgs: not a line of the plain apply changes)
  constexpr bool MAP = std::is_same<Args, ApplyMapArgs>::value;          // a strength map: M is the alpha = 1 matrix, the blend per row
  constexpr int TM = BC / 64, TN = BP / 64;
  constexpr int MI = BC * 4 / 256, XI = BP * 4 / 256;    // 16-B (8 k) pieces per thread and stage
  __shared__ __attribute__((aligned(16))) unsigned char lm[2][BC * 64];   // M hi, lo
  __shared__ __attribute__((aligned(16))) unsigned char lx[2][BP * 64];   // x hi, lo
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int pair = blockIdx.z;
  const int n0 = blockIdx.x * BP, c0 = blockIdx.y * BC;
  int seg0 = 0, N = p.N;
  [[maybe_unused]] int row0 = 0;                 // SEGB: the first row of the pair's frame in x, perm and the outputs
  if constexpr (SEGB) {
    const int f = seg_frame(p.fl[pair]), lab = seg_label(p.fl[pair]);
    const int first = p.seg_off[f * (WCT_MIX_MAX + 1) + lab];
    N = p.seg_off[f * (WCT_MIX_MAX + 1) + lab + 1] - first;
    if (n0 >= N) return;
    row0 = f * p.N;
    seg0 = row0 + first;
  } else if constexpr (SEG) {
    seg0 = p.seg_off[p.lab[pair]];
    N = p.seg_off[p.lab[pair] + 1] - seg0;
    if (n0 >= N) return;                         // (uniform per block: past the end of its segment)
  }
  const int C = p.C;
  const float* x = p.x + (SEG ? (size_t)seg0 * C : (size_t)pair * N * C);
  const float* M = p.M + (size_t)pair * C * C;
  const float* mean = p.mean + (size_t)pair * 2 * C;
  const float sx = p.xscale[2 * pair];
  float sM = 1.f;
  {
    const float m = __uint_as_float(p.mabs[pair]);
    if (m > 0.f) { int e; frexpf(m, &e); sM = ldexpf(1.f, 14 - e); }
  }

  // staging pointers (rows clamped: out-of-range rows are computed on valid data and dropped at the store)
  const float* mp[MI]; const float* xp[XI];
  int moff[MI], xoff[XI], xk[XI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int item = tid + i * 256, row = item >> 2, kq = item & 3;
    mp[i] = M + (size_t)min(c0 + row, C - 1) * C + kq * 8;
    moff[i] = (row * 4 + (kq ^ ((row >> 2) & 3))) * 16;
  }
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int item = tid + i * 256, row = item >> 2, kq = item & 3;
    xp[i] = x + (size_t)min(n0 + row, N - 1) * C + kq * 8;
    xoff[i] = (row * 4 + (kq ^ ((row >> 2) & 3))) * 16;
    xk[i] = kq * 8;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 rm[MI][2], rx[XI][2];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      rm[i][0] = *reinterpret_cast<const f32x4*>(mp[i] + k0);
      rm[i][1] = *reinterpret_cast<const f32x4*>(mp[i] + k0 + 4);
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      rx[i][0] = *reinterpret_cast<const f32x4*>(xp[i] + k0) - *reinterpret_cast<const f32x4*>(mean + k0 + xk[i]);
      rx[i][1] = *reinterpret_cast<const f32x4*>(xp[i] + k0 + 4) - *reinterpret_cast<const f32x4*>(mean + k0 + xk[i] + 4);
    }
  };
  auto split_store = [&](const f32x4 (&r)[2], float sc, unsigned char* hi, unsigned char* lo, int off) {
    half8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = r[j >> 2][j & 3] * sc;
      h[j] = (half_t)v;
      l[j] = (half_t)(v - (float)h[j]);
    }
    *reinterpret_cast<half8*>(hi + off) = h;
    *reinterpret_cast<half8*>(lo + off) = l;
  };

  load(0);
  for (int k0 = 0; k0 < C; k0 += 32) {
#pragma unroll
    for (int i = 0; i < MI; ++i) split_store(rm[i], sM, lm[0], lm[1], moff[i]);
#pragma unroll
    for (int i = 0; i < XI; ++i) split_store(rx[i], sx, lx[0], lx[1], xoff[i]);
    __syncthreads();
    if (k0 + 32 < C) load(k0 + 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int chunk = ks * 2 + (lane >> 5);
      half8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = (wm * TM + i) * 32 + (lane & 31);
        const int off = (r * 4 + (chunk ^ ((r >> 2) & 3))) * 16;
        ah[i] = *reinterpret_cast<const half8*>(lm[0] + off);
        al[i] = *reinterpret_cast<const half8*>(lm[1] + off);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int r = (wn * TN + j) * 32 + (lane & 31);
        const int off = (r * 4 + (chunk ^ ((r >> 2) & 3))) * 16;
        bh[j] = *reinterpret_cast<const half8*>(lx[0] + off);
        bl[j] = *reinterpret_cast<const half8*>(lx[1] + off);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }

  // epilogue: reg r of a tile = channel (r&3)+8*(r>>2)+4*(lane>>5), pixel lane&31
  const float inv = 1.f / (sx * sM);
  const float* bias = p.bias + (size_t)pair * C;
  const int kgrp = lane >> 5;
  // this lane's bias values, fetched before the first store (a load issued between the stores waits with vmcnt(0),
  // i.e. for every store issued so far: see conv_epilogue_t)
  f32x4 bvs[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int co = c0 + (wm * TM + i) * 32 + 8 * rq + 4 * kgrp;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      bvs[i][rq] = co < C ? *reinterpret_cast<const f32x4*>(bias + co) : z;
    }
  int dst[TN];                                   // SEG: the scatter rows, fetched before the first store as well
  if constexpr (SEG)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
      dst[j] = p.perm[seg0 + (n < N ? n : 0)];
      if constexpr (SEGB) dst[j] += row0;
    }
  // MAP: the strength a of this lane's pixels and their content features, in the epilogue's own layout (4 consecutive channels of
  // one pixel), fetched before the first store as well
  [[maybe_unused]] float amap[TN];
  [[maybe_unused]] f32x4 xv[TN][TM][4];
  if constexpr (MAP)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + (wn * TN + j) * 32 + (lane & 31), nc = n < N ? n : 0;
      const uint8_t* sm = p.smap + (size_t)pair * p.Hm * p.Wm;
      amap[j] = wct_strength_a(p.alpha, sm[wct_strength_index(nc / p.w, nc % p.w, p.stride, p.Hm, p.Wm)]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int co = c0 + (wm * TM + i) * 32 + 8 * rq + 4 * kgrp;
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          xv[j][i][rq] = co < C ? *reinterpret_cast<const f32x4*>(x + (size_t)nc * C + co) : z;
        }
    }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
    const bool n_ok = n < N;
    const size_t row = SEG ? (size_t)dst[j] * C : ((size_t)pair * N + (n_ok ? n : 0)) * C;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int cb = c0 + (wm * TM + i) * 32;
      unsigned pk[4][2];
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int co = cb + 8 * rq + 4 * kgrp;
        const f32x4 bv = bvs[i][rq];
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[i][j][rq * 4 + q] * inv + bv[q];
        if constexpr (MAP)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = wct_strength_blend(amap[j], v[q], xv[j][i][rq][q]);
        if (p.out32 && n_ok && co < C) *reinterpret_cast<f32x4*>(p.out32 + row + co) = v;
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        h2 lo = {(half_t)v[0], (half_t)v[1]}, hi = {(half_t)v[2], (half_t)v[3]};
        pk[rq][0] = __builtin_bit_cast(unsigned, lo);
        pk[rq][1] = __builtin_bit_cast(unsigned, hi);
      }
      if (p.out16) {
        // pair register quads across the two half-waves (v_permlane32_swap): 16-B stores of 8 channels
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          auto sxw = __builtin_amdgcn_permlane32_swap(pk[2 * m][0], pk[2 * m + 1][0], false, false);
          auto syw = __builtin_amdgcn_permlane32_swap(pk[2 * m][1], pk[2 * m + 1][1], false, false);
          u32x4 o = {sxw[0], syw[0], sxw[1], syw[1]};
          const int co = cb + 16 * m + 8 * kgrp;
          if (n_ok && co < C) *reinterpret_cast<u32x4*>(p.out16 + row + co) = o;
        }
      }
    }
  }
}

// P pairs of at most nmax rows each: the plain apply, a masked transform's segments, a masked batch's
template <typename Args>
int launch_apply_args(const Args& a, int nmax, int P, hipStream_t s) {
  const int C = a.C;
  if (C >= 128) hipLaunchKernelGGL((apply_f16x2_kernel<128, 128, Args>), dim3(cdiv(nmax, 128), cdiv(C, 128), P), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((apply_f16x2_kernel<64, 128, Args>), dim3(cdiv(nmax, 128), cdiv(C, 64), P), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
template int launch_apply_args<ApplySegArgs>(const ApplySegArgs&, int, int, hipStream_t);
template int launch_apply_args<ApplySegBatchArgs>(const ApplySegBatchArgs&, int, int, hipStream_t);
template int launch_apply_args<ApplyMapArgs>(const ApplyMapArgs&, int, int, hipStream_t);

// ---------------------------------------------------------------------------
// K7 at relu1_1, from the IMAGE: apply_f16x2_kernel<64, 128, ApplyArgs> with the x operand computed instead of loaded, as a strip
// kernel.  A block walks APPLY_IMAGE_TILES consecutive tiles of 128 rows: M is fetched, split and parked once (both k-stages),
// conv1_1's bias and the content mean sit in LDS, and the patch values of the next tile are fetched under the current one.  Per
// tile, wave w computes relu1_1 of rows 32 w .. + 31 (pixel (n / W, n % W), conv_first_tile.h: 64 channels, in registers) and
// parks channels 32 s .. + 31 of them, less the mean, scaled and split as split_store does, in the [pixel][32 k] image of
// k-stage s: the conv's D layout leaves a lane 4 consecutive channels of one pixel, an 8-byte store.  The MFMA order and the
// epilogue are the plain kernel's, so the output is equal bit for bit.
// ---------------------------------------------------------------------------
struct ApplyImageArgs : ApplyArgs { WctImageSide img; const half_t* wfrag; const float* bias1; };
constexpr int APPLY_IMAGE_TILES = 8;

__global__ __launch_bounds__(256, 2) void apply_image_kernel(ApplyImageArgs p) {
  constexpr int C = 64, BP = 128, TN = BP / 64;
  __shared__ __attribute__((aligned(16))) unsigned char lm[2][2][C * 64];    // per k-stage: M hi, lo
  __shared__ __attribute__((aligned(16))) unsigned char lx[2][2][BP * 64];   // per k-stage: x hi, lo
  __shared__ __attribute__((aligned(16))) float lbm[2][C];                   // conv1_1's bias, the content mean
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int pair = blockIdx.z;
  const int H = p.img.H, W = p.img.W, N = H * W;
  const int tile0 = blockIdx.x * APPLY_IMAGE_TILES;
  const int ntile = min(APPLY_IMAGE_TILES, (N + BP - 1) / BP - tile0);
  const float* x = p.img.img + (size_t)pair * N * 3;
  const float* M = p.M + (size_t)pair * C * C;
  const float* mean = p.mean + (size_t)pair * 2 * C;
  const float sx = p.xscale[2 * pair];
  float sM = 1.f;
  {
    const float m = __uint_as_float(p.mabs[pair]);
    if (m > 0.f) { int e; frexpf(m, &e); sM = ldexpf(1.f, 14 - e); }
  }
  const int kgrp = lane >> 5;

  // once per block: this thread's 16-B piece of M for both k-stages (the plain kernel's staging), the epilogue's bias, the
  // vectors the x staging reads, conv1_1's weights
  const int mrow = tid >> 2, mkq = tid & 3;
  const float* mp = M + (size_t)mrow * C + mkq * 8;
  const int moff = (mrow * 4 + (mkq ^ ((mrow >> 2) & 3))) * 16;
  f32x4 rm[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    rm[s][0] = *reinterpret_cast<const f32x4*>(mp + s * 32);
    rm[s][1] = *reinterpret_cast<const f32x4*>(mp + s * 32 + 4);
  }
  const float* bias = p.bias + (size_t)pair * C;
  f32x4 bvs[4];
#pragma unroll
  for (int rq = 0; rq < 4; ++rq) bvs[rq] = *reinterpret_cast<const f32x4*>(bias + wm * 32 + 8 * rq + 4 * kgrp);
  if (tid < C) { lbm[0][tid] = p.bias1[tid]; lbm[1][tid] = mean[tid]; }

  // this lane's pixel: row tile0 * 128 + 32 wave + (lane & 31), then 128 rows on per tile (a row past the end reads the last
  // image row and is dropped at the store); pre: its 16 patch values, fetched a tile ahead
  int py, px;
  {
    const int n = tile0 * BP + wave * 32 + (lane & 31);
    py = n / W; px = n - py * W;
  }
  float pre[2][8];
  auto fetch = [&]() {
    conv1_patch_load(x, min(py, H - 1), px, H, W, kgrp, pre);
    px += BP;
    while (px >= W) { px -= W; ++py; }
  };
  fetch();
  half8 wh[2][2], wl[2][2];
  conv1_weights(p.wfrag, lane, wh, wl);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    half8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = rm[s][j >> 2][j & 3] * sM;
      h[j] = (half_t)v;
      l[j] = (half_t)(v - (float)h[j]);
    }
    *reinterpret_cast<half8*>(lm[s][0] + moff) = h;
    *reinterpret_cast<half8*>(lm[s][1] + moff) = l;
  }
  __syncthreads();

  const int xrow = wave * 32 + (lane & 31);
  const float inv = 1.f / (sx * sM);
  for (int t = 0; t < ntile; ++t) {
    f32x16 f[2];
    {
      float cur[2][8];
      conv1_patch_values(pre, kgrp, p.img.clamp01, cur);
      if (t + 1 < ntile) fetch();
      conv1_tile(wh, wl, [=](int ks, int j) { return cur[ks][j]; }, f);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {           // channels s * 32 + 8 rq + 4 kgrp + j: k = 8 rq + 4 kgrp + j of the stage
        const int ch = s * 32 + 8 * rq + 4 * kgrp;
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(&lbm[0][ch]), mc = *reinterpret_cast<const f32x4*>(&lbm[1][ch]);
        half4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = (conv1_act(f[s][rq * 4 + j], b1[j]) - mc[j]) * sx;
          h[j] = (half_t)v;
          l[j] = (half_t)(v - (float)h[j]);
        }
        const int off = (xrow * 4 + (rq ^ ((xrow >> 2) & 3))) * 16 + kgrp * 8;
        *reinterpret_cast<half4*>(lx[s][0] + off) = h;
        *reinterpret_cast<half4*>(lx[s][1] + off) = l;
      }
    __syncthreads();

    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int chunk = ks * 2 + (lane >> 5);
        half8 bh[TN], bl[TN];
        const int r = wm * 32 + (lane & 31);
        const int offa = (r * 4 + (chunk ^ ((r >> 2) & 3))) * 16;
        const half8 ah = *reinterpret_cast<const half8*>(lm[s][0] + offa), al = *reinterpret_cast<const half8*>(lm[s][1] + offa);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int rb = (wn * TN + j) * 32 + (lane & 31);
          const int off = (rb * 4 + (chunk ^ ((rb >> 2) & 3))) * 16;
          bh[j] = *reinterpret_cast<const half8*>(lx[s][0] + off);
          bl[j] = *reinterpret_cast<const half8*>(lx[s][1] + off);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[j], 0, 0, 0);
        }
      }
    __syncthreads();                             // the x images are free for the next tile; the stores below need no LDS

    // epilogue, the plain kernel's: reg r of a tile = channel (r&3)+8*(r>>2)+4*(lane>>5), pixel lane&31
    const int n0 = (tile0 + t) * BP;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
      const bool n_ok = n < N;
      const size_t row = ((size_t)pair * N + (n_ok ? n : 0)) * C;
      const int cb = wm * 32;
      unsigned pk[4][2];
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int co = cb + 8 * rq + 4 * kgrp;
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[j][rq * 4 + q] * inv + bvs[rq][q];
        if (p.out32 && n_ok) *reinterpret_cast<f32x4*>(p.out32 + row + co) = v;
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        h2 lo = {(half_t)v[0], (half_t)v[1]}, hi = {(half_t)v[2], (half_t)v[3]};
        pk[rq][0] = __builtin_bit_cast(unsigned, lo);
        pk[rq][1] = __builtin_bit_cast(unsigned, hi);
      }
      if (p.out16) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          auto sxw = __builtin_amdgcn_permlane32_swap(pk[2 * m][0], pk[2 * m + 1][0], false, false);
          auto syw = __builtin_amdgcn_permlane32_swap(pk[2 * m][1], pk[2 * m + 1][1], false, false);
          u32x4 o = {sxw[0], syw[0], sxw[1], syw[1]};
          const int co = cb + 16 * m + 8 * kgrp;
          if (n_ok) *reinterpret_cast<u32x4*>(p.out16 + row + co) = o;
        }
      }
    }
  }
}

// launch_apply at relu1_1 with the content rows computed from the images `img` [P][H][W][3] (N = H * W rows a pair)
static int launch_apply_image(const WctCarve& w, const WctImageSrc& src, int P, half_t* out16, float* out32, hipStream_t s) {
  const WctImageSide& im = src.side[0];
  ARG_CHECK(im.img && im.H >= 2 && im.W >= 2 && src.wfrag && src.bias);
  ApplyImageArgs a;
  static_cast<ApplyArgs&>(a) = apply_args<ApplyArgs>(w, nullptr, im.H * im.W, 64, out16, out32);
  a.img = im; a.wfrag = src.wfrag; a.bias1 = src.bias;
  hipLaunchKernelGGL(apply_image_kernel, dim3(cdiv(cdiv(a.N, 128), APPLY_IMAGE_TILES), 1, P), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// workspace carving (P independent content/style pairs per call)
// ---------------------------------------------------------------------------
static int wct_nslab(int N) { int s = cdiv(N, 64); return s < 1 ? 1 : (s > 256 ? 256 : s); }

static void cov_split(int C, int Nmax, int P, int* nsplit, int* ksplit) {
  const int nt = C >= 128 ? cdiv(C, 128) : 1;
  const int tiles = nt * (nt + 1) / 2 * P;     // tiles on or above the diagonal
  // slices per matrix: x2 matrices per pair.  A single pair gets >= 64 blocks (its covariance is a few tens
  // of microseconds either way); a finer split only multiplies the partial-sum traffic of a large batch
  int want = 32 / tiles;
  if (want < 1) want = 1;
  int ks = cdiv(cdiv(Nmax, want), 32) * 32;    // multiple of the kernel's K-stage
  if (ks < 256) ks = 256;
  *ksplit = ks;
  *nsplit = cdiv(Nmax, ks);
}

PairLayout pair_layout(int C, int Nc, int Ns) {
  PairLayout L;
  const int Nmax = Nc > Ns ? Nc : Ns;
  L.nslab = wct_nslab(Nmax);
  cov_split(C, Nmax, 1, &L.nsplit, &L.ksplit);
  return L;
}

// P pairs whose per-matrix partial buffers hold lay.nslab slabs / lay.nsplit K-slices (the largest layout of the call: a slot
// plan's matrices each keep the layout of their own pair -- SlotPlan)
WctCarve carve(void* base, int C, int P, const PairLayout& lay) {
  WctCarve w;
  w.nslab = lay.nslab; w.nsplit = lay.nsplit; w.ksplit = lay.ksplit;
  size_t off = 0;
  char* b = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) { void* p = b ? b + off : nullptr; off += align_up(bytes); return p; };
  const size_t cc = (size_t)C * C * sizeof(float);
  w.mean = (float*)take((size_t)2 * P * C * sizeof(float));
  w.var = (float*)take((size_t)2 * P * C * sizeof(float));
  w.stat_partial = (float*)take((size_t)2 * P * w.nslab * C * sizeof(float));
  w.absmax = (float*)take((size_t)2 * P * w.nslab * sizeof(float));
  w.scale = (float*)take((size_t)2 * P * sizeof(float));
  w.cov_partial = (float*)take((size_t)2 * P * w.nsplit * cc);
  w.A = (float*)take(2 * P * cc);
  w.A0 = (float*)take(2 * P * cc);          // the covariances as computed (the solver rotates w.A in place)
  w.refresh = (int*)take((size_t)2 * P * sizeof(int));
  w.V = (float*)take(2 * P * cc);
  w.d = (float*)take((size_t)2 * P * C * sizeof(float));
  w.G = (float*)take(2 * P * cc);
  w.X = (float*)take(2 * P * cc);
  w.S2 = (float*)take(7 * P * cc);          // second-order operands of a level, all matrices at once: N [2P], X2 [2P], R, Pm, X1 [P]
  w.Tw = (float*)take(2 * P * cc);          // [2P][C][C] interleaved: whitening matrix of pair p at 2p, colouring matrix at 2p + 1
  w.Tcs = w.Tw + (size_t)C * C;             // (pair 0's colouring matrix.  Style-swap, one pair: the style's whitening matrix in T)
  w.T = (float*)take(P * cc);
  w.M = (float*)take(P * cc);
  w.bias = (float*)take((size_t)P * C * sizeof(float));
  w.mabs = (unsigned*)take((size_t)P * sizeof(unsigned));
  w.jacobi_bytes = jacobi_workspace_bytes(C, 2 * P) + 4 * (1024 + 64 * sizeof(JacobiState));   // (+ the alignment slack of
                                                                                                 //  the former four-group split)
  w.jacobi_ws = take(w.jacobi_bytes);
  w.mix = (float*)take((size_t)2 * C * sizeof(float));      // the AdaIN mix's mean and standard deviation (launch_adain_mix)
  w.total = off;
  return w;
}

size_t wct_workspace_bytes(int C, int Nc, int Ns, int P) {
  const int Cw = C < 32 ? 32 : C;
  return carve(nullptr, Cw, P, pair_layout(Cw, Nc, Ns)).total;
}

// M = alpha (Tcs . Tw) + (1 - alpha) I, max |M| -> mabs for P pairs: the blend in the product's epilogue
int launch_blend(const WctCarve& w, int C, int P, float alpha, WctSkip skip, hipStream_t s) {
  const size_t cc = (size_t)C * C;
  GemmArgs g = {};
  g.A = w.Tcs; g.lda = C; g.a_kmajor = 0; g.B = w.Tw; g.ldb = C; g.b_kmajor = 1; g.sA = one_style(skip) ? 0 : 2 * cc; g.sB = 2 * cc;
  g.M = C; g.N = C; g.K = C; g.ksplit = C; g.out32 = w.M; g.ldo = C; g.s_out = cc;
  g.blend = 1; g.alpha = alpha; g.mabs = w.mabs;
  return launch_gemm(g, 1, P, s);
}

// the apply out = (x - mc) M^T + bias of P pairs of Nc rows, on the mean, scale, M, bias and mabs of w:
// out[n][j] = sum_k (x[n][k]-mc[k]) M[j][k] + bias[j]
int launch_apply(const WctCarve& w, const float* content, int Nc, int C, int P, half_t* out16, float* out32, hipStream_t s) {
  return launch_apply_args(apply_args<ApplyArgs>(w, content, Nc, C, out16, out32), Nc, P, s);
}

// a strength map's geometry against the rows it serves
static bool strength_ok(const WctStrength& sm, int Nc) {
  return sm.smap && sm.Hm >= 1 && sm.Wm >= 1 && sm.w >= 1 && sm.stride >= 1 && Nc % sm.w == 0;
}

// the blend product at alpha = 1 for P pairs -- the plain alpha = 1 call's M, bias and mabs --, then the apply that blends every
// row with its content features by the strength of its pixel
static int launch_blend_apply_map(const WctCarve& w, const float* content, int Nc, int C, int P, WctSkip skip, const WctCall& r,
                                  const WctStrength& sm) {
  int rc;
  if ((rc = launch_blend(w, C, P, 1.f, skip, r.stream))) return rc;
  ApplyMapArgs a = apply_args<ApplyMapArgs>(w, content, Nc, C, r.out16, r.out32);
  a.smap = sm.smap; a.Hm = sm.Hm; a.Wm = sm.Wm; a.w = sm.w; a.stride = sm.stride; a.alpha = r.alpha;
  return launch_apply_args(a, Nc, P, r.stream);
}

// the blend product for P pairs, then the apply
static int launch_blend_apply(const WctCarve& w, const float* content, int Nc, int C, int P, WctSkip skip, const WctCall& r) {
  int rc;
  if ((rc = launch_blend(w, C, P, r.alpha, skip, r.stream))) return rc;
  return launch_apply(w, content, Nc, C, P, r.out16, r.out32, r.stream);
}

// ---------------------------------------------------------------------------
// Prepared styles (wct_style, api.h; the drivers in api_stylize.hip).  The colouring side of a level is content-independent up to the layout of its partial
// sums: the colouring matrix Tcs [C][C] and the style mean [C] (WCT), the mean and the variance (AdaIN).  A STATE holds them --
// [mean C][var C][Tcs C x C] floats -- for ONE layout and mode (WctStyleKey).  launch_style_state fills one from a style's features
// with the content slot dead (WCT_SKIP_CONTENT): the statistics, covariance, eigensolve and spectral tail of launch_wct on
// matrix 1 alone, so the state holds launch_wct's own bits.  A transform with `prep` set runs the content side alone
// (WCT_SKIP_STYLE; a mix: WCT_SKIP_MIX_STYLE) and style_load_kernel copies state k into the style slot 2k + 1 in front of the
// consumers, which read it as they read a computed one -- not a line of them changes.
// ---------------------------------------------------------------------------
WctStyleKey wct_style_key(int C, int Nc, int Ns) {
  const PairLayout L = pair_layout(std::max(C, 32), Nc, Ns);
  return WctStyleKey{L.nslab, L.nsplit, L.ksplit};
}
size_t wct_style_state_floats(int C) { return (size_t)2 * C + (size_t)C * C; }

// grid (blocks, K): state k -> mean / var slot 2k + 1 and, with_T, Tw matrix 2k + 1 (C % 4 == 0: no float4 straddles a part).
// Ref: WctStyleRef (the K styles of a call), or WctStyleSlots (a masked batch: the state of every (frame, region) pair)
template <typename Ref>
__global__ __launch_bounds__(256) void style_load_kernel(Ref r, float* mean, float* var, float* Tw, int C, int with_T) {
  const int k = blockIdx.y;
  const float* src = r.state[k];
  const size_t cc = (size_t)C * C, n = (size_t)2 * C + (with_T ? cc : 0), slot = (size_t)(2 * k + 1);
  for (size_t i = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * blockDim.x * 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
    float* dst = i < (size_t)C ? mean + slot * C + i : (i < (size_t)2 * C ? var + slot * C + (i - C) : Tw + slot * cc + (i - 2 * C));
    *reinterpret_cast<f32x4*>(dst) = v;
  }
}

template <typename Ref>
static int launch_style_load(const Ref& r, int K, const WctCarve& w, int C, bool with_T, hipStream_t s) {
  for (int k = 0; k < K; ++k) ARG_CHECK(r.state[k] != nullptr);
  const size_t n4 = ((size_t)2 * C + (with_T ? (size_t)C * C : 0)) / 4;
  hipLaunchKernelGGL(style_load_kernel<Ref>, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 256), K), dim3(256), 0, s, r, w.mean, w.var,
                     w.Tw, C, with_T ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_style_load_slots(const WctStyleSlots& r, int P, const WctCarve& w, int C, bool with_T, hipStream_t s) {
  ARG_CHECK(P >= 1 && P <= WCT_PLAN_PAIRS);
  return launch_style_load(r, P, w, C, with_T, s);
}

// the plan of a state: one pair, the style in slot 1 with the layout of the key, the content slot dead
static void style_plan(SlotPlan* sp, void* base, int C, const float* style, int Ns, const WctStyleKey& key) {
  *sp = SlotPlan{};
  sp->P = 1; sp->skip = WCT_SKIP_CONTENT; sp->nwhite = 0;
  sp->slot[1] = {style, Ns, PairLayout{key.nslab, key.nsplit, key.ksplit}};
  plan_carve(sp, base, C);
}

size_t wct_style_workspace_bytes(int C, int Ns, const WctStyleKey& key) {
  SlotPlan sp;
  style_plan(&sp, nullptr, C, nullptr, Ns, key);
  return sp.total;
}

int launch_style_state(const float* style, int Ns, int C, const WctStyleKey& key, int adain, const WctCall& r, float* state) {
  const int mode = r.mode; hipStream_t s = r.stream;
  ARG_CHECK(style && state && C % 32 == 0 && C >= 32 && C <= 1024 && Ns >= (adain ? 1 : 2) && launch_map_fits((size_t)Ns * C, 4));
  ARG_CHECK(adain || mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  ARG_CHECK(key.nslab >= 1 && key.nslab <= 256 && key.nsplit >= 1 && key.ksplit >= 256 && key.ksplit % 32 == 0 &&
            (long long)key.nsplit * key.ksplit >= Ns);
  SlotPlan sp;
  style_plan(&sp, r.workspace, C, style, Ns, key);
  ARG_CHECK(r.workspace_bytes >= sp.total);
  const WctCarve& w = sp.w;
  int rc;
  if (adain) {
    if ((rc = launch_plan_stats(sp, C, true, false, 0.f, s))) return rc;
    HIP_TRY(hipMemcpyAsync(state + C, w.var + C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    if ((rc = launch_plan_stats(sp, C, false, true, cov_eps(mode, r.eps), s))) return rc;
    if ((rc = launch_eig_stage(w, C, sp.P, sp.skip, 1, nullptr, r.eig_fail, s))) return rc;
    if ((rc = launch_spectral_tail(w, C, sp.P, 1.f, mode, r.eps, sp.skip, sp.nwhite, s))) return rc;
    HIP_TRY(hipMemcpyAsync(state + 2 * C, w.Tw + (size_t)C * C, (size_t)C * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  HIP_TRY(hipMemcpyAsync(state, w.mean + C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, s));
  return WCT_OK;
}

int launch_wct(const float* content, int Nc, const float* style, int Ns, int C, int P, WctSkip skip, const WctCall& r,
               const WctFeatStats* stats, const WctStyleRef* prep, const WctWarmRef* warm, const WctStrength* sm, const WctImageSrc* src) {
  const int mode = r.mode, stages = r.stages; hipStream_t s = r.stream;
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 1024 && Nc >= 2 && Ns >= 2 && P >= 1 && P <= 32);
  // covariance and apply from the images: relu1_1 of plain pairs, the means of both sides from the unit sums their conv1_1 pass took
  ARG_CHECK(!src || (C == 64 && !prep && !warm && !sm && stats && stats->u[0] && stats->umax[0] && stats->u[1] && stats->umax[1] &&
                     src->side[0].H * src->side[0].W == Nc && src->side[1].H * src->side[1].W == Ns));
  ARG_CHECK(!sm || strength_ok(*sm, Nc));
  ARG_CHECK(skip == WCT_SKIP_NONE || skip == WCT_SKIP_SHARED_STYLE);
  ARG_CHECK(!warm || (warm->basis && (skip == WCT_SKIP_NONE || prep)));
  if (prep) skip = WCT_SKIP_STYLE;               // (the style rows are not read: `style` may be null)
  ARG_CHECK(mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  // the covariance kernel addresses one feature map through a buffer resource with 32-bit byte offsets
  ARG_CHECK(launch_map_fits((size_t)Nc * C, 4) && launch_map_fits((size_t)Ns * C, 4));
  WctCarve w = carve(r.workspace, C, P, pair_layout(C, Nc, Ns));
  ARG_CHECK(r.workspace_bytes >= w.total);
  int rc;
  if (stages & WCT_STAGE_COV) {
    if ((rc = launch_means(content, Nc, style, Ns, C, P, w, false, skip, s, stats))) return rc;
    if (src) rc = launch_cov_image(*src, P, w, cov_eps(mode, r.eps), skip, s);
    else rc = launch_cov(content, Nc, style, Ns, C, P, w, cov_eps(mode, r.eps), skip, s);
    if (rc) return rc;
  }
  if (stages & WCT_STAGE_EIG) {
    // a warm start (warm.hip): the content matrices rotated into the stored basis, the same solve on them, the bases composed --
    // and the last content's eigenvectors, re-orthonormalised, kept for the next call (after a cold solve as well)
    const bool rotate = warm && warm->valid;
    if (rotate && (rc = launch_warm_rotate(w, C, P, warm->basis, s))) return rc;
    if ((rc = launch_eig_stage(w, C, P, skip, (stages & WCT_STAGE_EIG_FP32UPDATE) ? 0 : 1, r.sweeps_dev, r.eig_fail, s, rotate ? 0 : 2)))
      return rc;
    if (rotate && (rc = launch_warm_compose(w, C, P, warm->basis, s))) return rc;
    if (warm && (rc = launch_warm_store(w.V + (size_t)2 * (P - 1) * C * C, w.X, warm->basis, C, s))) return rc;
  }
  if (!(stages & WCT_STAGE_APPLY)) return WCT_OK;

  if (prep && (rc = launch_style_load(*prep, 1, w, C, true, s))) return rc;
  if ((rc = launch_spectral_tail(w, C, P, sm ? 1.f : r.alpha, mode, r.eps, skip, P, s))) return rc;
  if (sm) return launch_blend_apply_map(w, content, Nc, C, P, skip, r, *sm);
  if (src) {                                     // the apply computes the content rows from the images as well: `content` is not read
    if ((rc = launch_blend(w, C, P, r.alpha, skip, s))) return rc;
    return launch_apply_image(w, *src, P, r.out16, r.out32, s);
  }
  return launch_blend_apply(w, content, Nc, C, P, skip, r);
}

// ---------------------------------------------------------------------------
// Style mix (Li et al. 2017, sec. 4.2): mix(fc) = sum_k lambda_k T(fc, fs_k, alpha), sum_k lambda_k = 1.  T is affine in the
// colouring side, so the mix is ONE transform with Tcs_mix = sum_k lambda_k Tcs_k and bias_mix = sum_k lambda_k bias_k.
// Slot layout (mix_plan): the P = K pair layout of carve(), matrix 0 the content, matrix 2k + 1 style k; the content slots 2k
// (k >= 1) are skipped everywhere (WCT_SKIP_MIX), so the content's statistics, covariance, eigensystem and whitening run once, and
// the K + 1 live matrices share one batched eigensolve.  Every matrix keeps the slab / K-slice layout it has in the single-pair
// transform of its own (content, style) pair -- style k that of (content, style k), the content that of (content, style
// ref), ref = the style of the largest weight -- so each of them comes out bit for bit as launch_wct computes it: K = 1, and
// one-hot weights, give launch_wct's output exactly (the mix below starts from 0 and 0 + 1 x = x).
// ---------------------------------------------------------------------------
// the workspace of a plan: partial buffers for the largest layout of its live slots (at least one pair)
void plan_carve(SlotPlan* sp, void* base, int C) {
  PairLayout mx = {1, 1, 0};
  for (int m = 0; m < 2 * sp->P; ++m)
    if (sp->slot[m].n) { mx.nslab = std::max(mx.nslab, sp->slot[m].lay.nslab); mx.nsplit = std::max(mx.nsplit, sp->slot[m].lay.nsplit); }
  sp->w = carve(base, C, std::max(sp->P, 1), mx);
  sp->total = sp->w.total;
}

// the covariance kernel addresses one feature map through a buffer resource with 32-bit byte offsets
bool plan_fits(const SlotPlan& sp, int C) {
  for (int m = 0; m < 2 * sp.P; ++m)
    if (!launch_map_fits((size_t)sp.slot[m].n * C, 4)) return false;
  return true;
}

// The plan of a style mix (see above).  C: the channels (AdaIN takes C < 32; its workspace is laid out as for 32).  styles may
// be null (the workspace size alone).  False for arguments no mix takes.
static bool mix_plan(SlotPlan* sp, void* base, int C, const float* content, int Nc, const float* const* styles, const int* Ns,
                     int K, const float* lambda, int nmin, const WctFeatStats* stats, bool prepared = false) {
  if (!Ns || !lambda || K < 1 || K > WCT_MIX_MAX) return false;
  int ref = 0;
  for (int k = 0; k < K; ++k) {
    if ((styles && !styles[k]) || Ns[k] < nmin || !(lambda[k] >= 0.f && lambda[k] <= 1.f)) return false;
    if (lambda[k] > lambda[ref]) ref = k;
  }
  const int Cw = std::max(C, 32);
  *sp = SlotPlan{};
  sp->P = K; sp->skip = WCT_SKIP_MIX; sp->nwhite = 1;
  if (stats) { sp->u0 = stats->u[0]; sp->umax0 = stats->umax[0]; }
  sp->slot[0] = {content, Nc, pair_layout(Cw, Nc, Ns[ref])};
  for (int k = 0; k < K; ++k) sp->slot[2 * k + 1] = {styles ? styles[k] : nullptr, Ns[k], pair_layout(Cw, Nc, Ns[k])};
  if (prepared) {                                // the K style slots take prepared states: the content alone is live
    sp->skip = WCT_SKIP_MIX_STYLE;
    for (int k = 0; k < K; ++k) sp->slot[2 * k + 1].n = 0;
  }
  plan_carve(sp, base, Cw);
  return true;
}

size_t wct_mix_workspace_bytes(int C, int Nc, const int* Ns, int K, const float* lambda) {
  SlotPlan sp;     // (a prepared mix needs no more: its style slots are dead)
  return mix_plan(&sp, nullptr, C, nullptr, Nc, nullptr, Ns, K, lambda, 1, nullptr) ? sp.total : 0;
}

struct MixWeights { float lambda[WCT_MIX_MAX]; int K; };

// Tcs_mix = sum_k lambda_k Tcs_k (Tcs_k = matrix 2k + 1 of Tw) into matrix 1, bias_mix = sum_k lambda_k bias_k into bias[0]:
// fp32, k in order, from 0.  In place: an element is read (all k) and written by one thread.
__global__ __launch_bounds__(256) void wct_mix_kernel(float* Tw, float* bias, int C, MixWeights mw) {
  const size_t cc = (size_t)C * C, n4 = cc / 4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < mw.K; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(Tw + (2 * k + 1) * cc + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(mw.lambda[k], t[j], acc[j]);
    }
    *reinterpret_cast<f32x4*>(Tw + cc + i * 4) = acc;
  }
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float acc = 0.f;
      for (int k = 0; k < mw.K; ++k) acc = fmaf(mw.lambda[k], bias[(size_t)k * C + c], acc);
      bias[c] = acc;
    }
}

int launch_wct_mix(const float* content, int Nc, const float* const* styles, const int* Ns, int K, const float* lambda, int C,
                   const WctCall& r, const WctFeatStats* stats, const WctStyleRef* prep) {
  const int mode = r.mode, stages = r.stages; hipStream_t s = r.stream;
  SlotPlan sp;
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 1024 && Nc >= 2 && content && (styles || prep) &&
            mix_plan(&sp, r.workspace, C, content, Nc, prep ? nullptr : styles, Ns, K, lambda, 2, stats, prep != nullptr));
  ARG_CHECK(mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  ARG_CHECK(plan_fits(sp, C));
  ARG_CHECK(r.workspace_bytes >= sp.total);
  const WctCarve& w = sp.w;
  int rc;
  if ((stages & WCT_STAGE_COV) && (rc = launch_plan_stats(sp, C, false, true, cov_eps(mode, r.eps), s))) return rc;
  if ((stages & WCT_STAGE_EIG) && (rc = launch_eig_stage(w, C, sp.P, sp.skip, 1, r.sweeps_dev, r.eig_fail, s))) return rc;
  if (!(stages & WCT_STAGE_APPLY)) return WCT_OK;
  if (prep && (rc = launch_style_load(*prep, K, w, C, true, s))) return rc;
  if ((rc = launch_spectral_tail(w, C, sp.P, r.alpha, mode, r.eps, sp.skip, sp.nwhite, s))) return rc;
  MixWeights mw = {};
  mw.K = K;
  for (int k = 0; k < K; ++k) mw.lambda[k] = lambda[k];
  const size_t n4 = (size_t)C * C / 4;
  hipLaunchKernelGGL(wct_mix_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 1024)), dim3(256), 0, s, w.Tw, w.bias, C, mw);
  HIP_TRY(hipGetLastError());
  return launch_blend_apply(w, content, Nc, C, 1, WCT_SKIP_NONE, r);      // (the mixed colouring sits in pair 0's own slot)
}

// ---------------------------------------------------------------------------
// AdaIN (ops.py:282-294): out = alpha*((x-mu_c)*rsqrt(var_c+eps)*sqrt(var_s)+mu_s) + (1-alpha)*x
// ---------------------------------------------------------------------------
// mix_mu / mix_sd (or null): the style moments as a mean and a STANDARD DEVIATION (a style mix, launch_adain_mix: squaring the
// mixed deviation to hand it over as a variance would not round-trip through sqrtf)
__global__ void adain_apply_kernel(const float* x, size_t n4_per_pair, int C, const float* mean, const float* var,
                                   float alpha, float eps, half_t* out16, float* out32, int style_of_pair0,
                                   const float* mix_mu = nullptr, const float* mix_sd = nullptr) {
  const int pair = blockIdx.y;
  const int cq = C / 4;
  const float* mp = mean + (size_t)pair * 2 * C;
  const float* vp = var + (size_t)pair * 2 * C;
  const float* ms = mix_mu ? mix_mu : mean + (size_t)(style_of_pair0 ? 0 : pair) * 2 * C + C;   // style moments
  const float* vs = var + (size_t)(style_of_pair0 ? 0 : pair) * 2 * C + C;
  const size_t base = (size_t)pair * n4_per_pair;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4_per_pair; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + (base + i) * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float inv = 1.f / sqrtf(vp[c + j] + eps);
      const float sd = mix_sd ? mix_sd[c + j] : sqrtf(vs[c + j]);
      const float y = (v[j] - mp[c + j]) * inv * sd + ms[c + j];
      o[j] = alpha * y + (1.f - alpha) * v[j];
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + (base + i) * 4) = o;
    if (out16) {
      half4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (half_t)o[j];
      *reinterpret_cast<half4*>(out16 + (base + i) * 4) = h;
    }
  }
}

// adain_apply_kernel with a strength map: y is its expression (so the bits of its alpha = 1 output), the blend strength_rule.h's
// with the strength of the row's pixel; one row of C channels per C / 4 consecutive threads, as there
__global__ void adain_apply_map_kernel(const float* x, size_t n4_per_pair, int C, const float* mean, const float* var, float eps,
                                       half_t* out16, float* out32, int style_of_pair0, WctStrength m, float alpha) {
  const int pair = blockIdx.y;
  const int cq = C / 4;
  const float* mp = mean + (size_t)pair * 2 * C;
  const float* vp = var + (size_t)pair * 2 * C;
  const float* ms = mean + (size_t)(style_of_pair0 ? 0 : pair) * 2 * C + C;
  const float* vs = var + (size_t)(style_of_pair0 ? 0 : pair) * 2 * C + C;
  const uint8_t* sm = m.smap + (size_t)pair * m.Hm * m.Wm;
  const size_t base = (size_t)pair * n4_per_pair;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4_per_pair; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cq) * 4, n = (int)(i / cq);
    const float a = wct_strength_a(alpha, sm[wct_strength_index(n / m.w, n % m.w, m.stride, m.Hm, m.Wm)]);
    f32x4 v = *reinterpret_cast<const f32x4*>(x + (base + i) * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float inv = 1.f / sqrtf(vp[c + j] + eps);
      const float sd = sqrtf(vs[c + j]);
      const float y = (v[j] - mp[c + j]) * inv * sd + ms[c + j];
      o[j] = wct_strength_blend(a, y, v[j]);
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + (base + i) * 4) = o;
    if (out16) {
      half4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (half_t)o[j];
      *reinterpret_cast<half4*>(out16 + (base + i) * 4) = h;
    }
  }
}

int launch_adain(const float* content, int Nc, const float* style, int Ns, int C, int P, WctSkip skip, const WctCall& r,
                 const WctFeatStats* stats, const WctStyleRef* prep, const WctStrength* sm) {
  hipStream_t s = r.stream;
  ARG_CHECK(C % 4 == 0 && C <= 1024 && Nc >= 1 && Ns >= 1 && P >= 1 && P <= 32);
  ARG_CHECK(!sm || strength_ok(*sm, Nc));
  ARG_CHECK(skip == WCT_SKIP_NONE || skip == WCT_SKIP_SHARED_STYLE);
  if (prep) skip = WCT_SKIP_STYLE;
  const int Cw = C < 32 ? 32 : C;
  WctCarve w = carve(r.workspace, Cw, P, pair_layout(Cw, Nc, Ns));
  ARG_CHECK(r.workspace_bytes >= w.total);
  int rc;
  if ((rc = launch_means(content, Nc, style, Ns, C, P, w, true, skip, s, stats))) return rc;
  if (prep && (rc = launch_style_load(*prep, 1, w, C, false, s))) return rc;
  const size_t n4 = (size_t)Nc * C / 4;
  if (sm)
    hipLaunchKernelGGL(adain_apply_map_kernel, dim3(rows_grid(Nc, C), P), dim3(256), 0, s, content, n4, C, w.mean, w.var, r.eps, r.out16,
                       r.out32, one_style(skip) ? 1 : 0, *sm, r.alpha);
  else
  hipLaunchKernelGGL(adain_apply_kernel, dim3(rows_grid(Nc, C), P), dim3(256), 0, s, content, n4, C, w.mean, w.var, r.alpha, r.eps, r.out16, r.out32,
                     one_style(skip) ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// AdaIN style mix: mu_mix = sum_k lambda_k mu_k, sd_mix = sum_k lambda_k sqrt(var_k) (fp32, k in order, from 0) into w.mix
__global__ void adain_mix_moments_kernel(const float* mean, const float* var, float* mix, int C, MixWeights mw) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float mu = 0.f, sd = 0.f;
  for (int k = 0; k < mw.K; ++k) {
    mu = fmaf(mw.lambda[k], mean[(size_t)(2 * k + 1) * C + c], mu);
    sd = fmaf(mw.lambda[k], sqrtf(var[(size_t)(2 * k + 1) * C + c]), sd);
  }
  mix[c] = mu;
  mix[C + c] = sd;
}

int launch_adain_mix(const float* content, int Nc, const float* const* styles, const int* Ns, int K, const float* lambda, int C,
                     const WctCall& r, const WctFeatStats* stats, const WctStyleRef* prep) {
  hipStream_t s = r.stream;
  SlotPlan sp;
  ARG_CHECK(C % 4 == 0 && C <= 1024 && Nc >= 1 && content && (styles || prep) &&
            mix_plan(&sp, r.workspace, C, content, Nc, prep ? nullptr : styles, Ns, K, lambda, 1, stats, prep != nullptr));
  ARG_CHECK(!prep || C >= 32);
  ARG_CHECK(r.workspace_bytes >= sp.total);
  const WctCarve& w = sp.w;
  int rc;
  if ((rc = launch_plan_stats(sp, C, true, false, 0.f, s))) return rc;
  if (prep && (rc = launch_style_load(*prep, K, w, C, false, s))) return rc;
  MixWeights mw = {};
  mw.K = K;
  for (int k = 0; k < K; ++k) mw.lambda[k] = lambda[k];
  hipLaunchKernelGGL(adain_mix_moments_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, w.mean, w.var, w.mix, C, mw);
  const size_t n4 = (size_t)Nc * C / 4;
  hipLaunchKernelGGL(adain_apply_kernel, dim3(rows_grid(Nc, C), 1), dim3(256), 0, s, content, n4, C, w.mean, w.var, r.alpha, r.eps, r.out16,
                     r.out32, 0, (const float*)w.mix, (const float*)(w.mix + C));
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
