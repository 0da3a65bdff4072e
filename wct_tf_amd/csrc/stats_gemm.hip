// K3 column statistics, the generic fp32 GEMM (launch_gemm, common.h) and K4 covariance of the whiten-colour transform (the
// stage list: wct.hip), with the launchers of the statistics stage.  The GEMM stays between K3 and K4, where it has always
// been: hipcc inlines the small helpers (skip_style_mat, the blockIdx getters) in the order a unit first uses them, and
// gemm_f32_kernel alone in a unit comes out with other -- equivalent -- branches around skip_style_mat.
#include "wct_stages.h"
#include "conv_first_tile.h"    // conv1_1 on one pixel tile (cov_image_kernel)
#include <type_traits>

// ---------------------------------------------------------------------------
// K3: per-channel sums over the pixel axis
// ---------------------------------------------------------------------------
// grid (nslab, 2P): matrix m = 2*pair + side (0 content, 1 style); slab s reduces rows
// [s*rows_per_slab, ...) of X_m[N_side][C]

struct StatArgs {
  const float* x[2];     // content base [P][Nc][C], style base [P][Ns][C]
  int n[2];
  const float* u[2];     // per side: unit sums [P][ceil(n/16)][C] left by the conv epilogue that wrote x (ConvArgs::usum), or null
  const unsigned* umax[2];   // with u: [P][UMAX_SLOTS] bit patterns whose maximum is the largest value of each map
  const float* mean;     // [2P][C] or null; if set, accumulate (x-mean)^2 instead of x
  float* partial;        // [2P][nslab][C]
  float* absmax;         // [2P][nslab] max |x| of the slab (first pass only) or null
  int C, nslab;
  WctSkip skip;
};

// First pass (mean == null): the sum runs over UNITS of 16 consecutive rows, each added up in the fixed tree of
// unit_row_sum (common.h), then over the units of the slab in a fixed order.  A conv epilogue that wrote the features can
// hand the unit sums over (u): the 8 GB pass over the features of a 32-pair step shrinks to a pass over 1/16 of them, and
// the result is the same bit for bit whether the features come from the pipeline or from the caller (op-level entry
// points, widths that are not a multiple of 16).
__global__ __launch_bounds__(256) void colsum_kernel(StatArgs p) {
  __shared__ f32x4 red[256];
  const int mat = blockIdx.y, slab = blockIdx.x;
  if (skip_style_mat(mat, p.skip)) return;
  const int b = mat & 1, pair = mat >> 1;
  const int C = p.C, cq = C / 4;
  const int nrp = 256 / cq;                  // rows / units handled in parallel (C <= 1024)
  const int tid = threadIdx.x;
  const int rp = tid / cq, c4 = tid % cq;
  const int N = p.n[b];
  const float* x = p.x[b] + (size_t)pair * N * C;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float amax = 0.f;
  if (p.mean) {
    const int rows_per_slab = (N + p.nslab - 1) / p.nslab;
    const int r0 = slab * rows_per_slab;
    const int r1 = min(N, r0 + rows_per_slab);
    const f32x4 m = *reinterpret_cast<const f32x4*>(p.mean + mat * C + c4 * 4);
    if (rp < nrp)
      for (int r = r0 + rp; r < r1; r += nrp) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)r * C + c4 * 4);
        v -= m; acc += v * v;
      }
  } else {
    const int units = (N + 15) >> 4;
    const int ups = (units + p.nslab - 1) / p.nslab;
    const int u0 = slab * ups, u1 = min(units, u0 + ups);
    const float* U = p.u[b] ? p.u[b] + (size_t)pair * units * C : nullptr;
    if (rp < nrp)
      for (int u = u0 + rp; u < u1; u += nrp) {
        if (U) {
          acc += *reinterpret_cast<const f32x4*>(U + (size_t)u * C + c4 * 4);
        } else {
          f32x4 t[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int r = u * 16 + i;
            t[i] = *reinterpret_cast<const f32x4*>(x + (size_t)min(r, N - 1) * C + c4 * 4);
            if (r >= N) t[i] = f32x4{0.f, 0.f, 0.f, 0.f};            // ragged last unit: + 0 is exact
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(t[i][0]), fabsf(t[i][1]))), fmaxf(fabsf(t[i][2]), fabsf(t[i][3])));
          }
#pragma unroll
          for (int w = 1; w < 16; w <<= 1)
#pragma unroll
            for (int i = 0; i < 16; i += 2 * w) t[i] += t[i + w];
          acc += t[0];
        }
      }
    if (U) amax = __builtin_bit_cast(float, p.umax[b][pair * UMAX_SLOTS + (tid & (UMAX_SLOTS - 1))]);   // block max below
  }
  red[tid] = acc;
  __syncthreads();
  if (rp == 0) {
    for (int j = 1; j < nrp; ++j) acc += red[j * cq + c4];
    *reinterpret_cast<f32x4*>(p.partial + ((size_t)mat * p.nslab + slab) * C + c4 * 4) = acc;
  }
  if (p.absmax) {                            // block max (max is order-independent: deterministic)
    __syncthreads();
    float* redf = reinterpret_cast<float*>(red);
    redf[tid] = amax;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) redf[tid] = fmaxf(redf[tid], redf[tid + st]);
      __syncthreads();
    }
    if (tid == 0) p.absmax[(size_t)mat * p.nslab + slab] = redf[0];
  }
}

// scale[m] = 2^k with 2 * max|x| * 2^k in [8192, 16384): the centred features |x - mean| <= 2 max|x| then
// sit well inside the fp16 range, whatever the range of the fp32 input (1 if the input is all zero) -- computed by block 0 of
// colsum_finish_kernel (round 5; it was a launch of its own, cov_scale_kernel)
// out[m][c] = sum_slab partial / denom_side; with absmax / scale given, block 0 of a matrix also does cov_scale_kernel's job
// (round 5: one launch less per level)
__global__ void colsum_finish_kernel(const float* partial, float* out, int C, int nslab, float d0, float d1, int skip,
                                     const float* absmax = nullptr, float* scale = nullptr) {
  const int mat = blockIdx.y;
  if (skip_style_mat(mat, skip)) return;
  if (scale && blockIdx.x == 0 && threadIdx.x < 64) {
    float m = 0.f;
    for (int i = threadIdx.x; i < nslab; i += 64) m = fmaxf(m, absmax[(size_t)mat * nslab + i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) {
      float sc = 1.f;
      if (m > 0.f && m < 1e30f) {
        int e;
        frexpf(2.f * m, &e);                   // 2m = f * 2^e, f in [0.5, 1)
        sc = ldexpf(1.f, 14 - e);
      }
      scale[mat] = sc;
    }
  }
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  // eight independent partial sums keep eight loads in flight (a single dependent chain of up to 256 L2
  // round trips made this trivial kernel take 65 us); the order is fixed, so the result is reproducible
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* pp = partial + (size_t)mat * nslab * C + c;
  int i = 0;
  for (; i + 8 <= nslab; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += pp[(size_t)(i + j) * C];
  }
  for (; i < nslab; ++i) a[i & 7] += pp[(size_t)i * C];
  const float s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  out[mat * C + c] = s / ((mat & 1) == 0 ? d0 : d1);
}

// ---------------------------------------------------------------------------
// generic fp32 GEMM tile on v_mfma_f32_32x32x2_f32
//   D[m][n] = sum_k A(m,k) B(k,n)
// A element (m,k): a_kmajor ? A[k*lda+m] : A[m*lda+k];  B element (k,n): b_kmajor ? B[k*ldb+n] : B[n*ldb+k]
// ---------------------------------------------------------------------------
constexpr int GK = 16;

// one operand tile (GK x BX, k-major in LDS) moves global -> registers -> LDS in two phases so the
// loads of K-step t+1 are in flight while the MFMAs of step t run
template <int BX>
struct GemmStage {
  static constexpr int NV = GK * BX / 4 / 256;      // float4 per thread
  f32x4 v[NV];
  // kmajor: element (k, x) at src[k*ld + x];  else element (x, k) at src[x*ld + k]
  __device__ __forceinline__ void load(const float* src, int ld, bool kmajor, int k0, int kend, int x0, int X,
                                       const float* sub_x, const float* sub_k, const float* scale_k, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int item = tid + i * 256;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (kmajor) {
        const int k = item / (BX / 4), x4 = item % (BX / 4);
        const int gk = k0 + k, gx = x0 + x4 * 4;
        if (gk < kend && gx < X) {
          t = *reinterpret_cast<const f32x4*>(src + (size_t)gk * ld + gx);
          if (sub_x) t -= *reinterpret_cast<const f32x4*>(sub_x + gx);
        }
      } else {
        const int x = item / (GK / 4), k4 = item % (GK / 4);
        const int gx = x0 + x, gk = k0 + k4 * 4;
        if (gx < X && gk < kend) {          // K and ksplit are multiples of 4
          t = *reinterpret_cast<const f32x4*>(src + (size_t)gx * ld + gk);
          if (sub_k) t -= *reinterpret_cast<const f32x4*>(sub_k + gk);
          if (scale_k) t *= *reinterpret_cast<const f32x4*>(scale_k + gk);
        }
      }
      v[i] = t;
    }
  }
  __device__ __forceinline__ void store(float* lds /* [GK][BX+4] */, bool kmajor, int tid) const {
    constexpr int P = BX + 4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int item = tid + i * 256;
      if (kmajor) {
        const int k = item / (BX / 4), x4 = item % (BX / 4);
        *reinterpret_cast<f32x4*>(lds + k * P + x4 * 4) = v[i];
      } else {
        const int x = item / (GK / 4), k4 = item % (GK / 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds[(k4 * 4 + j) * P + x] = v[i][j];
      }
    }
  }
};

// Round 5: does the rotated matrix D + E the solver hands over need a REFRESH, E' = V^T A0 V recomputed from the eigenvectors
// and the untouched covariance?  The solver tracks the rotated matrix (fp32 tile updates, ~80 of them per element) and V (22-bit
// products, ~200 block rotations) separately, so V^T A0 V = D + E holds only to ~1e-6 ||A||.  The spectral functions take f(A0) =
// V f(D + E) V^T with E to first / second order: an inconsistency of 1e-6 ||A|| in E is harmless while the kept eigenvalues are
// within a few decades of the norm, and is the whole error (1e-3 .. 2e-3 of the transform, tests/test_gpu_fuzz.py wide bands) once
// kept eigenvalues sit 4+ decades below it -- rank-deficient covariances whose rounding noise the absolute 1e-5 cut-off keeps, gain
// up to 316.  With E' the identity f(A0) = V f(V^T A0 V) V^T is exact for orthogonal V whatever the sweeps left behind (NumPy model of
// the failing case: 3.3e-3 with the tracked E, 1.3e-6 with E', V in 22 bits either way).  Cost: two C^3 products per matrix that
// needs it, none for the others (the blocks of a batch whose predicate is false exit at once).
// Predicate (from the tracked diagonal = eigenvalue estimates): an eigenvalue that is kept, or within half a decade below the
// cut-off, and below 1e-4 of the largest.
constexpr float REFRESH_RATIO = 1e-4f;
__device__ __forceinline__ bool refresh_needed(const float* Am, int C, int tid) {     // all 256 threads of a block; contains barriers
  float dmax = 0.f, dmin = 3.0e38f;
  for (int i = tid; i < C; i += 256) {
    const float d = Am[(size_t)i * C + i];
    dmax = fmaxf(dmax, fabsf(d));
    // kept, or within half a decade below the cut-off (the `near` band of spectral_add2_all_kernel: its side of the cut-off is not settled)
    if (d > 3.3e-6f) dmin = fminf(dmin, d);
  }
  for (int o = 32; o > 0; o >>= 1) { dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64)); dmin = fminf(dmin, __shfl_xor(dmin, o, 64)); }
  __shared__ float red[2][4];
  if ((tid & 63) == 0) { red[0][tid >> 6] = dmax; red[1][tid >> 6] = dmin; }
  __syncthreads();
  dmax = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  dmin = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
  return dmin < 3.0e38f && dmin < REFRESH_RATIO * dmax;
}

template <int BM, int BN>
// (round 5: four blocks per CU -- 126 registers with the accumulators in VGPRs, 144 with AGPRs before: the tail's products
//  3.86 -> 3.81 ms per 32-pair step, bit-identical; a K-stage of 32 instead of 16 loses 0.4 ms: profiles/r05_gemm_variants.txt)
__global__ __launch_bounds__(256, 4) void gemm_f32_kernel(GemmArgs p) {
  constexpr int TM = BM / 64, TN = BN / 64;       // 32x32 MFMA tiles per wave (2x2 waves)
  constexpr int PA = BM + 4, PB = BN + 4;
  __shared__ __attribute__((aligned(16))) float As[GK * PA];
  __shared__ __attribute__((aligned(16))) float Bs[GK * PB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int batch = blockIdx.z / p.nsplit, split = blockIdx.z % p.nsplit;
  if (p.skip != WCT_SKIP_NONE && skip_style_mat(batch, p.skip)) return;
  if (p.mask_in && !p.mask_in[batch]) return;
  if (p.mask_diag) {                             // (uniform per block)
    const bool need = refresh_needed(p.mask_diag + batch * p.s_mask, p.M, tid);
    if (p.mask_out && blockIdx.x == 0 && blockIdx.y == 0 && split == 0 && tid == 0) p.mask_out[batch] = need ? 1 : 0;
    if (!need) return;
  }
  const int kbeg = split * p.ksplit;
  const int kend = min(p.K, kbeg + p.ksplit);
  if (p.A_odd) p.A = (batch & 1) ? p.A_odd + (batch >> 1) * p.sA_odd : p.A + (batch >> 1) * p.sA;
  else p.A += batch * p.sA;
  p.B += batch * p.sB;
  if (p.a_sub_m) p.a_sub_m += batch * p.s_sub_m;
  if (p.b_sub_n) p.b_sub_n += batch * p.s_sub_n;
  if (p.a_sub_k) p.a_sub_k += batch * p.s_sub_k;
  if (p.a_scale_k) p.a_scale_k += batch * p.s_scale_k;
  if (p.bias_n) p.bias_n += batch * p.s_bias;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  GemmStage<BM> sa;
  GemmStage<BN> sb;
  if (kbeg < kend) {
    sa.load(p.A, p.lda, p.a_kmajor, kbeg, kend, m0, p.M, p.a_sub_m, p.a_sub_k, p.a_scale_k, tid);
    sb.load(p.B, p.ldb, p.b_kmajor, kbeg, kend, n0, p.N, p.b_sub_n, nullptr, nullptr, tid);
  }
  for (int k0 = kbeg; k0 < kend; k0 += GK) {
    sa.store(As, p.a_kmajor, tid);
    sb.store(Bs, p.b_kmajor, tid);
    __syncthreads();
    if (k0 + GK < kend) {
      sa.load(p.A, p.lda, p.a_kmajor, k0 + GK, kend, m0, p.M, p.a_sub_m, p.a_sub_k, p.a_scale_k, tid);
      sb.load(p.B, p.ldb, p.b_kmajor, k0 + GK, kend, n0, p.N, p.b_sub_n, nullptr, nullptr, tid);
    }
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2) {
      float a[TM], b[TN];
      const int kr = kk + (lane >> 5);
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[kr * PA + (wm * TM + i) * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[kr * PB + (wn * TN + j) * 32 + (lane & 31)];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: reg r of a tile = row (r&3)+8*(r>>2)+4*(lane>>5), col lane&31
  float* o32 = p.out32 ? p.out32 + batch * p.s_out + (size_t)split * p.out_split_stride : nullptr;
  half_t* o16 = p.out16 ? p.out16 + batch * p.s_out : nullptr;
  float biasv[TN];                               // fetched before the first store (see conv_epilogue_t)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int gn = n0 + (wn * TN + j) * 32 + (lane & 31);
    biasv[j] = (p.bias_n && gn < p.N) ? p.bias_n[gn] : 0.f;
  }
  // ... and handed to the store loop as plain register values: hipcc otherwise re-issues `s_waitcnt vmcnt(0)` at the first
  // use in every predicated block, and each of those waits for all stores before it (64 serial round trips per thread)
#pragma unroll
  for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(biasv[j]));
  float av = 0.f;                                // blend epilogue: max |M| of this lane's elements
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int gn = n0 + (wn * TN + j) * 32 + (lane & 31);
      const float bias = biasv[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < p.M && gn < p.N) {
          float v = acc[i][j][r] + bias;
          if (p.blend) {                         // (uniform) what blend_matrix_kernel did to the stored T, element by element
            v = p.alpha * acc[i][j][r];
            if (gm == gn) v += 1.f - p.alpha;
            av = fmaxf(av, fabsf(v));
          }
          if (o32) o32[(size_t)gm * p.ldo + gn] = v;
          if (o16) o16[(size_t)gm * p.ldo + gn] = (half_t)v;
        }
      }
    }
  if (p.blend) {                                 // one atomic per wave; the maximum does not depend on the order
    for (int o = 32; o > 0; o >>= 1) av = fmaxf(av, __shfl_xor(av, o, 64));
    if (lane == 0 && av < 1e30f) atomicMax(p.mabs + batch, __float_as_uint(av));
  }
}

int launch_gemm(GemmArgs g, int nsplit, int nbatch, hipStream_t s) {
  g.nsplit = nsplit;
  const int gz = nsplit * nbatch;
  // few large tiles leave most of the chip idle when the batch is small (one pair's 512 x 512 products are 16 tiles of
  // 128 x 128 with a K loop of 512: 45 us apiece, 0.9 ms of a batch-1 frame); 64 x 64 tiles give four times the blocks.
  // Every output element is the same k-ordered fma chain under either tiling: the results are bit-identical.
  const bool small_grid = (long)cdiv(g.M, 128) * cdiv(g.N, 128) * gz < 256;
  if (g.M >= 128 && g.N >= 128 && !small_grid) {
    dim3 grid(cdiv(g.N, 128), cdiv(g.M, 128), gz);
    hipLaunchKernelGGL((gemm_f32_kernel<128, 128>), grid, dim3(256), 0, s, g);
  } else if (g.M >= 128 && !small_grid) {
    dim3 grid(cdiv(g.N, 64), cdiv(g.M, 128), gz);
    hipLaunchKernelGGL((gemm_f32_kernel<128, 64>), grid, dim3(256), 0, s, g);
  } else {
    dim3 grid(cdiv(g.N, 64), cdiv(g.M, 64), gz);
    hipLaunchKernelGGL((gemm_f32_kernel<64, 64>), grid, dim3(256), 0, s, g);
  }
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// ---------------------------------------------------------------------------
// K4: covariance partials  S[i][j] = sum_n (x[n][i]-m_i)(x[n][j]-m_j) s^2  on the fp16 MFMA pipe with
// split operands.  Every centred, scaled fp32 value v is split as v = hi + lo, hi = fp16(v),
// lo = fp16(v - hi) (the subtraction is exact): 22 significand bits, and hi*hi + hi*lo + lo*hi is
// accumulated in fp32 by three v_mfma_f32_32x32x16_f16 (the dropped lo*lo term is 2^-22 relative).  That
// is fp32-product accuracy at 3/16 of the fp32-MFMA time (v_mfma_f32_32x32x2_f32: 64 cycles for K=2).
// s is a power of two per matrix (colsum_finish_kernel) so no fp32 input can leave the fp16 range.
// Only tiles on or above the diagonal are computed (cov_finish_kernel mirrors); a diagonal tile stages
// its operand once.  Block = BT x BT tile, 256 threads = 2x2 waves; K-stage = 32 pixels.
// LDS operand image: [channel][32 k] fp16 = 64-B rows, 16-B pieces XOR-swizzled as in the conv kernel.
// ---------------------------------------------------------------------------
struct CovArgs {
  const float* x[2];     // content base [P][Nc][C], style base [P][Ns][C]
  int n[2];
  const float* mean;     // [2P][C]
  const float* scale;    // [2P]
  float* partial;        // [2P][nsplit][C][C]
  int C, ksplit, nsplit, ntile;   // ntile = tiles per side
  WctSkip skip;
};

template <int BT>
__global__ __launch_bounds__(256, 2) void cov_f16x2_kernel(CovArgs p) {
  constexpr int TM = BT / 64;                  // 32x32 MFMA tiles per wave and side
  constexpr int KPT = BT * 32 / 256;           // k values staged per thread and operand (16 or 8)
  constexpr int NPC = KPT / 8;                 // 16-B pieces per thread and operand half
  __shared__ __attribute__((aligned(16))) unsigned char lds[4][BT * 64];   // A hi, A lo, B hi, B lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // upper-triangular tile index -> (ti <= tj)
  int ti = 0, rem = blockIdx.x;
  while (rem >= p.ntile - ti) { rem -= p.ntile - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int m0 = ti * BT, n0 = tj * BT;
  const int mat = blockIdx.z, split = blockIdx.y;
  if (skip_style_mat(mat, p.skip)) return;
  const int side = mat & 1, pair = mat >> 1;
  const int N = p.n[side], C = p.C;
  const float* x = p.x[side] + (size_t)pair * N * C;
  const int kbeg = split * p.ksplit;
  const int kend = min(N, kbeg + p.ksplit);
  const float sc = p.scale[mat];

  // staging role: channel c of the tile, k-group kg (wave-uniform).  Loads go through a buffer resource
  // (32-bit lane offset + scalar row offset, rows past N read 0, no branches around the loads).  Rows past
  // the slice end get a zero scale (scalar select), so they contribute exactly 0; channels past C (ragged
  // tile) produce values that the store mask drops.
  const int c = tid % BT;
  const int kg = __builtin_amdgcn_readfirstlane(tid / BT);
  const float mean_a = p.mean[mat * C + min(m0 + c, C - 1)];
  const float mean_b = p.mean[mat * C + min(n0 + c, C - 1)];
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)((size_t)N * C * 4), 0x00020000);
  const int voff_a = min(m0 + c, C - 1) * 4, voff_b = min(n0 + c, C - 1) * 4;

  f32x16 acc[TM][TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto load = [&](float (&r)[KPT], int voff, int k0) {
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      r[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (k0 + kg * KPT + j) * C * 4, 0));
  };
  // split (x - mean) * s into fp16 hi + lo and park the 16-B pieces in the swizzled LDS image
  // (`tail`: the stage straddles the slice end; rows past it get a zero scale -- a uniform select that only
  //  the last stage of a slice pays for)
  auto split_store = [&](const float (&r)[KPT], float mean, int k0, bool tail, unsigned char* hi, unsigned char* lo) {
#pragma unroll
    for (int q = 0; q < NPC; ++q) {
      half8 h, l;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s_in = (!tail || k0 + kg * KPT + q * 8 + j < kend) ? sc : 0.f;
        const float v = (r[q * 8 + j] - mean) * s_in;
        h[j] = (half_t)v;
        l[j] = (half_t)(v - (float)h[j]);
      }
      const int chunk = kg * NPC + q;          // 16-B piece (8 k values) within the 64-B row
      const int off = (c * 4 + (chunk ^ ((c >> 2) & 3))) * 16;
      *reinterpret_cast<half8*>(hi + off) = h;
      *reinterpret_cast<half8*>(lo + off) = l;
    }
  };
  auto mma_stage = [&](const unsigned char* bh, const unsigned char* bl) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int chunk = ks * 2 + (lane >> 5);
      half8 ah[TM], al[TM], bhf[TM], blf[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = (wm * TM + i) * 32 + (lane & 31);
        const int off = (r * 4 + (chunk ^ ((r >> 2) & 3))) * 16;
        ah[i] = *reinterpret_cast<const half8*>(lds[0] + off);
        al[i] = *reinterpret_cast<const half8*>(lds[1] + off);
      }
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int r = (wn * TM + j) * 32 + (lane & 31);
        const int off = (r * 4 + (chunk ^ ((r >> 2) & 3))) * 16;
        bhf[j] = *reinterpret_cast<const half8*>(bh + off);
        blf[j] = *reinterpret_cast<const half8*>(bl + off);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bhf[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], blf[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bhf[j], acc[i][j], 0, 0, 0);
        }
    }
  };

  float ra[KPT], rb[KPT];
  if (diag) {                                  // one operand: the tile is its own transpose partner
    if (kbeg < kend) load(ra, voff_a, kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
      if (k0 + 32 <= kend) split_store(ra, mean_a, k0, false, lds[0], lds[1]);
      else split_store(ra, mean_a, k0, true, lds[0], lds[1]);
      __syncthreads();
      if (k0 + 32 < kend) load(ra, voff_a, k0 + 32);
      mma_stage(lds[0], lds[1]);
      __syncthreads();
    }
  } else {
    if (kbeg < kend) { load(ra, voff_a, kbeg); load(rb, voff_b, kbeg); }
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
      if (k0 + 32 <= kend) {
        split_store(ra, mean_a, k0, false, lds[0], lds[1]);
        split_store(rb, mean_b, k0, false, lds[2], lds[3]);
      } else {
        split_store(ra, mean_a, k0, true, lds[0], lds[1]);
        split_store(rb, mean_b, k0, true, lds[2], lds[3]);
      }
      __syncthreads();
      if (k0 + 32 < kend) { load(ra, voff_a, k0 + 32); load(rb, voff_b, k0 + 32); }
      mma_stage(lds[2], lds[3]);
      __syncthreads();
    }
  }

  // reg r of a tile = row (r&3)+8*(r>>2)+4*(lane>>5), col lane&31
  float* out = p.partial + ((size_t)mat * p.nsplit + split) * C * C;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int gn = n0 + (wn * TM + j) * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < C && gn < C) out[(size_t)gm * C + gn] = acc[i][j][r];
      }
    }
}

// cov[m] = sum_split partial / (scale_m^2 (N_m - 1)) + eps I; entries below the diagonal tiles are the
// mirror of the computed upper tiles (BT = tile side of the partials)
// (round 4: in 64 x 64 tiles -- a tile below the diagonal of the BT grid reads its mirror tile's rows, coalesced, and turns
//  them in LDS; element by element the lower triangle walked columns of every partial.  Same sums in the same order.)
// grid (C / 64, C / 64, 2P)
__global__ __launch_bounds__(256) void cov_finish_kernel(const float* partial, const float* scale, float* cov, int C, int nsplit, int BT,
                                                         float inv0, float inv1, float eps, int skip, float* cov0 = nullptr) {
  __shared__ float tt[64][65];
  const int mat = blockIdx.z;             // 2*pair + side
  if (skip_style_mat(mat, skip)) return;
  const size_t cc = (size_t)C * C;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const bool mirror = r0 / BT > c0 / BT;  // (uniform: BT is a multiple of 64)
  const float* pb = partial + (size_t)mat * nsplit * cc;
  const float sc = scale[mat];
  const float f = ((mat & 1) == 0 ? inv0 : inv1) / (sc * sc);
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // direct: element (r0 + 4 ty + i, c0 + 4 tx ..); mirror: element (c0 + 4 ty + i, r0 + 4 tx ..) of the upper triangle
    const int r = (mirror ? c0 : r0) + ty * 4 + i, c = (mirror ? r0 : c0) + tx * 4;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (r < C && c < C)
      for (int k = 0; k < nsplit; ++k) sum += *reinterpret_cast<const f32x4*>(pb + (size_t)k * cc + (size_t)r * C + c);
    acc[i] = sum;
  }
  if (mirror) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tt[ty * 4 + i][tx * 4 + j] = acc[i][j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = tt[tx * 4 + j][ty * 4 + i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty * 4 + i, c = c0 + tx * 4;
    if (r >= C || c >= C) continue;
    f32x4 v = acc[i] * f;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (r == c + j) v[j] += eps;
    *reinterpret_cast<f32x4*>(cov + (size_t)mat * cc + (size_t)r * C + c) = v;
    if (cov0) *reinterpret_cast<f32x4*>(cov0 + (size_t)mat * cc + (size_t)r * C + c) = v;     // (the copy the solver does not rotate: refresh_needed)
  }
}

// ---------------------------------------------------------------------------
// K4 at relu1_1, from the IMAGE: the rows of the level-1 feature matrix are what conv1_1 makes of a 3x3 image patch (27
// multiply-adds from 12 bytes a pixel), so the block computes them instead of reading 256 bytes a pixel.  Grid (1, nsplit, 2P),
// the K-slices, skip rule, partial layout and finish of cov_f16x2_kernel<64>; its diagonal tile is the whole 64 x 64 matrix.
// A block stage is 128 rows: wave w computes relu1_1 of rows k0 + 32 w .. + 31 (pixel (k / W, k % W), patch values straight from
// the image, reflected as conv_first_kernel reflects them) with conv_first_tile.h's arithmetic, operands swapped so that a lane
// holds 4 consecutive pixels of one channel, centres, scales and splits them as split_store does and parks them in k-stage w of
// the [channel][32 k] LDS image (8-byte stores).  Every wave then runs the covariance MFMAs of its 32 x 32 tile over the four
// k-stages in order: the products and their order are cov_f16x2_kernel<64>'s, so the partials are equal bit for bit.
// Rows past the slice end get a zero scale (exact zeros), k-stages that start past it are left out.
// ---------------------------------------------------------------------------
struct CovImageArgs {
  WctImageSrc src;
  const float* mean;     // [2P][64]
  const float* scale;    // [2P]
  float* partial;        // [2P][nsplit][64][64]
  int ksplit, nsplit;
  WctSkip skip;
};

__global__ __launch_bounds__(256, 2) void cov_image_kernel(CovImageArgs p) {
  constexpr int C = 64;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4][2][C * 64];   // per k-stage: hi, lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int mat = blockIdx.z, split = blockIdx.y;
  if (skip_style_mat(mat, p.skip)) return;
  const int side = mat & 1, pair = mat >> 1;
  const int H = side ? p.src.side[1].H : p.src.side[0].H, W = side ? p.src.side[1].W : p.src.side[0].W;
  const int clamp01 = side ? p.src.side[1].clamp01 : p.src.side[0].clamp01;
  const int N = H * W;
  const float* x = (side ? p.src.side[1].img : p.src.side[0].img) + (size_t)pair * N * 3;
  const int kbeg = split * p.ksplit;
  const int kend = min(N, kbeg + p.ksplit);
  const float sc = p.scale[mat];
  const int kgrp = lane >> 5, ch = lane & 31;    // this lane's channels: nt * 32 + ch

  half8 wh[2][2], wl[2][2];
  conv1_weights(p.src.wfrag, lane, wh, wl);
  float bias[2], mean[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) { bias[nt] = p.src.bias[nt * 32 + ch]; mean[nt] = p.mean[mat * C + nt * 32 + ch]; }

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // the 16 patch values of this lane's pixel at k = ks * 16 + kgrp * 8 + j (k >= 27 reads a valid address and is zeroed when it
  // is used).  The pixel (py, px) is row kbeg + 32 wave + (lane & 31) of the matrix and moves on by 128 rows a stage; a row
  // past the image (the last stage of the last slice) reads the last image row: it is scaled by zero.
  float pre[2][8];
  int py, px;
  {
    const int n = kbeg + wave * 32 + (lane & 31);
    py = n / W; px = n - py * W;
  }
  auto fetch = [&]() {
    conv1_patch_load(x, min(py, H - 1), px, H, W, kgrp, pre);
    px += 128;                                   // the next stage's pixel
    while (px >= W) { px -= W; ++py; }
  };
  auto mma_stage = [&](const unsigned char* hi, const unsigned char* lo) {     // cov_f16x2_kernel<64>'s, a diagonal tile
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int chunk = ks * 2 + (lane >> 5);
      const int ra = wm * 32 + (lane & 31), rb = wn * 32 + (lane & 31);
      const int offa = (ra * 4 + (chunk ^ ((ra >> 2) & 3))) * 16, offb = (rb * 4 + (chunk ^ ((rb >> 2) & 3))) * 16;
      const half8 ah = *reinterpret_cast<const half8*>(hi + offa), al = *reinterpret_cast<const half8*>(lo + offa);
      const half8 bh = *reinterpret_cast<const half8*>(hi + offb), bl = *reinterpret_cast<const half8*>(lo + offb);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
    }
  };

  // relu1_1 of the k-stage, centred, scaled and split as split_store does, into k-stage `wave` of the LDS image (TAIL: the
  // stage straddles the slice end; rows past it get a zero scale)
  auto park = [&](const f32x16 (&f)[2], int ks0, auto tail) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int c = nt * 32 + ch;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        half4 h, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float s_in = (!decltype(tail)::value || ks0 + rq * 8 + kgrp * 4 + j < kend) ? sc : 0.f;
          const float v = (conv1_act(f[nt][rq * 4 + j], bias[nt]) - mean[nt]) * s_in;
          h[j] = (half_t)v;
          l[j] = (half_t)(v - (float)h[j]);
        }
        const int off = (c * 4 + (rq ^ ((c >> 2) & 3))) * 16 + kgrp * 8;     // k = rq * 8 + kgrp * 4 + j of the k-stage
        *reinterpret_cast<half4*>(lds[wave][0] + off) = h;
        *reinterpret_cast<half4*>(lds[wave][1] + off) = l;
      }
    }
  };

  if (kbeg + wave * 32 < kend) fetch();          // (wave-uniform: does this wave's k-stage hold rows of the slice?)
  for (int k0 = kbeg; k0 < kend; k0 += 128) {
    const int ks0 = k0 + wave * 32;
    if (ks0 < kend) {
      // this stage's values out of the landing registers, the next stage's loads into them: a whole stage ahead of their use
      float cur[2][8];
      conv1_patch_values(pre, kgrp, clamp01, cur);
      if (ks0 + 128 < kend) fetch();
      f32x16 f[2];
      conv1_tile<true>(wh, wl, [=](int ks, int j) { return cur[ks][j]; }, f);
      if (ks0 + 32 <= kend) park(f, ks0, std::false_type());
      else park(f, ks0, std::true_type());
    }
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 4; ++st)
      if (k0 + st * 32 < kend) mma_stage(lds[st][0], lds[st][1]);      // (uniform)
    __syncthreads();
  }

  // reg r of the tile = row (r&3)+8*(r>>2)+4*(lane>>5), col lane&31
  float* out = p.partial + ((size_t)mat * p.nsplit + split) * C * C;
  const int gn = wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gm = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    out[(size_t)gm * C + gn] = acc[r];
  }
}

// The statistics passes over the nmat matrices of a grid -- the 2P matrices of a batch (launch_means), or one slot of a plan on
// a one-matrix grid, pointed at the slot (launch_slot_means): sa with its inputs, partial / absmax buffers and skip mode set;
// the means and the fp16 scale into mean / scale and, var given, the variances; d0 / d1: the rows of an even / odd matrix
static int stat_passes(StatArgs sa, int nmat, float* mean, float* var, float* scale, float d0, float d1, hipStream_t s) {
  const int C = sa.C;
  sa.mean = nullptr;
  hipLaunchKernelGGL(colsum_kernel, dim3(sa.nslab, nmat), dim3(256), 0, s, sa);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv(C, 256), nmat), dim3(256), 0, s, sa.partial, mean, C, sa.nslab, d0, d1, (int)sa.skip,
                     (const float*)sa.absmax, scale);
  if (var) {
    sa.mean = mean; sa.absmax = nullptr;
    hipLaunchKernelGGL(colsum_kernel, dim3(sa.nslab, nmat), dim3(256), 0, s, sa);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv(C, 256), nmat), dim3(256), 0, s, sa.partial, var, C, sa.nslab, d0, d1, (int)sa.skip,
                       (const float*)nullptr, (float*)nullptr);
  }
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_means(const float* content, int Nc, const float* style, int Ns, int C, int P, const WctCarve& w, bool with_var, WctSkip skip,
                 hipStream_t s, const WctFeatStats* fs) {
  StatArgs sa;
  sa.x[0] = content; sa.x[1] = style; sa.n[0] = Nc; sa.n[1] = Ns;
  for (int b = 0; b < 2; ++b) {
    sa.u[b] = fs && fs->umax[b] ? fs->u[b] : nullptr;
    sa.umax[b] = sa.u[b] ? fs->umax[b] : nullptr;
  }
  sa.partial = w.stat_partial; sa.absmax = w.absmax; sa.C = C; sa.nslab = w.nslab; sa.skip = skip;
  return stat_passes(sa, 2 * P, w.mean, with_var ? w.var : nullptr, w.scale, (float)Nc, (float)Ns, s);
}

// The covariance passes over the nmat matrices of a grid, as stat_passes: the partials of ca (matrix 2p + side, side 0 =
// content, 1 = style; slices past a side's N write zeros), then their sum into A and A0 with eps on the diagonal; inv0 / inv1:
// 1 / (rows - 1) of an even / odd matrix
static int cov_passes(CovArgs ca, int nmat, float* A, float* A0, float inv0, float inv1, float eps, hipStream_t s) {
  const int C = ca.C, BT = C >= 128 ? 128 : 64;
  ca.ntile = cdiv(C, BT);
  dim3 grid(ca.ntile * (ca.ntile + 1) / 2, ca.nsplit, nmat);
  if (BT == 128) hipLaunchKernelGGL((cov_f16x2_kernel<128>), grid, dim3(256), 0, s, ca);
  else hipLaunchKernelGGL((cov_f16x2_kernel<64>), grid, dim3(256), 0, s, ca);
  hipLaunchKernelGGL(cov_finish_kernel, dim3(cdiv(C, 64), cdiv(C, 64), nmat), dim3(256), 0, s, ca.partial, ca.scale, A, C, ca.nsplit, BT,
                     inv0, inv1, eps, (int)ca.skip, A0);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_cov(const float* content, int Nc, const float* style, int Ns, int C, int P, const WctCarve& w, float eps, WctSkip skip,
               hipStream_t s) {
  CovArgs ca;
  ca.x[0] = content; ca.x[1] = style; ca.n[0] = Nc; ca.n[1] = Ns;
  ca.mean = w.mean; ca.scale = w.scale; ca.partial = w.cov_partial;
  ca.C = C; ca.ksplit = w.ksplit; ca.nsplit = w.nsplit; ca.skip = skip;
  return cov_passes(ca, 2 * P, w.A, w.A0, 1.f / (float)(Nc - 1), 1.f / (float)(Ns - 1), eps, s);
}

// launch_cov at relu1_1 with both sides' rows computed from their images (cov_image_kernel), the same finish
int launch_cov_image(const WctImageSrc& src, int P, const WctCarve& w, float eps, WctSkip skip, hipStream_t s) {
  constexpr int C = 64;
  for (int b = 0; b < 2; ++b) ARG_CHECK(src.side[b].img && src.side[b].H >= 2 && src.side[b].W >= 16 && src.side[b].W % 16 == 0);
  ARG_CHECK(src.wfrag && src.bias && w.ksplit % 32 == 0);
  const int Nc = src.side[0].H * src.side[0].W, Ns = src.side[1].H * src.side[1].W;
  CovImageArgs ca;
  ca.src = src; ca.mean = w.mean; ca.scale = w.scale; ca.partial = w.cov_partial;
  ca.ksplit = w.ksplit; ca.nsplit = w.nsplit; ca.skip = skip;
  hipLaunchKernelGGL(cov_image_kernel, dim3(1, w.nsplit, 2 * P), dim3(256), 0, s, ca);
  hipLaunchKernelGGL(cov_finish_kernel, dim3(1, 1, 2 * P), dim3(256), 0, s, ca.partial, ca.scale, w.A, C, ca.nsplit, 64,
                     1.f / (float)(Nc - 1), 1.f / (float)(Ns - 1), eps, (int)skip, w.A0);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// first statistics pass (means, the fp16 scale; with_var: the variances) of ONE matrix, slot `m` of the workspace, with its own
// slab count; u / umax: its unit sums from a conv epilogue, or null
static int launch_slot_means(const float* x, int N, int C, int m, int nslab, const WctCarve& w, bool with_var, hipStream_t s,
                             const float* u, const unsigned* umax) {
  StatArgs sa = {};
  sa.x[0] = sa.x[1] = x; sa.n[0] = sa.n[1] = N;
  sa.u[0] = umax ? u : nullptr; sa.umax[0] = sa.u[0] ? umax : nullptr;
  sa.partial = w.stat_partial + (size_t)m * w.nslab * C; sa.absmax = w.absmax + (size_t)m * w.nslab;
  sa.C = C; sa.nslab = nslab; sa.skip = WCT_SKIP_NONE;
  return stat_passes(sa, 1, w.mean + (size_t)m * C, with_var ? w.var + (size_t)m * C : nullptr, w.scale + m, (float)N, (float)N, s);
}

// covariance of ONE matrix into slot m (A and A0), K-slices of its own layout
static int launch_slot_cov(const float* x, int N, int C, int m, int nsplit, int ksplit, float eps, const WctCarve& w, hipStream_t s) {
  const size_t cc = (size_t)C * C;
  CovArgs ca;
  ca.x[0] = ca.x[1] = x; ca.n[0] = ca.n[1] = N;
  ca.mean = w.mean + (size_t)m * C; ca.scale = w.scale + m; ca.partial = w.cov_partial + (size_t)m * w.nsplit * cc;
  ca.C = C; ca.ksplit = ksplit; ca.nsplit = nsplit; ca.skip = WCT_SKIP_NONE;
  return cov_passes(ca, 1, w.A + m * cc, w.A0 + m * cc, 1.f / (float)(N - 1), 1.f / (float)(N - 1), eps, s);
}

// the statistics stage of a plan, slot by slot in index order (the skipped slots left out): means and the fp16 scale, with_var
// the variances, with_cov the covariance (eps on its diagonal) into A and A0
int launch_plan_stats(const SlotPlan& sp, int C, bool with_var, bool with_cov, float eps, hipStream_t s) {
  int rc;
  for (int m = 0; m < 2 * sp.P; ++m) {
    const SlotPlan::Slot& t = sp.slot[m];
    if (!t.n) continue;
    if ((rc = launch_slot_means(t.x, t.n, C, m, t.lay.nslab, sp.w, with_var, s, m ? nullptr : sp.u0, m ? nullptr : sp.umax0))) return rc;
    if (with_cov && (rc = launch_slot_cov(t.x, t.n, C, m, t.lay.nsplit, t.lay.ksplit, eps, sp.w, s))) return rc;
  }
  return WCT_OK;
}
