// Video warm start: the content eigensolve of a level starts from the eigenvectors V0 of an earlier frame instead of
// the identity.  The solver is not touched: the covariance is rotated into the old basis, A' = V0^T A V0 (nearly diagonal for a
// slowly varying video), the batched solver runs on A' from the identity as it always does and gives V', and V = V0 V' is what
// the spectral tail takes -- with the rotated A' and the untouched A0 exactly as after a cold solve.  The basis kept for the next
// call is re-orthonormalised by one Newton-Schulz step, V <- V (3 I - V^T V) / 2, so that the orthogonality error of a solve
// (~3e-5) does not add up over the frames of a video.
//
// ONE kernel family, five products, all on v_mfma_f32_32x32x2_f32 with the blocking of gemm_f32_kernel (stats_gemm.hip): 64 x 64
// tiles, 2 x 2 waves, K-stage 16, operands global -> registers -> LDS with the next stage's loads in flight.  fp32: the study
// (tools/probe/warm_congruence_study.py, profiles/warm_congruence_study.txt) finds no case in which float64 or the split-fp16
// products move the transform's error, because the tail re-derives the rotated matrix from (A0, V) wherever the spectrum is graded
// enough to notice (launch_refresh).  Every output element is one k-ordered fma chain whatever the batch: a matrix's result does
// not depend on its neighbours in the launch.
#include "wct_stages.h"

namespace {

constexpr int WK = 16;            // K-stage
constexpr int WT = 64;            // tile
constexpr int WP = WT + 4;        // LDS row pitch (floats)

struct WarmGemmArgs {
  const float* A; size_t sA; int a_kmajor;   // A(m, k) = a_kmajor ? A[k * C + m] : A[m * C + k]; sA: elements between batches (0: shared)
  const float* B; size_t sB;                 // B(k, n) = B[k * C + n]
  float* out; size_t s_out;                  // out[m * C + n]
  int C;
  int sym;                                   // the product is symmetric: tiles g <= h only, every element stored to both sides
  int ns;                                    // Newton-Schulz epilogue: out = 1.5 I - 0.5 D
};

// one 16 x 64 operand stage: a float4 per thread
struct WarmStage {
  f32x4 v;
  __device__ __forceinline__ void load(const float* src, int C, bool kmajor, int k0, int x0, int tid) {
    v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kmajor) {
      const int k = tid >> 4, gx = x0 + (tid & 15) * 4;           // (C is a multiple of 32: a float4 is inside or outside)
      if (gx < C) v = *reinterpret_cast<const f32x4*>(src + (size_t)(k0 + k) * C + gx);
    } else {
      const int gx = x0 + (tid >> 2), gk = k0 + (tid & 3) * 4;
      if (gx < C) v = *reinterpret_cast<const f32x4*>(src + (size_t)gx * C + gk);
    }
  }
  __device__ __forceinline__ void store(float* lds, bool kmajor, int tid) const {
    if (kmajor) *reinterpret_cast<f32x4*>(lds + (tid >> 4) * WP + (tid & 15) * 4) = v;
    else {
      const int x = tid >> 2, k4 = (tid & 3) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) lds[(k4 + j) * WP + x] = v[j];
    }
  }
};

// grid (tiles, 1, batch); sym: the tiles of the upper triangle, row by row
__global__ __launch_bounds__(256) void warm_gemm_kernel(WarmGemmArgs p) {
  __shared__ __attribute__((aligned(16))) float As[WK * WP];
  __shared__ __attribute__((aligned(16))) float Bs[WK * WP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int C = p.C, nt = (C + WT - 1) / WT;
  int ti, tj;
  if (p.sym) {
    ti = 0;
    int t = blockIdx.x;
    while (t >= nt - ti) { t -= nt - ti; ++ti; }
    tj = ti + t;
  } else {
    ti = blockIdx.x / nt; tj = blockIdx.x % nt;
  }
  const int m0 = ti * WT, n0 = tj * WT;
  const float* A = p.A + blockIdx.z * p.sA;
  const float* B = p.B + blockIdx.z * p.sB;
  float* out = p.out + blockIdx.z * p.s_out;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  WarmStage sa, sb;
  sa.load(A, C, p.a_kmajor, 0, m0, tid);
  sb.load(B, C, true, 0, n0, tid);
  for (int k0 = 0; k0 < C; k0 += WK) {              // (C is a multiple of 32)
    sa.store(As, p.a_kmajor, tid);
    sb.store(Bs, true, tid);
    __syncthreads();
    if (k0 + WK < C) {
      sa.load(A, C, p.a_kmajor, k0 + WK, m0, tid);
      sb.load(B, C, true, k0 + WK, n0, tid);
    }
#pragma unroll
    for (int kk = 0; kk < WK; kk += 2) {
      const int kr = kk + (lane >> 5);
      const float a = As[kr * WP + wm * 32 + (lane & 31)];
      const float b = Bs[kr * WP + wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }

  // reg r = row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), col lane & 31
  const int gn = n0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (gm >= C || gn >= C) continue;
    float v = acc[r];
    if (p.ns) v = (gm == gn ? 1.5f : 0.f) - 0.5f * v;
    if (p.sym) {
      if (gm > gn) continue;                        // (a diagonal tile: the upper side is the one that is kept)
      out[(size_t)gn * C + gm] = v;
    }
    out[(size_t)gm * C + gn] = v;
  }
}

int warm_gemm(const WarmGemmArgs& a, int nbatch, hipStream_t s) {
  const int nt = cdiv(a.C, WT);
  const int tiles = a.sym ? nt * (nt + 1) / 2 : nt * nt;
  hipLaunchKernelGGL(warm_gemm_kernel, dim3(tiles, 1, nbatch), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

}  // namespace

// A' = V0^T A V0 for the content matrices (slots 2p) of w, in place in w.A; w.X is scratch.  V0: one basis for all P.
int launch_warm_rotate(const WctCarve& w, int C, int P, const float* V0, hipStream_t s) {
  const size_t cc = (size_t)C * C;
  int rc;
  WarmGemmArgs l = {w.A, 2 * cc, 0, V0, 0, w.X, 2 * cc, C, 0, 0};            // X = A V0
  if ((rc = warm_gemm(l, P, s))) return rc;
  WarmGemmArgs r = {V0, 0, 1, w.X, 2 * cc, w.A, 2 * cc, C, 1, 0};            // A' = V0^T X, symmetric to the bit
  return warm_gemm(r, P, s);
}

// V = V0 V' for the content matrices of w: w.V holds V' and gets V; w.X is scratch
int launch_warm_compose(const WctCarve& w, int C, int P, const float* V0, hipStream_t s) {
  const size_t cc = (size_t)C * C;
  int rc;
  WarmGemmArgs g = {V0, 0, 0, w.V, 2 * cc, w.X, 2 * cc, C, 0, 0};
  if ((rc = warm_gemm(g, P, s))) return rc;
  HIP_TRY(hipMemcpy2DAsync(w.V, 2 * cc * sizeof(float), w.X, 2 * cc * sizeof(float), cc * sizeof(float), P, hipMemcpyDeviceToDevice, s));
  return WCT_OK;
}

// basis <- V (3 I - V^T V) / 2 for the C x C matrix V (one Newton-Schulz step); scratch: C x C floats
int launch_warm_store(const float* V, float* scratch, float* basis, int C, hipStream_t s) {
  int rc;
  WarmGemmArgs g = {V, 0, 1, V, 0, scratch, 0, C, 1, 1};                      // S = 1.5 I - 0.5 V^T V
  if ((rc = warm_gemm(g, 1, s))) return rc;
  WarmGemmArgs n = {V, 0, 0, scratch, 0, basis, 0, C, 0, 0};                  // basis = V S
  return warm_gemm(n, 1, s);
}
