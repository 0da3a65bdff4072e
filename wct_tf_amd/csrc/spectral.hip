// K6 of the whiten-colour transform (the stage list: wct.hip): the spectral functions of the solved covariances, for all
// matrices of a level in merged launches (the transforms and style-swap alike), and the refresh before them.
#include "wct_stages.h"

// ---------------------------------------------------------------------------
// K6: spectral functions with the reference cut-off
// ---------------------------------------------------------------------------
// First-order completion of the matrix function (Daleckii-Krein): the sweeps stop with A = D + E, E a small
// off-diagonal residual (|e_pq| up to ~tol sqrt(d_p d_q)), and V^T A0 V = D + E holds to round-off, so
//   f(A0) = V f(D + E) V^T = V (f(D) + F o E) V^T + O(|E|^2),  F_pq = (f(d_p) - f(d_q)) / (d_p - d_q).
// Using G = f(D) + F o E instead of f(D) squares the error the residual leaves in the transform (measured on the
// level features of a 512x512 frame: 2.7e-3 -> see DESIGN) and lets the sweeps stop a whole sweep earlier.
// f is the reference's spectral function INCLUDING its cut-off (ops.py:68-77 / 112-127): f(l) = 0 for l <= 1e-5,
// else l^-1/2 | l^1/2 (wct_tf), (l + eps)^-1/2 | (l + eps)^1/2 (wct_np).  The divided differences of l^+-1/2 have
// closed forms without cancellation: -1 / (sa sb (sa + sb)) and 1 / (sa + sb) with sa = sqrt(a), sb = sqrt(b);
// across the cut-off (one eigenvalue kept, one dropped) F_pq = f(d_kept) / (d_kept - d_dropped).
// `kind`: 0 whitening gain l^-1/2, 1 colouring gain l^1/2.   G [nmat][C][C], as A.
// Round 6: the expansion is one in the squared cosines e^2 / (d_p d_q), and it is only used where it converges.  The sweeps may
// stop with pairs that are NOT resolved: the rounding-noise diagonals of a rank-deficient covariance (N < C pixels) never settle
// against each other (the lenient rule of jacobi_check_end lets such a matrix go), and when the feature scale puts that noise
// above the 1e-5 cut-off -- 1e-7 ||cov|| ~ 1 at features of ~1e3 -- those diagonals are KEPT, with squared cosines of order one
// and more among them.  The second divided differences then grow like f(a) e^2 / (2 d_a d_b) per term: measured on
// C = 256, 84 / 78 pixels, features ~1e3 (tools/probe/r06_fuzz_case.py, profiles/r06_noise_block.txt) the transform was off by
// 0.14 .. 11.5 (six seeds of six).  A pair with e^2 > d_p d_q / 4 takes no part in either order of the completion: f of its two
// diagonals stands alone (0.02 .. 0.15 on the same six; the rest is spectral_cut's, below).  On a matrix that met the stop test
// no pair is near that bound (the test bounds the mean over the rows of a row's SUM of squared cosines by 1.6e-3), so every
// converged result keeps its bits.
__device__ __forceinline__ bool pair_resolved(float dp, float dq, float e) { return e * e <= 0.25f * dp * dq; }

// The cut-off of ONE matrix (round 6).  The reference drops eigenvalues <= 1e-5 (ops.py:68-69 / 112,125).  A covariance is positive
// semi-definite in exact arithmetic, so a NEGATIVE diagonal of the rotated matrix is rounding noise and nothing else, and the most
// negative one, -r, measures the noise of this evaluation on this matrix (N < C pixels: C - N + 1 directions of exact zeros come
// out as a cluster symmetric around 0, radius r ~ 1.5e-7 ||cov||).  A positive diagonal no larger than 2 r is the same noise: it is
// dropped like the exact zero it stands for -- cut = max(1e-5, 2 r).  Below a feature scale of ~10 (r < 5e-6) this is the
// reference's cut-off unchanged; above it the noise directions, which the absolute 1e-5 would keep with gains (d + eps)^-1/2
// that dwarf the signal's, no longer enter.  Why it is needed (profiles/r06_noise_block.txt: C = 256, 84 / 78 pixels, features
// ~1e3, six seeds; error of the transform against the float64 oracle, the reference's own float32 evaluation 1.3e-4 .. 7e-4):
// diagonal gains only 3.5e-3 .. 1.9e-2, with the first-order completion 5e-2 .. 1.3, with the second-order one 0.35 .. 16.
// The kept count stays inside the band the parity tests accept as the reference's (tests/test_gpu_fuzz.py: eigenvalues within
// 2e-6 + 1e-6 ||cov|| of 1e-5 may fall on either side in float32).  Block-wide (256 threads), `red`: 4 floats of LDS.
constexpr float SPECTRAL_NOISE_CUT = 2.f;
__device__ __forceinline__ float spectral_cut(const float* Am, int C, int tid, float* red) {
  float mn = 0.f;
  for (int i = tid; i < C; i += 256) mn = fminf(mn, Am[(size_t)i * C + i]);
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mn;
  __syncthreads();
  mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  return fmaxf(1e-5f, -SPECTRAL_NOISE_CUT * mn);
}

__device__ __forceinline__ float spectral_entry(float dp, float dq, float e, bool diag, int kind, float shift, float cut) {
  const bool kp = dp > cut, kq = dq > cut;
  if (diag) return kp ? (kind == 0 ? 1.f / sqrtf(dp + shift) : sqrtf(dp + shift)) : 0.f;
  if (!kp && !kq) return 0.f;
  if (kp && kq) {
    if (!pair_resolved(dp, dq, e)) return 0.f;
    const float sa = sqrtf(dp + shift), sb = sqrtf(dq + shift);
    return kind == 0 ? -e / (sa * sb * (sa + sb)) : e / (sa + sb);
  }
  const float dk = kp ? dp : dq, dd = kp ? dq : dp;
  const float fk = kind == 0 ? 1.f / sqrtf(dk + shift) : sqrtf(dk + shift);
  // across the cut-off f jumps, and the first-order term e f_k / (d_k - d_d) is only the expansion of
  // (f_k - 0) sin(theta) cos(theta) for a small rotation angle theta ~ e / gap: it can never exceed f_k / 2.  A residual
  // that is not small against the gap (two eigenvalues within a per cent of 1e-5) is clamped to that bound
  return e * fk / fmaxf(dk - dd, 2.f * fabsf(e));
}

// The elementwise passes over a matrix in 64 x 64 TILES (round 4).  Written element by element (round 3) every
// output read two diagonal entries (a gather with stride C + 1: one cache line per thread) and the mirrored entry
// (a column walk), ~1.4 ms per 32-pair step for three kernels that move 100 MB each.  A block now parks the two
// diagonal segments of its tile and the MIRROR tile in LDS (rows loaded coalesced, read transposed), so every global
// access is a coalesced 16-byte row piece.  Per element the arithmetic is what it was, in the same order.
struct SpectralTile {
  float dp[64], dq[64];          // diagonal entries of the tile's rows / columns
  float mt[64][65];              // mirror tile: mt[c][r] = A[q0 + c][p0 + r]
};
// (`used`: spectral_open_all_kernel is the only caller left, and hipcc's link-time passes then specialise this function on that
// kernel's tile BEFORE they inline it -- measured: equivalent instructions, the two diagonal stores arranged differently, but
// not the kernel text that tools/kernel_isa_diff.py pins.  Kept whole, it is inlined as it always was; the price is an
// uncalled copy of it in the code object.)
__attribute__((used)) __device__ __forceinline__ void spectral_tile_load(SpectralTile& t, const float* Am, int C, int p0, int q0, int tid) {
  if (tid < 64) t.dp[tid] = p0 + tid < C ? Am[(size_t)(p0 + tid) * C + p0 + tid] : 0.f;
  else if (tid < 128) t.dq[tid - 64] = q0 + tid - 64 < C ? Am[(size_t)(q0 + tid - 64) * C + q0 + tid - 64] : 0.f;
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + ty * 4 + i, c = p0 + tx * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < C && c < C) v = *reinterpret_cast<const f32x4*>(Am + (size_t)r * C + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) t.mt[ty * 4 + i][tx * 4 + j] = v[j];
  }
}

// ---- round 5: the transform tail in MERGED launches.  Until round 4 every level ran the chain spectral_matrix -> prep2 ->
// products -> add2 -> V G -> (V G) V^T twice, content side then style side (13 launches), then T = Tcs Tw, a memset, the blend
// and the apply: 17 launches per level, most of them a few microseconds of work on half the matrices.  Here one launch of each
// kind covers all 2P matrices of the level (matrix m = 2 pair + side; kind = m & 1: 0 whitening, 1 colouring), the first-order
// matrix and the second-order operands come out of ONE pass over the tile, the blend rides on the epilogue of T = Tcs Tw
// (gemm_f32_kernel), and the pass that opens the chain also clears mabs and writes the bias vector: 8 launches per level.
// These two kernels hold the only copy of the per-element arithmetic: style-swap's three functions run through them too.
struct SpecAllArgs {
  const float* A;            // [2P][C][C] rotated covariances (diagonal = eigenvalues, off-diagonal = residual)
  float* G;                  // [2P][C][C]
  float *N, *R, *Pm;         // N [2P][C][C]; R, Pm [P][C][C] (whitening side only)
  const float *X1, *X2;      // add2: X1 [P][C][C], X2 [2P][C][C]
  int C; float shift; int correct, second; WctSkip skip;
  unsigned* mabs; const float* mean; float* bias; float alpha; int mode;     // per-pair housekeeping of the opening pass
};

// Second-order term of the same expansion (round 3):  (L2)_pq = sum_k f[d_p, d_k, d_q] E_pk E_kq  with the second divided
// differences of the spectral functions, which have closed forms without cancellation (sa = sqrt(a + shift) ...):
//   l^+1/2:  f[a,b,c] = -1 / ((sa+sb)(sb+sc)(sa+sc))
//   l^-1/2:  f[a,b,c] = (sa+sb+sc) / (sa sb sc (sa+sb)(sb+sc)(sa+sc))
// and both SEPARATE into matrix products of elementwise-scaled copies of E:  with N_pk = E_pk / (s_p + s_k),
// R_pk = E_pk / s_k, P_pk = N_pk / s_k,
//   l^+1/2:  L2 = -(N N) o 1/(s_p + s_q)
//   l^-1/2:  L2 = ( sym(R N) + (s_p + s_q)/2 (P N) ) o 1/(s_p s_q (s_p + s_q))      (P N = N diag(1/s) N is symmetric)
// (checked against an exact eigendecomposition in NumPy: the error of f(D + E) drops from ~r^2 to ~r^3).  Only the block
// of kept eigenvalues takes part: a dropped direction's couplings are bounded by sqrt(1e-5 d_p) tol and enter squared.
// It lets the sweeps stop one sweep earlier for the same transform error (profiles/r03_eig_calibration.txt).
// grid (C / 64, C / 64, 2P): tile rows p0 = 64 blockIdx.y, columns q0 = 64 blockIdx.x
__global__ __launch_bounds__(256) void spectral_open_all_kernel(SpecAllArgs a) {
  __shared__ SpectralTile t;
  const int m = blockIdx.z, p0 = blockIdx.y * 64, q0 = blockIdx.x * 64, tid = threadIdx.x;
  const int C = a.C, kind = m & 1, pair = m >> 1;
  const size_t cc = (size_t)C * C;
  if (kind == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    // what blend_matrix_kernel did besides the blend: bias = alpha ms (+ (1 - alpha) mc in tf mode); and mabs starts at 0
    if (tid == 0) a.mabs[pair] = 0u;
    const float* mp = a.mean + (size_t)(one_content(a.skip) ? 0 : pair) * 2 * C;     // (a mix: the one content)
    const float* ms = a.mean + (size_t)(one_style(a.skip) ? 0 : pair) * 2 * C + C;
    for (int i = tid; i < C; i += 256) {
      float b = a.alpha * ms[i];
      if (a.mode == WCT_MODE_TF) b += (1.f - a.alpha) * mp[i];
      a.bias[pair * C + i] = b;
    }
  }
  if (skip_style_mat(m, a.skip)) return;
  __shared__ float cutred[4];
  const float* Am = a.A + m * cc;
  const float cut = spectral_cut(Am, C, tid, cutred);
  spectral_tile_load(t, Am, C, p0, q0, tid);
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pl = ty * 4 + i, p = p0 + pl, q = q0 + tx * 4;
    if (p >= C || q >= C) continue;
    const f32x4 av = *reinterpret_cast<const f32x4*>(Am + (size_t)p * C + q);
    const float dp = t.dp[pl];
    f32x4 g, n4 = {0.f, 0.f, 0.f, 0.f}, r4 = n4, p4 = n4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dk = t.dq[tx * 4 + j];
      const float em = 0.5f * (av[j] + t.mt[tx * 4 + j][pl]);      // the two triangles agree to round-off; their mean keeps G symmetric
      g[j] = spectral_entry(dp, dk, a.correct ? em : 0.f, p == q + j, kind, a.shift, cut);
      if (a.second && p != q + j && dp > cut && dk > cut && pair_resolved(dp, dk, em)) {
        const float sp = sqrtf(dp + a.shift), sk = sqrtf(dk + a.shift);
        n4[j] = em / (sp + sk);
        r4[j] = em / sk;
        p4[j] = n4[j] / sk;
      }
    }
    const size_t o = (size_t)p * C + q;
    *reinterpret_cast<f32x4*>(a.G + m * cc + o) = g;
    if (a.second) {
      *reinterpret_cast<f32x4*>(a.N + m * cc + o) = n4;
      if (kind == 0) { *reinterpret_cast<f32x4*>(a.R + pair * cc + o) = r4; *reinterpret_cast<f32x4*>(a.Pm + pair * cc + o) = p4; }
    }
  }
}

__global__ __launch_bounds__(256) void spectral_add2_all_kernel(SpecAllArgs a) {
  __shared__ float dps[64], dqs[64];
  __shared__ float x1t[64][65], x2t[64][65];       // mirror tiles of X1 (kind 0 only), X2
  const int m = blockIdx.z, p0 = blockIdx.y * 64, q0 = blockIdx.x * 64, tid = threadIdx.x;
  if (skip_style_mat(m, a.skip)) return;
  const int C = a.C, kind = m & 1;
  const size_t cc = (size_t)C * C;
  const float* Am = a.A + m * cc;
  float* Gm = a.G + m * cc;
  const float* X2 = a.X2 + m * cc;
  const float* X1 = a.X1 + (size_t)(m >> 1) * cc;
  // a matrix with an eigenvalue within half a decade of the cut-off keeps the first-order completion and the old stop
  // threshold (jacobi_resid_kernel weighs its residual accordingly): around the cut-off sit the noise directions of
  // rank-deficient covariances, whose mutual couplings never become small, and a second-order sum over them is noise
  int near = 0;
  for (int i = tid; i < C; i += 256) {
    const float d = fabsf(Am[(size_t)i * C + i]);
    near |= (d > 3.3e-6f) & (d < 3e-5f);
  }
  if (__syncthreads_or(near)) return;
  __shared__ float cutred[4];
  const float cut = spectral_cut(Am, C, tid, cutred);
  if (tid < 64) dps[tid] = p0 + tid < C ? Am[(size_t)(p0 + tid) * C + p0 + tid] : 0.f;
  else if (tid < 128) dqs[tid - 64] = q0 + tid - 64 < C ? Am[(size_t)(q0 + tid - 64) * C + q0 + tid - 64] : 0.f;
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + ty * 4 + i, c = p0 + tx * 4;
    f32x4 v1 = {0.f, 0.f, 0.f, 0.f}, v2 = v1;
    if (r < C && c < C) {
      v2 = *reinterpret_cast<const f32x4*>(X2 + (size_t)r * C + c);
      if (kind == 0) v1 = *reinterpret_cast<const f32x4*>(X1 + (size_t)r * C + c);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { x2t[ty * 4 + i][tx * 4 + j] = v2[j]; x1t[ty * 4 + i][tx * 4 + j] = v1[j]; }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pl = ty * 4 + i, p = p0 + pl, q = q0 + tx * 4;
    if (p >= C || q >= C) continue;
    const size_t o = (size_t)p * C + q;
    const f32x4 x2 = *reinterpret_cast<const f32x4*>(X2 + o);
    f32x4 x1 = {0.f, 0.f, 0.f, 0.f};
    if (kind == 0) x1 = *reinterpret_cast<const f32x4*>(X1 + o);
    f32x4 g = *reinterpret_cast<const f32x4*>(Gm + o);
    const float dp = dps[pl];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dq = dqs[tx * 4 + j];
      if (!(dp > cut && dq > cut)) continue;
      const float sp = sqrtf(dp + a.shift), sq = sqrtf(dq + a.shift);
      float l2;
      if (kind == 1) l2 = -0.5f * (x2[j] + x2t[tx * 4 + j][pl]) / (sp + sq);
      else l2 = (0.5f * (x1[j] + x1t[tx * 4 + j][pl]) + 0.25f * (sp + sq) * (x2[j] + x2t[tx * 4 + j][pl])) / (sp * sq * (sp + sq));
      g[j] += l2;
    }
    *reinterpret_cast<f32x4*>(Gm + o) = g;
  }
}

// what the C x C products over the matrices of a level have in common; the operands, their layouts and the output are the caller's
static GemmArgs level_product(int C, WctSkip skip) {
  GemmArgs g = {};
  g.lda = g.ldb = g.ldo = C; g.M = g.N = g.K = g.ksplit = C; g.sA = g.sB = g.s_out = (size_t)C * C; g.skip = skip;
  return g;
}

// refresh (see refresh_needed): X = A0 V, then A <- V^T X, for the matrices whose kept spectrum reaches 4 decades below their
// norm; the others' blocks exit at once.  Before ANY spectral function of the tracked (A, V): launch_wct's apply stage and the
// three of launch_style_swap (relu5_1, C = 512: every input of 352 x 352 or smaller has N < C -- the rank-deficient case).
// Refreshing EVERY matrix, whatever its spectrum, was measured for style-swap when the solver's tile update moved to split fp16:
// the 3 of 900 patch matches that flipped on the 32 x 32 test case flipped with the rotated matrix recomputed as well -- it is V,
// not the tracked matrix, that carries the difference.
static int launch_refresh(const WctCarve& w, int C, int P, WctSkip skip, hipStream_t s) {
  int rc;
  GemmArgs r1 = level_product(C, skip);
  r1.A = w.A0; r1.a_kmajor = 0; r1.B = w.V; r1.b_kmajor = 1; r1.out32 = w.X;
  r1.mask_diag = w.A; r1.s_mask = (size_t)C * C; r1.mask_out = w.refresh;
  if ((rc = launch_gemm(r1, 1, 2 * P, s))) return rc;
  GemmArgs r2 = level_product(C, skip);
  r2.A = w.V; r2.a_kmajor = 1; r2.B = w.X; r2.b_kmajor = 1; r2.out32 = w.A; r2.mask_in = w.refresh;
  return launch_gemm(r2, 1, 2 * P, s);
}

// The spectral tail of a level, all 2P matrices in merged launches: Tw / Tcs [m] = V f(A) V^T (whitening for the even matrices,
// colouring for the odd ones), plus the bias vectors and cleared mabs words of the opening pass.  nwhite: the pairs whose
// whitening side is live (P; 1 for a style mix, whose content is matrix 0 alone).  This is the tail behind its refresh: on
// its own for a second run over matrices that have had theirs (style-swap's style whitening).
int launch_spectral_tail_refreshed(const WctCarve& w, int C, int P, float alpha, int mode, float eps_in, WctSkip skip, int nwhite,
                                   hipStream_t s) {
  int rc;
  const size_t cc = (size_t)C * C;
  // Tw = Vc f_c(Ac) Vc^T, Tcs = Vs f_s(As) Vs^T with the first- and second-order completion of f on the residual
  // off-diagonals; the wct_np semantics shift the kept eigenvalues by eps inside the gains (ops.py:114,127), wct_tf does not.
  // One launch of each kind over all 2P matrices of the level (see spectral_open_all_kernel).
  const float shift = mode == WCT_MODE_NP ? (eps_in >= 0.f ? eps_in : 1e-5f) : 0.f;
  const int second = EIG_CORRECT >= 2;
  const dim3 tiles(cdiv(C, 64), cdiv(C, 64), 2 * P);
  SpecAllArgs sa = {};
  sa.A = w.A; sa.G = w.G; sa.C = C; sa.shift = shift; sa.correct = EIG_CORRECT; sa.second = second; sa.skip = skip;
  sa.N = w.S2; float* X2 = sa.N + 2 * P * cc; sa.R = X2 + 2 * P * cc; sa.Pm = sa.R + P * cc; float* X1 = sa.Pm + P * cc;
  sa.X1 = X1; sa.X2 = X2;
  sa.mabs = w.mabs; sa.mean = w.mean; sa.bias = w.bias; sa.alpha = alpha; sa.mode = mode;
  hipLaunchKernelGGL(spectral_open_all_kernel, tiles, dim3(256), 0, s, sa);
  HIP_TRY(hipGetLastError());
  if (second) {
    GemmArgs a = level_product(C, skip);   // X2[m] = (colouring: N[m], whitening: Pm[pair]) . N[m]
    a.A = sa.Pm; a.A_odd = sa.N + cc; a.sA_odd = 2 * cc; a.a_kmajor = 0; a.B = sa.N; a.b_kmajor = 1; a.out32 = X2;
    if ((rc = launch_gemm(a, 1, 2 * P, s))) return rc;
    GemmArgs b = level_product(C, WCT_SKIP_NONE);   // X1[pair] = R[pair] . N[2 pair]   (whitening side only)
    b.A = sa.R; b.a_kmajor = 0; b.B = sa.N; b.b_kmajor = 1; b.sB = 2 * cc; b.out32 = X1;
    if (nwhite > 0 && (rc = launch_gemm(b, 1, nwhite, s))) return rc;
    hipLaunchKernelGGL(spectral_add2_all_kernel, tiles, dim3(256), 0, s, sa);
    HIP_TRY(hipGetLastError());
  }
  GemmArgs g = level_product(C, skip);   // X[m] = V[m] G[m]
  g.A = w.V; g.a_kmajor = 0; g.B = w.G; g.b_kmajor = 1; g.out32 = w.X;
  if ((rc = launch_gemm(g, 1, 2 * P, s))) return rc;
  GemmArgs h = level_product(C, skip);   // Tw / Tcs [m] = X[m] V[m]^T
  h.A = w.X; h.a_kmajor = 0; h.B = w.V; h.b_kmajor = 0; h.out32 = w.Tw;
  return launch_gemm(h, 1, 2 * P, s);
}

int launch_spectral_tail(const WctCarve& w, int C, int P, float alpha, int mode, float eps_in, WctSkip skip, int nwhite,
                         hipStream_t s) {
  const int rc = launch_refresh(w, C, P, skip, s);
  return rc ? rc : launch_spectral_tail_refreshed(w, C, P, alpha, mode, eps_in, skip, nwhite, s);
}
