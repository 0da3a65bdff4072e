// What the pieces of the batched block-Jacobi eigensolver (K5) share: the solver's state words, the pairing schedule, the
// rotation family, the argument block of the look-ahead launches and the fragment order of the rotation logs.  The pair
// problems themselves live in jacobi_pair32.h (32-wide block pairs, {S, Q} image in LDS) and jacobi_pair64.h (64-wide, resident
// in registers); the kernels and the host driver in eigh.hip.  Device code only: nothing here touches the HIP runtime API.  The
// includer provides the vector typedefs of common.h (the CPU lane emulation brings its own prelude, tests/emul/hip_emul.h).
#pragma once

struct JacobiState {
  unsigned int offmax;   // max |a_pq|/sqrt(a_pp a_qq) over the pairs rotated this sweep (float bits)
  int done;              // 0 rotating, 1 converged, 2 failed: non-finite input
  int sweeps;
  unsigned int offsig;   // the same maximum over the SIGNIFICANT pairs only (a diagonal above `floor`)
  float floor;           // 1e-4 max|a_ii| of the previous sweep (-> 1e-4 lambda_max): diagonals below it are taken to belong
                         // to the numerical null space of a matrix of this norm (~1700 eps ||A||) when the STATUS is judged
  unsigned int last_sig; // offsig of the last completed sweep (what jacobi_finalize_kernel judges)
  unsigned int dmax;     // max |a_ii| seen by this sweep's pair problems (float bits)
  float r2;              // strict residual measure of the last completed sweep (jacobi_resid_kernel), -1 before the first
  float r2l;             // the lenient one (what the final status is judged by)
  int pad;               // the buffer (0: A, 1: the second one) that held the matrix when it was declared done
  int seg_stop;          // number of launch segments whose rotations belong to this matrix (INT_MAX while it is still rotating)
  int pad2;              // 1: a diagonal within half a decade of the 1e-5 cut-off at the last residual measurement (first-order completion only)
};
constexpr float JACOBI_SIG_FLOOR = 1e-4f;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- pairing schedule: column blocks of B = M2 / 2 are paired round-robin, C / B - 1 cross steps and one intra step a sweep
__device__ __forceinline__ int rr_idx(int pos, int step, int n) {
  // circle method: position 0 is fixed, the other n-1 rotate
  if (pos == 0) return 0;
  int v = pos - 1 + step;
  if (v >= n - 1) v -= n - 1;
  return v + 1;
}

// blocks (bi, bj) of pair g at outer step `step`; step < 0 is the intra step: neighbours (2g, 2g+1)
__device__ __forceinline__ void block_pair(int g, int step, int nblk, int& bi, int& bj) {
  if (step < 0) { bi = 2 * g; bj = 2 * g + 1; }
  else { bi = rr_idx(g, step, nblk); bj = rr_idx(nblk - 1 - g, step, nblk); }
}

// inverse of block_pair: pair index and half (0: first block, 1: second) of block b at outer step `step`
__device__ __forceinline__ void block_locate(int b, int step, int nblk, int& g, int& half) {
  if (step < 0) { g = b >> 1; half = b & 1; return; }
  int pos = 0;
  if (b != 0) {
    int v = b - 1 - step;                       // step <= nblk - 2: one wrap is enough
    if (v < 0) v += nblk - 1;
    pos = v + 1;
  }
  const int npair = nblk >> 1;
  if (pos < npair) { g = pos; half = 0; } else { g = nblk - 1 - pos; half = 1; }
}

// row / column r of the pair problem (bi, bj) in the matrix (B = 16 and 32)
template <int B>
__device__ __forceinline__ int pair_index(int r, int bi, int bj) {
  return r < B ? bi * B + r : bj * B + (r - B);
}

// ---- rotation family
constexpr float JACOBI_ROT_TOL = 1e-6f;    // skip rotations below this relative size
constexpr float JACOBI_CONV_TOL = 1e-2f;   // a sweep that never saw more than this is the last one (quadratic convergence;
                                           // measured: WCT error vs the oracle identical for 2e-3 and 1e-2, 100x worse at 5e-2)
constexpr float JACOBI_FLOOR = 1e-6f;      // both diagonals below this: the pair cannot reach the 1e-5 cut-off

// The one formula: t = tan(theta) of the rotation that annihilates a_pq, and whether the pair is rotated at all (the return
// value `rot`; t comes back as computed either way, the callers select on `rot`).
// t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), zeta = (a_qq - a_pp) / (2 a_pq), written as
// t = +-|a_pq| / (|tau| + sqrt(tau^2 + a_pq^2)), tau = (a_qq - a_pp)/2: two transcendentals on the dependent chain (sqrt, rcp)
// and no division by a_pq.  Not rotated:
//   (a) both diagonals far below the 1e-5 cut-off: whatever they mix stays dropped;
//   (b) coupling of a kept direction into a noise-level one with a negligible angle;
//   (c) a_pq below JACOBI_ROT_TOL of sqrt(a_pp a_qq).
// Bitwise & on the predicates: && would become an exec-mask branch around the second half.
__device__ __forceinline__ bool jacobi_tangent(float app, float aqq, float apq, float& t) {
  const float den2 = fabsf(app * aqq);
  const float aapq = fabsf(apq);
  const float big = fmaxf(fabsf(app), fabsf(aqq)), small = fminf(fabsf(app), fabsf(aqq));
  const bool live = (fabsf(app) + fabsf(aqq) > JACOBI_FLOOR) & !((small < JACOBI_FLOOR) & (aapq < 1e-6f * big));
  const bool rot = live & (aapq * aapq > JACOBI_ROT_TOL * JACOBI_ROT_TOL * den2) & (aapq > 1e-36f);
  const float tau = 0.5f * (aqq - app);
  const float h = __builtin_amdgcn_sqrtf(tau * tau + apq * apq);
  t = aapq * __builtin_amdgcn_rcpf(rot ? fabsf(tau) + h : 1.f);
  t = (tau >= 0.f) == (apq >= 0.f) ? t : -t;
  return rot;
}
// Only tan(theta), 0 for a pair that is not rotated -- what the chain of a rotation set of the register-resident pair problems
// waits for (pair64::strip_sets).  (c, s) follow from it (jacobi_cs_from_t) and feed nothing but the pivot lane's own closed-form
// diagonals of the NEXT set, so they are derived after the barrier, under the latency of that set's first LDS reads.
__device__ __forceinline__ bool jacobi_rotation_t(float app, float aqq, float apq, float& tt) {
  float t;
  const bool rot = jacobi_tangent(app, aqq, apq, t);
  tt = rot ? t : 0.f;
  return rot;
}
__device__ __forceinline__ void jacobi_cs_from_t(float tt, float& c, float& s) {
  const float n2 = 1.f + tt * tt;
  float r = __builtin_amdgcn_rsqf(n2);
  r = r * (1.5f - 0.5f * n2 * r * r);            // one Newton step: c^2 + s^2 = 1 to fp32 round-off
  c = tt != 0.f ? r : 1.f;                       // (no rotation: exactly the identity)
  s = r * tt;
}
// (c, s) alone, the identity for a pair that is not rotated: the part of a rotation that is on the serial chain of a set in the
// pivot wave of pair32::cross_sets (it gates every other wave at the barrier).  The convergence statistics are not on the chain:
// jacobi_rotation_stats evaluates them after (c, s) has been published, under the latency of that LDS write.
__device__ __forceinline__ bool jacobi_rotation_cs(float app, float aqq, float apq, float& c, float& s) {
  float t;
  const bool rot = jacobi_tangent(app, aqq, apq, t);
  const float n2 = 1.f + t * t;
  float r = __builtin_amdgcn_rsqf(n2);
  r = r * (1.5f - 0.5f * n2 * r * r);            // one Newton step: c^2 + s^2 = 1 to fp32 round-off
  c = rot ? r : 1.f;
  s = rot ? r * t : 0.f;
  return rot;
}
// `off` = pre-rotation relative size |a_pq| / sqrt(a_pp a_qq) (0 if the pair was not rotated).
// `sig` = the same measure if the pair is significant, else 0: pairs inside the numerical null space keep relative
// off-diagonals of O(1) for ever (every update regenerates rounding noise there) without mattering for f(A); they are still
// rotated, but they do not count as "not converged".  Both diagonals above the matrix' noise floor: the cosine; one above, the
// other inside the rounding noise (a cosine against it cannot settle): the rotation angle a_pq / big, and -- if the small one
// is below the reference's 1e-5 cut-off -- that it stays there: contamination a_pq^2 / big below 1 % of the cut-off; none
// above: does not count.  Branch-free (selects, not exec-mask branches: the pivot wave is the pole of every set).
__device__ __forceinline__ void jacobi_rotation_stats(float app, float aqq, float apq, float floor_m, bool rot, float& off, float& sig) {
  const float den2 = fabsf(app * aqq);
  const float aapq = fabsf(apq);
  const float big = fmaxf(fabsf(app), fabsf(aqq)), small = fminf(fabsf(app), fabsf(aqq));
  const float rel = den2 > 0.f ? fminf(aapq * __builtin_amdgcn_rsqf(den2), 1.f) : 1.f;
  off = rot ? rel : 0.f;
  const float mixed = fmaxf(aapq * __builtin_amdgcn_rcpf(big), small < 1e-5f ? 0.1f * aapq * __builtin_amdgcn_rsqf(big * 1e-5f) : 0.f);
  const float sig_mixed = big > floor_m ? fminf(off, mixed) : 0.f;
  sig = small > floor_m ? off : sig_mixed;
}
// Rotation and statistics in one, for the rotations that are on no chain.  (Written out on jacobi_tangent, not as
// jacobi_rotation_cs + jacobi_rotation_stats: that is the same arithmetic and other instructions in both fused kernels --
// profiles/eigh_widths_isa.txt.)
__device__ __forceinline__ void jacobi_rotation(float app, float aqq, float apq, float floor_m, float& c, float& s, float& off, float& sig) {
  float t;
  const bool rot = jacobi_tangent(app, aqq, apq, t);
  const float den2 = fabsf(app * aqq);
  const float aapq = fabsf(apq);
  const float big = fmaxf(fabsf(app), fabsf(aqq)), small = fminf(fabsf(app), fabsf(aqq));
  const float rel = den2 > 0.f ? fminf(aapq * __builtin_amdgcn_rsqf(den2), 1.f) : 1.f;
  const float n2 = 1.f + t * t;
  float r = __builtin_amdgcn_rsqf(n2);
  r = r * (1.5f - 0.5f * n2 * r * r);            // one Newton step: c^2 + s^2 = 1 to fp32 round-off
  c = rot ? r : 1.f;
  s = rot ? r * t : 0.f;
  off = rot ? rel : 0.f;
  const float mixed = fmaxf(aapq * __builtin_amdgcn_rcpf(big), small < 1e-5f ? 0.1f * aapq * __builtin_amdgcn_rsqf(big * 1e-5f) : 0.f);
  sig = small > floor_m ? off : (big > floor_m ? fminf(off, mixed) : 0.f);
}

// ---- argument block of a look-ahead launch { D(step_d), U(step_u) } (eigh.hip: jacobi_fused_launch)
struct JacobiFusedArgs {
  const float* Pr;      // [nmat][C][C] state the U part reads and the D part takes its look-ahead block from
  float* Pw;            // [nmat][C][C] state the U part writes
  float* V;             // [nmat][C][C] eigenvector accumulation, in place
  const float* Qr; const float* Sr;   // [nmat][npair][M2*M2] rotations / rotated pair problems of step_u
  float* Qw; float* Sw;               // ... written by the D part (step_d)
  const half_t* Qr16; half_t* Qw16;   // the same rotations split into fp16 hi + lo MFMA fragments (V <- V Q; see qfrag16_k)
  int u_f16 = 0;                      // tile update of the 64-wide block pairs on split fp16 (pair64::fused_u) instead of fp32 MFMA
  JacobiState* st;
  int C, nmat;
  int step_d, step_u;   // outer step of the pair problems / of the tile update (= the step before step_d)
  int has_d, has_u;
  int first;            // the D part loads its pair problems straight from Pr (nothing is pending on it)
  int with_v;           // the U part also updates V (otherwise jacobi_vstrip_kernel applies the segment's rotations later)
};

// ---- fragment order of the rotation logs
// Rotation matrices are stored in FRAGMENT order (the A operand of v_mfma_f32_16x16x4_f32): float4 f = (mt * (M2/16) + t) * 64
// + lane holds Q[16 t + 4 (lane >> 4) + r][16 mt + (lane & 15)], r = 0..3.  Every consumer stages whole tiles, so the order
// costs the others nothing.
template <int M2>
__device__ __forceinline__ void qfrag_rc(int f, int& row, int& col) {
  constexpr int NTL = M2 / 16;
  const int l = f & 63, t = (f >> 6) % NTL, mt = (f >> 6) / NTL;
  row = 16 * t + 4 * (l >> 4); col = 16 * mt + (l & 15);
}

// V <- V Q runs on the fp16 MFMA pipe with split operands (hi = fp16(x), lo = fp16(x - hi): 22 significand bits; hi*hi +
// hi*lo + lo*hi accumulated in fp32 -- the covariance kernel's scheme): the entries of V and Q are bounded by 1, and three
// v_mfma_f32_16x16x32_f16 replace eight v_mfma_f32_16x16x4_f32 at a sixteenth of their cost each.  The rotation matrices
// are therefore ALSO stored as fp16 fragments: unit u = ((mt * NCH + c) * 2 + part) * 64 + lane (16 bytes = 8 halfs;
// part 0 = hi, 1 = lo; NCH = M2 / 32 K-chunks) holds the A operand of output tile mt and chunk c for lane (m, g) = (lane
// & 15, lane >> 4): element j is Q[k][16 mt + m] with k = qfrag16_k(c, g, j).  That k-slot order is what makes the accumulator
// layout of a 16 x 16 tile of V^T (lane (n, g), register r <-> V[n][4 g + r]) the B operand of the next product without any
// data movement: elements 0..3 come from tile 2c, 4..7 from tile 2c + 1.
// (M2 = 32 and 64, the caller's pair width: the value does not depend on it, hipcc's code for the 32-wide epilogue does --
//  profiles/eigh_widths_isa.txt)
template <int M2>
__device__ __forceinline__ int qfrag16_k(int c, int g, int j) { return 16 * (2 * c + (j >> 2)) + 4 * g + (j & 3); }

__device__ __forceinline__ void split_f16x8(const float (&x)[8], half8& hi, half8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hi[j] = (half_t)x[j];
    lo[j] = (half_t)(x[j] - (float)hi[j]);
  }
}
