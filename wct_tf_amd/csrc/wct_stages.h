// What the translation units of the whiten-colour transform share among themselves -- stats_gemm.hip (K3, the GEMM, K4),
// eigh.hip (K5), spectral.hip (K6), wct.hip (K7, the carve, the plans, the transforms), mask.hip, style_swap.hip.  Private to
// those units: the api_*.hip units see common.h alone.  Every kernel lives in ONE unit, behind the launcher declared here.
#pragma once
#include "common.h"

// (the matrices of a batch, and the skip mode that says which of them are dead: skip_rule.h, through common.h)

// 0: spectral functions of the diagonal only, 1: + first-order completion, 2 (the product): + second-order completion
constexpr int EIG_CORRECT = 2;
// residual at which the WCT path stops sweeping.  Calibrated on the level features of a 512x512 frame
// (profiles/r02_eig_calibration.txt): with r2 the strict measure at the stop, the transform error is ~0.55 sqrt(r2)
// without the first-order completion and ~0.8 r2 (+ ~3e-5 from the other stages) with it, so 1.5e-2 bounds the
// completed transform's error by ~1.8e-4 -- five times inside the 1e-3 budget.  0 without the completion.
constexpr float JACOBI_TOL_FN = 1.5e-2f;
constexpr float JACOBI_TOL_FN2 = 4e-2f;            // with the second-order completion (profiles/r03_eig_calibration.txt: the transform error
                                                   // at 4e-2 with it, 3.1e-5 .. 1.3e-4, is what 1.5e-2 gave without it, one sweep later)
constexpr float JACOBI_TOL_FN_WCT = EIG_CORRECT >= 2 ? JACOBI_TOL_FN2 : (EIG_CORRECT ? JACOBI_TOL_FN : 0.f);   // the one in use

// ---- workspace carving (P independent content/style pairs per call; wct.hip) ----------------------------------------------
static inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct WctCarve {
  float *mean, *var, *stat_partial, *absmax, *scale, *cov_partial, *A, *A0, *V, *d, *G, *X, *S2, *Tw, *Tcs, *T, *M, *bias, *mix;
  unsigned* mabs; int* refresh;
  void* jacobi_ws; size_t jacobi_bytes;
  int nslab, nsplit, ksplit;
  size_t total;
};

// the slab count and K-slices of ONE (content, style) pair of Nc and Ns rows: independent of P, as a pair's result must not
// depend on its batch
struct PairLayout { int nslab, nsplit, ksplit; };
PairLayout pair_layout(int C, int Nc, int Ns);
// P pairs whose per-matrix partial buffers hold lay.nslab slabs / lay.nsplit K-slices
WctCarve carve(void* base, int C, int P, const PairLayout& lay);

// eps_in < 0 selects the reference defaults: 1e-8 on the covariance diagonal for wct_tf (ops.py:24,45,50); wct_np adds none
// there (its 1e-5 sits inside the spectral gains, ops.py:92,114,127 -- launch_spectral_tail)
static inline float cov_eps(int mode, float eps_in) {
  return mode == WCT_MODE_TF ? (eps_in >= 0.f ? eps_in : 1e-8f) : 0.f;
}

// blocks of a grid-stride pass over N rows of C channels, 4 channels a thread (the AdaIN applies, the mask gather)
static inline unsigned rows_grid(size_t N, int C) {
  const size_t blocks = (N * C / 4 + 255) / 256;
  return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

// The slot plan of a per-slot transform (a style mix, spatial control): 2P matrix slots in the pair layout of carve(), each
// slot's statistics and covariance launched on its own rows with the layout of its own single-pair transform (pair_layout).
// A mix or a masked frame has at most WCT_MIX_MAX pairs; the (frame, region) pairs of a masked batch fill one batched
// eigensolve of 64 matrices: WCT_PLAN_PAIRS.
constexpr int WCT_PLAN_PAIRS = 32;
struct SlotPlan {
  int P; WctSkip skip; int nwhite;             // pairs; the skip mode; pairs whose whitening side is live
  struct Slot { const float* x; int n; PairLayout lay; } slot[2 * WCT_PLAN_PAIRS];   // rows (null while only sizing the
                                                                                    // workspace), their count (0: skipped), layout
  const float* u0; const unsigned* umax0;      // slot 0's unit sums from a conv epilogue, or null
  WctCarve w;
  size_t total;
};
void plan_carve(SlotPlan* sp, void* base, int C);    // the workspace of a plan (wct.hip)
bool plan_fits(const SlotPlan& sp, int C);           // every slot within the covariance kernel's 32-bit byte offsets

// ---- K7 apply (wct.hip) ------------------------------------------------------------------------------------------------------
struct ApplyArgs {
  const float* x; int N; int C;     // content features [P][N][C]
  const float* mean;                // [2P][C]: content mean of pair p at 2p
  const float* M; const float* bias;  // [P][C][C], [P][C]
  const float* xscale;              // [2P]: content scale of pair p at 2p
  const unsigned* mabs;             // [P] max |M| (float bits)
  half_t* out16; float* out32;      // [P][N][C], either may be null
};
// A masked transform (launch_wct_masked): pair p is the segment of label lab[p] -- rows [seg_off[lab], seg_off[lab + 1]) of the
// label-compacted content x -- and its row r is stored to row perm[r] of out16 / out32 (the scatter back to pixel order)
struct ApplySegArgs : ApplyArgs { const int* seg_off; const int* perm; int lab[WCT_MIX_MAX]; };
// The segments of a masked BATCH (launch_wct_masked_batch): x, out16 / out32 hold G frames of N rows, seg_off [G][WCT_MIX_MAX + 1]
// and perm [G][N] are per frame, and pair p is the segment of label fl[p] & 7 of frame fl[p] >> 3
struct ApplySegBatchArgs : ApplyArgs { const int* seg_off; const int* perm; unsigned char fl[WCT_PLAN_PAIRS]; };
// A strength map (launch_wct with a WctStrength): M, bias and mabs are the alpha = 1 call's, and row r of pair p
// leaves as strength_rule.h blends it with x -- a = alpha * smap[p][pixel of r] / 255 (the map addressing of WctStrength)
struct ApplyMapArgs : ApplyArgs { const uint8_t* smap; int Hm, Wm, w, stride; float alpha; };
// the ApplyArgs part of any of the four: x [N rows a pair, or a masked transform's gathered rows] against the matrices of w
template <typename Args>
static inline Args apply_args(const WctCarve& w, const float* x, int N, int C, half_t* out16, float* out32) {
  Args a;
  a.x = x; a.N = N; a.C = C; a.mean = w.mean; a.M = w.M; a.bias = w.bias;
  a.xscale = w.scale; a.mabs = w.mabs; a.out16 = out16; a.out32 = out32;
  return a;
}
__device__ __host__ __forceinline__ int seg_frame(unsigned char fl) { return fl >> 3; }
__device__ __host__ __forceinline__ int seg_label(unsigned char fl) { return fl & 7; }

// ---- stage launchers, by the unit that holds their kernels -----------------------------------------------------------------
// stats_gemm.hip: means and the fp16 scale (with_var: the variances) of the 2P matrices; their covariances into w.A and w.A0
// (eps on the diagonal); both for the live slots of a plan, each with its own layout
int launch_means(const float* content, int Nc, const float* style, int Ns, int C, int P, const WctCarve& w, bool with_var,
                 WctSkip skip, hipStream_t s, const WctFeatStats* fs);
int launch_cov(const float* content, int Nc, const float* style, int Ns, int C, int P, const WctCarve& w, float eps, WctSkip skip,
               hipStream_t s);
int launch_plan_stats(const SlotPlan& sp, int C, bool with_var, bool with_cov, float eps, hipStream_t s);
// launch_cov at relu1_1 (C = 64), the rows of both sides computed from their images; w laid out for the sides' H * W rows
int launch_cov_image(const WctImageSrc& src, int P, const WctCarve& w, float eps, WctSkip skip, hipStream_t s);
// eigh.hip: the 2P matrices of w in one batched solve
// (check_from: the first sweep after which the host looks at the done-flags -- JacobiGroup::check_from; a warm solve passes 0)
int launch_eig_stage(const WctCarve& w, int C, int P, WctSkip skip, int u_f16, int* sweeps_dev, int* eig_fail, hipStream_t s,
                     int check_from = 2);
// spectral.hip: the merged spectral tail of a level, which begins with the refresh of the rotated matrices; the tail alone, for
// matrices that have had their refresh (style-swap's second run)
int launch_spectral_tail(const WctCarve& w, int C, int P, float alpha, int mode, float eps_in, WctSkip skip, int nwhite, hipStream_t s);
int launch_spectral_tail_refreshed(const WctCarve& w, int C, int P, float alpha, int mode, float eps_in, WctSkip skip, int nwhite,
                                   hipStream_t s);
// wct.hip: the blend product M = alpha Tcs Tw + (1 - alpha) I of P pairs; the apply of P pairs of Nc rows on the matrices of w
// (any number of calls on one set of matrices: the chunks of a banded map); the apply of a masked transform's P segments (the
// longest has nmax rows), whose argument blocks start from apply_args
int launch_blend(const WctCarve& w, int C, int P, float alpha, WctSkip skip, hipStream_t s);
int launch_apply(const WctCarve& w, const float* content, int Nc, int C, int P, half_t* out16, float* out32, hipStream_t s);
template <typename Args> int launch_apply_args(const Args& a, int nmax, int P, hipStream_t s);   // (ApplySegArgs, ApplySegBatchArgs, ApplyMapArgs)
// warm.hip (video warm start): A' = V0^T A V0 of the P content matrices of w in place (w.X scratch); V = V0 V' of the same in place
// (w.X scratch); basis = V (3 I - V^T V) / 2 of one C x C matrix (scratch: C x C floats)
int launch_warm_rotate(const WctCarve& w, int C, int P, const float* V0, hipStream_t s);
int launch_warm_compose(const WctCarve& w, int C, int P, const float* V0, hipStream_t s);
int launch_warm_store(const float* V, float* scratch, float* basis, int C, hipStream_t s);
// wct.hip: state p of `r` into the style slot 2p + 1 of w (mean, var and, with_T, the colouring matrix), P <= WCT_PLAN_PAIRS
int launch_style_load_slots(const WctStyleSlots& r, int P, const WctCarve& w, int C, bool with_T, hipStream_t s);
