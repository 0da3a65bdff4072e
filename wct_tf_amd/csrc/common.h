// Shared declarations for libwct_hip.so (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "skip_rule.h"

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define WCT_OK 0
#define WCT_ERR_HIP -1
#define WCT_ERR_ARG -2
#define WCT_ERR_STATE -3
#define WCT_ERR_NOMEM -4
#define WCT_ERR_NOCONV -5

void wct_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      wct_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                    __FILE__, __LINE__);                                       \
      return WCT_ERR_HIP;                                                      \
    }                                                                          \
  } while (0)

#define ARG_CHECK(cond)                                                        \
  do {                                                                         \
    if (!(cond)) {                                                             \
      wct_set_error("invalid argument: %s (%s:%d)", #cond, __FILE__, __LINE__);\
      return WCT_ERR_ARG;                                                      \
    }                                                                          \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// The conv kernels address one image's activations, and the transform one feature map, with 32-bit byte offsets: a map of `elems`
// elements of `bytes` each fits one launch below 2^31 bytes.  The one bound behind the size check of every launcher and behind
// the routing of the banded path (banded.hip), which cuts what does not fit into pieces that do.
constexpr size_t WCT_LAUNCH_BYTES = (size_t)1 << 31;
static inline bool launch_map_fits(size_t elems, size_t bytes) { return elems * bytes < WCT_LAUNCH_BYTES; }

// Environment variables: the library reads five TEST hooks and nothing else, all safe by construction (a library whose
// contract is bit-reproducible output must not change its numerics on a stray variable): WCT_JACOBI_MAX_SWEEPS can only
// LOWER the sweep budget (clamped to the compiled one; the solve then fails loudly, never silently); WCT_FUSE_STATS=0,
// WCT_FUSE_CONV1=0 and WCT_L1_FROM_IMAGE=0 each select a path whose output is bit-identical (asserted by
// tests/test_gpu_pipeline.py and tests/test_gpu_level1_image.py); WCT_WINOGRAD=0
// keeps every 3x3 layer on the direct kernel (the round-5 arithmetic: other roundings, same tolerances).  The A-B switches of
// the tuning rounds and the variants they selected were removed after round 6.

// ---- conv.hip -------------------------------------------------------------
struct ConvArgs {
  const half_t* x;     // [B][Hin][Win][Cin] fp16 NHWC
  const half_t* w;     // [Cout][9][Cin] fp16 (tap-major, K contiguous)
  const float* bias;   // [Cout]
  half_t* y16;         // [B][H][W][Cout] fp16 or nullptr
  float* y32;          // [B][H][W][Cout] fp32 or nullptr
  int B, H, W;         // output size (== input size, or 2x input if upsample)
  int Cin, Cout;
  int upsample;        // input is the x2 nearest upsample of x (model.py:293)
  int relu;
  int pool;            // fuse the following 2x2/2 'same' max-pool: outputs are [(H+1)/2][(W+1)/2][Cout]
  // feature statistics from the fp32 epilogue (null: off; need y32, relu, W % 16 == 0): usum [B][H*W/16][Cout] = the sum of
  // every run of 16 consecutive pixels (unit_row_sum's fixed tree -- what colsum_kernel computes from the stored features),
  // umax [B][UMAX_SLOTS] = bit patterns whose maximum is the largest value of the image (>= 0 after the ReLU), merged with
  // atomicMax: zero it before the launch
  float* usum;
  unsigned* umax;
  // conv1_1 fused into the patch loader (conv1_2 of an encoder pass whose relu1_1 nobody else reads; Cin = Cout = 64): the
  // block computes its halo patch of relu1_1 activations from the IMAGE instead of reading them -- x is unused, img1 is the
  // [B][H][W][3] fp32 image and (w1frag, bias1, clamp01) are conv1_1's ConvFirstArgs.  null img1: off.
  const float* img1 = nullptr;
  const half_t* w1frag = nullptr;
  const float* bias1 = nullptr;
  int clamp01 = 0;
  // the layer's filters transformed for the reduced-FLOP kernel (conv_wino.hip): fp16 MFMA A-fragments
  // [Cout/32][f*3+kx][Cin/16][lane][8] of U_f[kx] = sum_ky G[f][ky] g[ky][kx].  null: the direct kernel only.
  const half_t* w_wino = nullptr;
};
// The maxima of an image are merged into UMAX_SLOTS words (two cache lines) instead of one: tens of thousands of
// wavefronts bumping ONE word -- or 32 words of one cache line -- serialise in a single L2 channel (measured: +94 us per
// launch); a wave also reads its slot first and skips the atomic when it cannot raise it (values only grow).
constexpr int UMAX_SLOTS = 64;
__device__ __forceinline__ void umax_merge(unsigned* umax_img, int slot, float vmax, int lane) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
  if (lane == 0) {
    unsigned* w = umax_img + (slot & (UMAX_SLOTS - 1));
    const unsigned bits = __builtin_bit_cast(unsigned, vmax);
    if (bits > __atomic_load_n(w, __ATOMIC_RELAXED)) atomicMax(w, bits);
  }
}
int launch_conv3x3(const ConvArgs& a, hipStream_t s);
// conv_wino.hip: Winograd F(2,3) along y x direct along x -- 12 MFMA products per 2 outputs instead of 18 (fp16 output only)
bool conv3x3_wino_takes(const ConvArgs& a);
int launch_conv3x3_wino(const ConvArgs& a, hipStream_t s);

struct ConvFirstArgs {   // 3 -> 64 with the 1x1 'preprocess' folded in
  const float* x;      // [B][H][W][3] fp32 image in [0,1]
  const half_t* wfrag; // folded weights as fp16 hi/lo MFMA A-fragments [cout/32][k-step 2][hi,lo][lane][8], k = tap*3+cin (27 -> 32)
  const float* bias;   // [64]
  half_t* y16;
  float* y32;
  int B, H, W;
  int clamp01;         // clip(x,0,1) at load (model.py:86)
  float* usum;         // as in ConvArgs (W % 16 == 0), of the fp32 values whether y32 stores them or not; y16 and y32 both
  unsigned* umax;      // null: the statistics alone (conv_first_kernel<false>)
};

// Sums over the 16 lanes of a DPP row (= the 16 pixels of one row of an MFMA pixel tile), the same bits in every
// lane: ((p0+p1)+(p2+p3) + (p4+p5)+(p6+p7)) + (the same of p8..p15).  colsum_kernel adds 16 consecutive feature rows in
// exactly this tree, so statistics taken in a conv epilogue and statistics taken from the stored features agree bit for bit.
// Four values at once (the clang DPP builtin costs a v_mov_b32_dpp + v_add_f32 per step; written out, a step is one
// v_add_f32_dpp, and interleaving the four chains covers the VALU-write -> DPP-read wait states; the leading s_nop
// covers the writer of the inputs).  dst = dpp(src0) + src1 with all three the same register.
__device__ __forceinline__ void unit_row_sum4(f32x4& t) {
  float a = t[0], b = t[1], c = t[2], d = t[3];
#define WCT_DPP_STEP(ctrl)                                                             \
  "v_add_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"       \
  "v_add_f32_dpp %1, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"       \
  "v_add_f32_dpp %2, %2, %2 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"       \
  "v_add_f32_dpp %3, %3, %3 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
  asm volatile("s_nop 1\n"
               WCT_DPP_STEP("quad_perm:[1,0,3,2]")
               WCT_DPP_STEP("quad_perm:[2,3,0,1]")
               WCT_DPP_STEP("row_half_mirror")
               WCT_DPP_STEP("row_mirror")
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef WCT_DPP_STEP
  t[0] = a; t[1] = b; t[2] = c; t[3] = d;
}
int launch_conv_first(const ConvFirstArgs& a, hipStream_t s);

struct ConvLastArgs {    // 64 -> 3, no activation (model.py:298)
  const half_t* x;     // [B][H][W][64]
  const half_t* wfrag; // fp16 MFMA A-fragments [k-step 4][lane][8]: row tap*3+cout (27 of 32), k = cin
  const float* bias;   // [3]
  float* y;            // [B][H][W][3] fp32, unclipped
  int B, H, W;
};
int launch_conv_last(const ConvLastArgs& a, hipStream_t s);

int launch_maxpool2x2(const half_t* x, half_t* y, int B, int H, int W, int C, hipStream_t s);
int launch_u8_to_f32(const uint8_t* x, float* y, size_t n, hipStream_t s);       // /255 (wct.py:64)
int launch_f32_to_u8(const float* x, uint8_t* y, size_t n, hipStream_t s);       // uint8(clip*255) (wct.py:68)
int launch_f32_to_f16(const float* x, half_t* y, size_t n, hipStream_t s);
int launch_f16_to_f32(const half_t* x, float* y, size_t n, hipStream_t s);

// ---- the whiten-colour transform: stats_gemm.hip, eigh.hip, spectral.hip, wct.hip, mask.hip, style_swap.hip ----
// generic fp32 GEMM on v_mfma_f32_32x32x2_f32:  D[m][n] = sum_k A(m,k) B(k,n)
// A element (m,k): a_kmajor ? A[k*lda+m] : A[m*lda+k];  B element (k,n): b_kmajor ? B[k*ldb+n] : B[n*ldb+k]
struct GemmArgs {
  const float* A; int lda; int a_kmajor;
  const float* B; int ldb; int b_kmajor;
  const float* a_sub_m;   // subtract vector indexed by m from A (cov centring)       or null
  const float* b_sub_n;   // subtract vector indexed by n from B                      or null
  const float* a_sub_k;   // subtract vector indexed by k from A (apply centring)     or null
  const float* a_scale_k; // scale A by vector indexed by k (E diag(d))               or null
  int M, N, K;
  int ksplit;             // K elements per blockIdx.z slice (multiple of 16)
  float* out32; half_t* out16; int ldo;
  size_t out_split_stride;  // elements between K-slices of out32 (split-K partials)
  const float* bias_n;    // added per output column or null
  // batching: blockIdx.z = batch * nsplit + split; strides in elements (0 = shared)
  int nsplit;
  size_t sA, sB, s_sub_m, s_sub_n, s_sub_k, s_scale_k, s_out, s_bias;
  // round 5 (the transform tail in merged launches over the 2P matrices of a level, batch b = matrix 2 * pair + side):
  const float* A_odd;     // if set: A of an odd batch b is A_odd + (b >> 1) * sA_odd, that of an even one A + (b >> 1) * sA
  size_t sA_odd;
  WctSkip skip;           // batches b with skip_style_mat(b, skip) have nothing to do (skip_rule.h; WCT_SKIP_NONE: a plain batch)
  // blend epilogue (T = Tcs Tw -> M = alpha T + (1 - alpha) I, ops.py:83 folded into the apply matrix): the store carries the
  // blend and the block merges max |M| into mabs[batch] (bit patterns of non-negative floats; zeroed by an earlier kernel)
  int blend; float alpha; unsigned* mabs;
  // refresh products (round 5, launch_wct): run for the batches whose matrix needs it, a no-op for the others.  mask_diag: the
  // [nbatch][M][M] matrices whose DIAGONAL decides (refresh_needed, csrc/stats_gemm.hip); every block of a batch evaluates it the same way
  // and block (0, 0) stores it in mask_out[batch].  mask_in: a mask stored by an earlier launch.
  const float* mask_diag; size_t s_mask; int* mask_out; const int* mask_in;
};

int launch_gemm(GemmArgs g, int nsplit, int nbatch, hipStream_t s);

// Feature matrices are pixel-major: X[n][c] (NHWC flattened), fp32.
enum { WCT_MODE_NP = 0, WCT_MODE_TF = 1 };

// Statistics a conv epilogue took while it wrote a feature map (ConvArgs::usum / umax): [0] content, [1] style; a side
// whose u is null is summed from the features themselves (same bits either way, colsum_kernel).
struct WctFeatStats { const float* u[2]; const unsigned* umax[2]; };

// relu1_1 computed where it is read: the 64-channel map of a side is what conv1_1 makes of an image, so a reader
// that has the image and conv1_1's parameters needs no stored map.  side[0] content, side[1] style: img [P][H][W][3] fp32 (a shared
// style: one image), row n of the side's feature matrix is pixel (n / W, n % W); W a multiple of 16 (the unit sums the means come
// from); wfrag / bias: ConvFirstArgs'.  Given to launch_wct, the covariance of BOTH sides and the apply's content rows are taken
// from the images (C = 64, the statistics of both sides in `stats`): neither feature pointer is read, both may be null.
struct WctImageSide { const float* img; int H, W, clamp01; };
struct WctImageSrc { WctImageSide side[2]; const half_t* wfrag; const float* bias; };

// Prepared styles (wct.hip): a STATE is the style side of one level for one layout and mode -- [mean C][var C][Tcs C x C] floats
// (var for AdaIN, Tcs for WCT).  Its bits depend on the slab count and K-slices of the (content, style) pair it serves: the key.
struct WctStyleKey { int nslab, nsplit, ksplit; };
WctStyleKey wct_style_key(int C, int Nc, int Ns);
size_t wct_style_state_floats(int C);
size_t wct_style_workspace_bytes(int C, int Ns, const WctStyleKey& key);
// the states a transform takes in place of its style features (`prep` below): state[0], or state[k] for style k of a mix.  The
// style pointers may then be null; Ns still names the styles' rows (the content's layout depends on them).
struct WctStyleRef { const float* state[8]; };
// the states of a masked batch (launch_wct_masked_batch): state[p] serves pair p = the p-th (frame, label) with >= 2 rows
struct WctStyleSlots { const float* state[32]; };

// Video warm start (warm.hip): the C x C basis a level's content eigensolves start from when `valid`, and which takes the
// re-orthonormalised eigenvectors of the call's LAST content matrix either way
struct WctWarmRef { float* basis; int valid; };

// Strength maps (strength_rule.h): smap [P][Hm][Wm] uint8 on the device, one map per pair; row n of a pair's N = h x w feature map
// is pixel (n / w, n % w) and reads smap[min(i stride, Hm - 1)][min(j stride, Wm - 1)] -- 255 is the call's alpha, 0 keeps the
// content features.  The statistics, covariance, eigensystem and matrices of the level are the plain call's: only the blend moves
// from the matrix M (alpha = 1 here) to the rows the apply stores.
struct WctStrength { const uint8_t* smap; int Hm, Wm, w, stride; };

// The call block of a transform launcher: what every one of them takes besides its features and their geometry.  The drivers
// (api.h: run_stages) fill workspace, stream, eig_fail, mode and stages from the context, their callers the rest.
struct WctCall {
  float alpha; int mode;    // mode: WCT_MODE_NP / WCT_MODE_TF (unused by the AdaIN launchers, as are stages and sweeps_dev)
  float eps;                // < 0: the reference default; the AdaIN launchers: AdaIN's epsilon
  half_t* out16; float* out32;   // the outputs, either may be null
  void* workspace; size_t workspace_bytes;
  int* sweeps_dev;          // device: the sweeps of every solved matrix, or null
  int stages;               // WCT_STAGE_* of this call
  int* eig_fail;            // device-visible status words: [2] (not converged, non-finite), bumped by the eigensolver, then
                            // [6 size classes][3] solver statistics; or null
  hipStream_t stream;
};
// WCT_STAGE_EIG_FP32UPDATE (with WCT_STAGE_EIG): the eigensolver's tile updates on fp32 MFMA instead of split fp16 -- style-swap, whose
// patch matching is an argmax over the whitened features (csrc/jacobi_pair64.h fused_u)
enum { WCT_STAGE_COV = 1, WCT_STAGE_EIG = 2, WCT_STAGE_APPLY = 4, WCT_STAGE_ALL = 7, WCT_STAGE_EIG_FP32UPDATE = 8 };

// the state of `style` [Ns][C] under `key`: launch_wct's style side alone (adain: launch_adain's), bit for bit
int launch_style_state(const float* style, int Ns, int C, const WctStyleKey& key, int adain, const WctCall& r, float* state);

// P independent whiten-colour transforms:  out = blend(T (x - mc) + ms); content [P][Nc][C], style [P][Ns][C]; out16/out32 [P][Nc][C].
// skip: WCT_SKIP_NONE, or WCT_SKIP_SHARED_STYLE -- style holds ONE feature map used by all P pairs, its statistics and eigensystem
// are computed once.  stats: unit sums / maxima a conv epilogue left beside the features.  prep: one prepared style for all P pairs
// (skip is then ignored; style may be null).  warm: start the P content eigensolves from a stored basis (plain pairs or a prepared
// style only).  sm: a strength map per pair (Nc a multiple of sm->w).  Each of the four may be null.
size_t wct_workspace_bytes(int C, int Nc, int Ns, int P);
int launch_wct(const float* content, int Nc, const float* style, int Ns, int C, int P, WctSkip skip, const WctCall& r,
               const WctFeatStats* stats, const WctStyleRef* prep, const WctWarmRef* warm, const WctStrength* sm = nullptr,
               const WctImageSrc* src = nullptr /* relu1_1 from the images (plain pairs or a shared style) */);
int launch_adain(const float* content, int Nc, const float* style, int Ns, int C, int P, WctSkip skip, const WctCall& r,
                 const WctFeatStats* stats, const WctStyleRef* prep, const WctStrength* sm = nullptr);
// Style mix (Li et al. 2017, sec. 4.2): out = sum_k lambda[k] T(content, styles[k]) for K <= WCT_MIX_MAX styles of any sizes
// Ns[k]; lambda[k] in [0, 1] summing to 1 (normalised by the caller).  One content whitening, K colourings mixed before ONE
// blend product and apply.  sweeps_dev [2K]: slot 2k + 1 style k, slot 0 the content (the even slots k >= 1 read 0).  stats:
// the content side only (u[0] / umax[0]).
enum { WCT_MIX_MAX = 8 };
size_t wct_mix_workspace_bytes(int C, int Nc, const int* Ns, int K, const float* lambda);
int launch_wct_mix(const float* content, int Nc, const float* const* styles, const int* Ns, int K, const float* lambda, int C,
                   const WctCall& r, const WctFeatStats* stats, const WctStyleRef* prep);
int launch_adain_mix(const float* content, int Nc, const float* const* styles, const int* Ns, int K, const float* lambda, int C,
                     const WctCall& r, const WctFeatStats* stats, const WctStyleRef* prep);
// Spatial control (Li et al. 2017, sec. 4.2): K <= WCT_MIX_MAX labelled regions of one content, region k transformed with style k
// alone.  Row r = (i, j) of an h x w feature map has the label mask[min(i * stride, Hm - 1)][min(j * stride, Wm - 1)] of the
// Hm x Wm label map (the content's, at stride 2^(level - 1)).  nk[k]: the rows of label k, counted by the caller (they size
// the launches; nothing is read back), summing to Nc.  A label with nk < 2 rows passes its rows through unchanged.
// sweeps_dev [2P]: pair p = the p-th label with nk >= 2, content 2p, style 2p + 1.
struct MaskGeom { const uint8_t* mask; int Hm, Wm, w, stride; };
size_t mask_compact_workspace_bytes(int N, int G = 1);
// stable partition of the N rows by label: perm [N] (the rows of label 0 in order, then label 1, ...), seg_off [K + 1]
int launch_mask_compact(const MaskGeom& g, int N, int K, int* perm, int* seg_off, void* workspace, hipStream_t s);
// a style region: the nk (host-counted) rows of label k of x [N][C] into xg [nk][C] in pixel order, from a compaction with K > k labels
int launch_mask_gather_segment(const float* x, const int* perm, const int* seg_off, int k, int nk, int C, float* xg, hipStream_t s);
size_t wct_masked_workspace_bytes(int C, int Nc, const int* nk, const int* Ns, int K);
int launch_wct_masked(const float* content, int Nc, const MaskGeom& g, const int* nk, const float* const* styles, const int* Ns, int K,
                      int C, const WctCall& r);
int launch_adain_masked(const float* content, int Nc, const MaskGeom& g, const int* nk, const float* const* styles, const int* Ns, int K,
                        int C, const WctCall& r);
// Spatial control of G <= 32 frames on prepared styles, one launch of every stage for all of them: content and out16 / out32
// [G][Nc][C], g.mask [G][Hm][Wm] (one label map per frame), nk [G][WCT_MIX_MAX] the rows of every label of every frame.  The
// live (frame, label) pairs -- nk >= 2, in frame-major order, at most 32 of them -- take the content side alone; pair p's style
// side is states.state[p], the state of style k under wct_style_key(C, nk, Ns[k]).  Frame f comes out as launch_wct_masked /
// launch_adain_masked give it alone, bit for bit.  (sweeps_dev is not served.)
size_t wct_masked_batch_workspace_bytes(int C, int Nc, int G, const int* nk, const int* Ns, int K);
int wct_masked_batch_pairs(int G, const int* nk, int K);
int launch_mask_compact_batch(const MaskGeom& g, int N, int K, int G, int* perm, int* seg_off, void* workspace, hipStream_t s);
int launch_wct_masked_batch(const float* content, int Nc, int G, const MaskGeom& g, const int* nk, const int* Ns, int K, int C,
                            const WctCall& r, const WctStyleSlots& states);
int launch_adain_masked_batch(const float* content, int Nc, int G, const MaskGeom& g, const int* nk, const int* Ns, int K, int C,
                              const WctCall& r, const WctStyleSlots& states);
// Symmetric eigensolver (batched): A [nmat][C][C] is overwritten (diag -> eigenvalues),
// V [nmat][C][C] gets eigenvectors in columns, unsorted: eigenpair j is the one that grew out of coordinate j
// (jacobi_unexchange_kernel).  C multiple of 32, 32 <= C <= 1024.
// sweeps_done_dev[m]: sweeps used (> 0) if matrix m converged, -sweeps if it was still rotating when the sweep
// budget ran out, <= -1000 for non-finite input; eig_fail as in WctCall.
int launch_jacobi_eigh(float* A, float* V, int C, int nmat, void* workspace,
                       size_t workspace_bytes, int* sweeps_done_dev, int* eig_fail, hipStream_t s);
size_t jacobi_workspace_bytes(int C, int nmat);

// Style-swap at relu5_1 (ops.py:145-278): one pair, content [hc*wc][C], style [hs*ws][C] fp32.
size_t style_swap_workspace_bytes(int C, int hc, int wc, int hs, int ws, int patch, int stride);
int launch_style_swap(const float* content, int hc, int wc, const float* style, int hs, int ws, int C,
                      float alpha, int patch, int stride, float eps, half_t* out16, float* out32,
                      void* workspace, size_t workspace_bytes, hipStream_t s, int* eig_fail);

// ---- train.hip ------------------------------------------------------------
int launch_im2col_act(const half_t* x, float* col, int B, int H, int W, int C, int upsample, hipStream_t s);
int launch_im2col_grad(const float* g, float* col, int B, int H, int W, int C, hipStream_t s);
int launch_reflect_fold(const float* gp, float* g, int B, int H, int W, int C, hipStream_t s);
int launch_relu_mask16(float* g, const half_t* act, size_t n, hipStream_t s);
int launch_relu_mask32(float* g, const float* act, size_t n, hipStream_t s);
int launch_upsample_adjoint(const float* gb, float* gs, int B, int h, int w, int C, hipStream_t s);
int launch_maxpool_adjoint(const half_t* pre, const float* gpool, float* gpre, int B, int H, int W, int C, hipStream_t s);
int launch_mse(const float* a, const float* b, size_t n, float weight, float* grad, int accumulate, double* partial,
               float* loss_out, hipStream_t s);
int launch_tv(const float* x, int B, int H, int W, int C, float weight, float* grad, double* partial, float* loss_out, hipStream_t s);
int launch_bias_grad(const float* g, size_t rows, int C, float* partial, float* out, hipStream_t s);
int launch_reduce_slabs(const float* partial, size_t n, int nslab, float* out, hipStream_t s);
int launch_adam(float* w, float* m, float* v, const float* g, size_t n, float lr_t, float b1, float b2, float eps, hipStream_t s);
int launch_pack_conv_frag(const float* w, half_t* frag, int cin, int cout, hipStream_t s);
int launch_pack_conv_wino_frag(const float* w, half_t* frag, int cin, int cout, hipStream_t s);
int launch_pack_last_frag(const float* w, half_t* frag, hipStream_t s);
int launch_transpose_w(const float* w, float* wt, int cin, int cout, int cout_pad, hipStream_t s);
int launch_pad3to4(const float* x, float* y, size_t n, hipStream_t s);
int launch_conv_dgrad(const float* g, const float* wt, int B, int H, int W, int cin, int cout,
                      float* col, float* gp, float* gin, void* scratch, hipStream_t s);
int launch_conv_wgrad(const half_t* x16, int upsample, const float* g, int ldg, int B, int H, int W, int cin, int cout,
                      float* col, float* partial, int nsplit, float* dw, void* scratch, hipStream_t s);
int conv_wgrad_splits(int B, int H, int W);
int launch_pow2_scale(const float* x, size_t n, void* scratch, hipStream_t s);   // scratch[1] = 2^k with max|x| 2^k in [8192,16384)
int launch_conv_first_dgrad(const float* g, const float* wf, float* gp, int B, int H, int W, hipStream_t s);

// ---- coral.hip ------------------------------------------------------------
struct CoralApplyArgs {
  double M[9], src_mean[3], src_std[3], tgt_mean[3], tgt_std[3];
};
int launch_coral_stats(const uint8_t* img, size_t npix, unsigned long long* partial, int nblocks,
                       unsigned long long* out9, hipStream_t s);
int launch_coral_apply(const uint8_t* src, size_t npix, const CoralApplyArgs& a, uint8_t* out_u8,
                       double* out_f64, hipStream_t s);

// ---- colors.hip -----------------------------------------------------------
// Luminance-only colour preservation (colors_rule.h): out [B][Ho][Wo][3] = the luminance of the stylized frame on the colours of
// content [B][Hc][Wc][3], content pixel (min(y, Hc - 1), min(x, Wc - 1)); Ho >= Hc, Wo >= Wc.
// _f32: the chain's last launch -- frame is the fp32 decode (quantised as launch_f32_to_u8 does), content uint8 or, with
// content_f32, fp32 in [0,1] (quantised the same way).  _u8: both uint8; out may be stylized.
int launch_content_colors_f32(const float* frame, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                              uint8_t* out, hipStream_t s);
int launch_content_colors_u8(const uint8_t* stylized, const uint8_t* content, int B, int Ho, int Wo, int Hc, int Wc, uint8_t* out,
                             hipStream_t s);
// _u8_any: _u8 with the content of a stylize call (content_f32: fp32 in [0,1], quantised as above) -- the colour op behind the
// guided filter, on frames that are uint8 already
int launch_content_colors_u8_any(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                                 uint8_t* out, hipStream_t s);

// ---- guided.hip -----------------------------------------------------------
// Guided smoothing (guided_rule.h): out [B][Ho][Wo][3] = the stylized frames filtered with the grey of content [B][Hc][Wc][3]
// (uint8, or with content_f32 fp32 in [0,1] quantised as launch_f32_to_u8 does) as guide, content pixel (min(y, Hc - 1),
// min(x, Wc - 1)).  Two launches; workspace: guided_workspace_bytes(B, Ho, Wo) bytes on the device; out may be stylized; any base
// address.  guided_check: B outside 1 .. 32, Ho < Hc or Wo < Wc, a radius outside 1 .. 64, eps_q outside 1 .. 65025, or
// B * Ho * Wo * 3 >= 2^31, or a guide that is neither of the two, is WCT_ERR_ARG with a message.
// guide: GUIDE_GREY (the grey of the content, guided_rule.h: 24 B of workspace per pixel) or GUIDE_COLOR (its three channels,
// guided_color_rule.h: 48 B per pixel, the kernels of guided_color.hip) -- the values of WCT_GUIDE_* of the public header.
constexpr int GUIDE_GREY = 0, GUIDE_COLOR = 1;
int guided_check(int B, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int guide);
size_t guided_workspace_bytes(int B, int Ho, int Wo, int guide);
int launch_guided_filter(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                         int eps_q, int guide, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_ab: pass 1 alone under the grey guide -- ab [B][Ho][Wo][3][2] int32, guided_workspace_bytes(B, Ho, Wo, GUIDE_GREY)
int launch_guided_ab(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                     int eps_q, void* ab, hipStream_t s);
// ---- guided_up.hip --------------------------------------------------------
// Guided upsampling (guided_up_rule.h): out [B][H][W][3] = the small stylized frames s [B][h][w][3], filtered with the small
// contents c [B][hc][wc][3] as guide, delivered at the size of the full contents C [B][H][W][3] (both contents uint8, or with
// content_f32 both fp32 in [0,1] quantised as launch_f32_to_u8 does).  Three launches: launch_guided_ab, the window means of the
// coefficients, the full-size pass.  workspace: guided_up_workspace_bytes(B, h, w) bytes on the device (8-byte aligned); out
// overlaps no input; any base address (whole-dword loads and stores where W % 4 == 0 and the bases allow them).
// guided_up_check: B outside 1 .. 32, h < hc or w < wc, H < hc or W < wc, a radius or eps_q out of range, or B * H * W * 3
// (or B * h * w * 3) >= 2^31 is WCT_ERR_ARG with a message that names the argument.
int guided_up_check(int B, int h, int w, int hc, int wc, int H, int W, int radius, int eps_q);
size_t guided_up_workspace_bytes(int B, int h, int w);
int launch_guided_upsample(const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B, int h,
                           int w, int hc, int wc, int H, int W, int radius, int eps_q, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_up_full: the full-size pass alone -- mean [B][h][w][3][2] int32 (8-byte aligned) + content_full [B][H][W][3] uint8 ->
// out [B][H][W][3]; the caller has checked the arguments (guided_up_check)
int launch_guided_up_full(const int32_t* mean, const uint8_t* content_full, uint8_t* out, int B, int H, int W, int h, int w, int hc, int wc,
                          hipStream_t s);
// ---- guided_color.hip: the two launches of the colour guide; launch_guided_filter has checked the arguments
int launch_guided_color(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                        int eps_q, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_color_ab: pass 1 alone under the colour guide -- ab [B][Ho][Wo][12] int32, 16-byte aligned,
// guided_workspace_bytes(B, Ho, Wo, GUIDE_COLOR)
int launch_guided_color_ab(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc, int radius,
                           int eps_q, void* ab, hipStream_t s);
// ---- guided_up_color.hip --------------------------------------------------
// Guided upsampling under the colour guide (guided_up_color_rule.h): the arguments, the refusals (guided_up_check) and the
// contract of launch_guided_upsample.  Three launches: launch_guided_color_ab, the window means of the twelve coefficients, the
// full-size pass.  workspace: guided_up_color_workspace_bytes(B, h, w) bytes on the device (96 B per small pixel, 16-byte aligned);
// any base address of the images (whole 16-bit loads and stores where W is even and the bases allow them).
size_t guided_up_color_workspace_bytes(int B, int h, int w);
int launch_guided_upsample_color(const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B,
                                 int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, void* workspace, uint8_t* out,
                                 hipStream_t s);
// ---- guided_time.hip ------------------------------------------------------
// Temporal guided smoothing (guided_time_rule.h): the grey-guide filter with its box extended over frames_t frames on each side,
// on a clip of F frames [F][Ho][Wo][3] with contents [F][Hc][Wc][3] resident on the device.  out [f1 - f0][Ho][Wo][3] = the
// filtered frames f0 .. f1 - 1 of that clip; it may be stylized + f0 Ho Wo 3.  Two launches; workspace:
// guided_workspace_bytes(F, Ho, Wo, GUIDE_GREY) bytes (a frame's coefficients sit at its position in the clip).
// guided_time_check: F outside 1 .. 32, a range that is not 0 <= f0 < f1 <= F, Ho < Hc or Wo < Wc, parameters outside
// wct_guided_time_params_ok, or F * Ho * Wo * 3 >= 2^31 is WCT_ERR_ARG with a message.
int guided_time_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1);
int guided_time_max_radius(int frames_t);                  // 64 / 51 / 40 / 33 at 0 .. 3 frames on each side, else 0
int launch_guided_time(const uint8_t* stylized, const void* content, int content_f32, int F, int Ho, int Wo, int Hc, int Wc, int radius,
                       int eps_q, int frames_t, int f0, int f1, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_time_ab: pass 1 alone on uint8 contents -- ab [F][Ho][Wo][3][2] int32, the frames max(0, f0 - T) .. min(F, f1 + T) - 1
int launch_guided_time_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                          int frames_t, int f0, int f1, int32_t* ab, hipStream_t s);
// ---- guided_motion.hip ----------------------------------------------------
// Temporal guided smoothing along camera motion (guided_motion_rule.h): launch_guided_time with the window of every neighbouring
// frame shifted by the difference of the positions pos [F][2] (py, px), host memory, read before the call returns.  Same clip,
// range, workspace and aliasing.  guided_motion_check: what guided_time_check refuses, a null pos, or a step between two frames
// above 16 on either axis.
int guided_motion_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1, const int32_t* pos);
int launch_guided_motion(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                         int frames_t, const int32_t* pos, int f0, int f1, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_motion_ab: pass 1 alone -- ab as launch_guided_time_ab writes it, under the positions
int launch_guided_motion_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                            int frames_t, const int32_t* pos, int f0, int f1, int32_t* ab, hipStream_t s);
// The estimator of those positions: one step per pair of consecutive contents [F][Hc][Wc][3] on the device, by exhaustive search
// over |dy|, |dx| <= range.  Three launches (none for F = 1); *steps = where in the workspace the F - 1 steps (dy, dx) int32 will
// be.  workspace: motion_workspace_bytes bytes.  motion_check: F outside 1 .. 32, a range outside 1 .. 16, Hc or Wc < 4 range, or
// Hc * Wc > 2^28.
int motion_check(int F, int Hc, int Wc, int range);
size_t motion_workspace_bytes(int F, int Hc, int Wc, int range);
int launch_motion_global(const uint8_t* content, int F, int Hc, int Wc, int range, void* workspace, const int32_t** steps, hipStream_t s);
// ---- guided_color_time.hip ------------------------------------------------
// Temporal guided smoothing with the colour guide (guided_color_time_rule.h): launch_guided_motion with the three content channels
// as guide -- uint8 contents, the same clip, range and aliasing; pos may be null (no motion: every position zero).  Two launches.
// workspace: guided_workspace_bytes(F, Ho, Wo, GUIDE_COLOR) bytes, 16-byte aligned (48 B per pixel of the clip).
// guided_color_time_check: guided_motion_check with positions, guided_time_check without, so their messages stay in front.
int guided_color_time_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1, const int32_t* pos);
int launch_guided_color_time(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                             int frames_t, const int32_t* pos, int f0, int f1, void* workspace, uint8_t* out, hipStream_t s);
// launch_guided_color_time_ab: pass 1 alone -- ab [F][Ho][Wo][12] int32, the frames max(0, f0 - T) .. min(F, f1 + T) - 1
int launch_guided_color_time_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                                int frames_t, const int32_t* pos, int f0, int f1, int32_t* ab, hipStream_t s);
// ---- guided_up_time.hip ---------------------------------------------------
// Temporal guided upsampling (guided_up_time_rule.h): out [f1 - f0][H][W][3] = frames f0 .. f1 - 1 of the clip of F small stylized
// frames s [F][h][w][3] with small contents c [F][hc][wc][3], the coefficients formed over the 3-D window of frames_t frames on
// each side -- shifted by the differences of pos [F][2] (host memory, read before the call returns) unless pos is null --,
// delivered against content_full [f1 - f0][H][W][3], the full contents of the delivered frames only.  Three launches: pass 1 of
// the temporal (or motion) filter, the window means, the full-size pass of guided_up.hip.  workspace:
// guided_up_time_workspace_bytes bytes (24 B per small pixel of the F frames and of the delivered ones, 8-byte aligned); out
// overlaps no input.  guided_up_time_check: what guided_time_check refuses on the small clip, what guided_up_check refuses on
// f1 - f0 delivered frames, or a step of pos above 16 on either axis.
int guided_up_time_check(int F, int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, int frames_t, int f0, int f1,
                         const int32_t* pos);
size_t guided_up_time_workspace_bytes(int F, int h, int w, int f0, int f1);
int launch_guided_upsample_time(const uint8_t* stylized, const uint8_t* content_small, const uint8_t* content_full, int F, int h, int w,
                                int hc, int wc, int H, int W, int radius, int eps_q, int frames_t, const int32_t* pos, int f0, int f1,
                                void* workspace, uint8_t* out, hipStream_t s);

// ---- noise.hip ------------------------------------------------------------
// Seeded noise for texture synthesis (noise_rule.h): out [B][H][W][3] uint8 on the device, image b = sample first_sample + b of
// `seed`; smooth: the rule's 27 202 27 filter along y and x.  One launch; any base address; B * H * W * 3 >= 2^31 is WCT_ERR_ARG.
int launch_texture_noise(uint8_t* out, int B, int H, int W, unsigned seed, unsigned first_sample, int smooth, hipStream_t s);

// ---- wrap.hip -------------------------------------------------------------
// Periodic extension and its inverse, B maps of E elements of elem_bytes (4: fp32, any E; 2: fp16, E a multiple of 8) per pixel:
// out [B][t + H + b][l + W + r][E] with out(y, x) = in((y - t) mod H, (x - l) mod W), and out [B][h][w][E] = the interior of
// in [B][Hp][Wp][E] at (t, l).  A padded map of 2^31 bytes or more is WCT_ERR_ARG with a message.
int launch_wrap_pad(const void* in, void* out, int B, int H, int W, int E, int elem_bytes, int t, int b, int l, int r, hipStream_t s);
int launch_wrap_crop(const void* in, void* out, int B, int Hp, int Wp, int E, int elem_bytes, int t, int l, int h, int w, hipStream_t s);

// ---- resize.hip -----------------------------------------------------------
// Bilinear resize by Pillow's 8-bit rule (resize_rule.h): in [B][H][W][3] -> out [B][h][w][3] uint8 on the device, one launch, no
// workspace.  A geometry's plan is host work: resize_plan fills `tabs` (resize_table_ints int32 words: the bounds and taps of both
// axes) and picks the tile height `th`; the caller keeps the tables on the device.  WCT_ERR_ARG: input or output bytes >= 2^31
// (resize_check_bytes, launch_resize), a vertical reduction whose taps of one output row do not fit the kernel's LDS (resize_plan).
struct ResizeGeom { int H, W, h, w, ksx, ksy, th; };
int resize_check_bytes(int B, int H, int W, int h, int w);
size_t resize_table_ints(int H, int W, int h, int w);
int resize_plan(int H, int W, int h, int w, ResizeGeom* g, int* tabs);
int launch_resize(const uint8_t* in, uint8_t* out, int B, const ResizeGeom& g, const int* tabs_dev, hipStream_t s);
