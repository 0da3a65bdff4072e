// K5 of the whiten-colour transform (the stage list: wct.hip): the batched symmetric eigensolver -- two-sided block Jacobi.
//   Column blocks of B = M2/2 are paired round-robin (jacobi_dev.h); each pair's M2 x M2 diagonal problem gets one cyclic
//   Jacobi step -- the D part --, then every M2 x M2 tile of A (and of the eigenvector matrix V) is updated as Qg^T A_gh Qh
//   on the MFMA pipe -- the U part.  ONE launch per outer step carries { D(s), U(s-1) } (the look-ahead launches:
//   jacobi_pair32.h), C/B steps per sweep.  A per-matrix `done` flag turns later launches into no-ops.
//   Two kernels: jacobi_fused_kernel for the 32-wide block pairs, pair problems as LDS images (jacobi_pair32.h), and
//   jacobi_fused4_kernel for the 64-wide ones, pair problems resident in registers (jacobi_pair64.h); jacobi_wide_pairs
//   chooses.  With many matrices the 64-wide path takes V out of the tile update: jacobi_vstrip_kernel applies a whole launch
//   segment's rotations to V held in registers, on a side stream.
// This unit: those kernels, the residual measurement and the checks, the host driver of a solve (segments, look-ahead
// launches, the V pass) and the transform's eigensolve stage.
#include "wct_stages.h"
#include <stdlib.h>
#include "jacobi_pair32.h"
#include "jacobi_pair64.h"

// A launcher that returns void (the per-launch helpers of the eigensolver's trains) notes a refused launch here, with the kernel's
// name, the moment it happens; the train's driver returns it (launch_rc_take) instead of a generic failure at a later sync.
static thread_local int launch_rc_sticky = WCT_OK;
#define LAUNCH_NOTE(what) do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess && launch_rc_sticky == WCT_OK) { \
    wct_set_error("launch of %s refused: %s (%s:%d)", what, hipGetErrorString(e_), __FILE__, __LINE__); launch_rc_sticky = WCT_ERR_HIP; } } while (0)
static inline int launch_rc_take() { const int r = launch_rc_sticky; launch_rc_sticky = WCT_OK; return r; }

// grid: [nmat * npair pair problems (if has_d)] [ntask * nmat update tasks, task-major (if has_u)]; pair32::NT = 256 threads
__global__ __launch_bounds__(256, 2) void jacobi_fused_kernel(JacobiFusedArgs p) {
  extern __shared__ __attribute__((aligned(16))) float jsm[];
  const int npair = p.C / pair32::B / 2;
  const int n_d = p.has_d ? p.nmat * npair : 0;
  int b = blockIdx.x;
  if (b < n_d) {
    const int m = b / npair, g = b % npair;
    pair32::fused_d(p, m, g, jsm);                  // (checks the matrix' done flag itself, after issuing its loads)
  } else {
    b -= n_d;
    const int task = b / p.nmat, m = b % p.nmat;
    if (p.st[m].done) return;
    pair32::fused_u(p, m, task, jsm);
  }
}

// the same grid; pair64::NT = 256 threads
__global__ __launch_bounds__(256, 4) void jacobi_fused4_kernel(JacobiFusedArgs p) {
  extern __shared__ __attribute__((aligned(16))) float jsm[];
  const int npair = p.C / pair64::B / 2;
  const int n_d = p.has_d ? p.nmat * npair : 0;
  int b = blockIdx.x;
  if (b < n_d) {
    const int m = b / npair, g = b % npair;
    pair64::fused_d(p, m, g, jsm);
  } else {
    b -= n_d;
    const int task = b / p.nmat, m = b % p.nmat;
    if (p.st[m].done) return;
    pair64::fused_u(p, m, task, jsm);
  }
}
static_assert(pair32::NT == 256 && pair64::NT == 256, "the launch bounds above");

// ---------------------------------------------------------------------------
// V <- V Q for all the rotations of one launch segment, with V resident in REGISTERS (the V pass; 64-wide block pairs).
// Updating V inside the tile update streams the whole of V through the chip at every outer step (64 % of the update's
// traffic: 4 MB per 512-channel matrix and step), although nothing in the solver reads V.  Here a wave owns 16 rows of V
// -- C/16 tiles of 16x16 held as MFMA accumulators, C/4 registers per lane -- and applies the rotation matrices of all
// the steps of a segment (the fp16 log the pair problems wrote) without V leaving the registers:
//   (V Q_h)^T = Q_h^T V^T is computed tile by tile on split fp16 (see qfrag16_k, jacobi_dev.h); two 16x16 tiles of V^T in the
//   C/D layout (lane (n, q), register r  <->  V[row n][tile column 4 q + r]) are ALREADY the B operand of a K-chunk, so the
//   old tiles feed the MFMAs straight from the accumulator registers (split into hi + lo on the way), the results arrive
//   in the same layout, and the only operand that is loaded is Q (fragment order: one 16-byte LDS read per fragment).
// Register indices must be static: the strip is kept in POSITION order of the round-robin pairing (pair g = positions g
// and NBLK-1-g; the intra step pairs positions 2g, 2g+1, natural order = the order of step 0); advancing one outer step
// moves position pos+1 to pos (pos >= 1) and position 1 to NBLK-1 -- a static register rotation.
// V traffic: one read and one write per SEGMENT instead of per step.  Runs on a side stream behind the segment, beside
// the next segment's pair problems (MFMA pipe and registers here, LDS and VALU there).
// ---------------------------------------------------------------------------
struct VStripArgs {
  float* V; const half_t* Qlog;     // Qlog: [slot][nmat][npair][2*M2*M2] fp16 hi/lo fragments (qfrag16_k), slot = step - step_begin
  const JacobiState* st;
  int C, nmat, step_begin, step_end, seg;
  int mat_major; // grid (nmat, strips) instead of (strips, nmat): see vstrip_launch
};

// The rotation log reaches the block by LDS-DMA into a RING of VS_RING tiles (buffer_load_dwordx4 ... lds, 1 KiB per wave
// instruction, no registers), VS_RING - 1 tiles ahead of the one in use: an access takes ~2 us (the log streams from HBM: 64 MB
// per segment at 64 matrices) against ~0.2 us of MFMA work per tile, and while a block waits it holds its registers.  Protocol per
// tile q: s_waitcnt vmcnt((VS_RING - 2) x NDMA) retires this wave's share of tile q (the counter is in order), the barrier makes it
// everybody's and retires slot (q - 1) % VS_RING, whose refill (tile q + VS_RING - 1) is issued at once.  Past the end of the
// segment the refills re-fetch the last tile into slots nobody reads: the outstanding count stays constant and so does the wait.
// FIVE tiles (80 KB), and the fragments of a tile requested one K-chunk ahead instead of all sixteen at once (364 registers per
// lane against 398): two pair-problem / update blocks fit beside a block of the pass on every CU, and the launch that opens the
// next segment does not wait for it (per-launch trace: 86-117 us for that launch behind a pass that held its CU alone, 25-35
// without): eigensolver 12.05 -> 11.55 ms per 32-pair step, 8.44 -> 7.9 at 16 pairs, frames identical
// (profiles/r05_vstrip_coresident.txt: rings of 4 / 5 / 6 / 7 / 8 tiles = 11.86 / 11.55 / 11.60 / 11.78 / 11.88).
// Four waves a block, one per SIMD: 224 VGPRs + 72 AGPRs, no scratch (profiles/r06_vstrip_w4.txt).
constexpr int VS_RING = 5, VS_WAVES = 4;
constexpr size_t VS_LDS_BYTES = (size_t)VS_RING * pair64::FR * sizeof(float);   // a tile of fp16 hi / lo fragments = FR * 4 bytes
static_assert(VS_LDS_BYTES == 81920, "the ring of the V pass");

// NBLK = C / 32 column blocks: 8 and 16 (C = 256 and 512)
template <int NBLK>
__global__ __launch_bounds__(256) void jacobi_vstrip_kernel(VStripArgs p) {
  constexpr int M2 = pair64::M2, B = pair64::B, NCH = pair64::NCH, FR = pair64::FR, W = VS_WAVES;
  constexpr int TB = B / 16, NPAIR = NBLK / 2, C = NBLK * B;
  constexpr int TILE_BYTES = FR * 4;                       // fp16 hi / lo fragments of one rotation matrix
  constexpr int NDMA = TILE_BYTES / 1024 / W;              // 1-KiB DMA pieces per wave and tile
  static_assert(W * 64 == 256, "the launch bound above");
  static_assert(NDMA >= 1 && NDMA * W * 1024 == TILE_BYTES, "a tile is a whole number of 1-KiB pieces per wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char vs_ring[];
  const int m = p.mat_major ? blockIdx.x : blockIdx.y;
  if (p.st[m].seg_stop <= p.seg) return;   // no rotations of this segment belong to the matrix (done before it began)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int row0 = ((p.mat_major ? blockIdx.y : blockIdx.x) * W + wave) * 16;
  float* Vm = p.V + (size_t)m * C * C + (size_t)(row0 + li) * C + 4 * lq;
  const size_t slot_stride = (size_t)p.nmat * NPAIR * FR;
  const float* qbase = reinterpret_cast<const float*>(p.Qlog) + (size_t)m * NPAIR * FR;   // a tile of fp16 hi/lo fragments = FR * 4 bytes too
  // tile q of the segment: step = step_begin + q / NPAIR, pair = q % NPAIR
  const int ntile = (p.step_end - p.step_begin) * NPAIR;
  const __amdgpu_buffer_rsrc_t q_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)qbase, 0, 0x7FFFFFFF, 0x00020000);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  auto dma = [&](int q) {                                  // (uniform) tile min(q, ntile - 1) -> ring slot q % VS_RING
    const int qq = q < ntile ? q : ntile - 1;
    const unsigned soff = (unsigned)(((size_t)(qq / NPAIR) * slot_stride + (size_t)(qq % NPAIR) * FR) * sizeof(float));
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int piece = wave_u + i * W;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(q_rsrc, reinterpret_cast<__attribute__((address_space(3))) void*>(
          (__attribute__((address_space(3))) unsigned char*)vs_ring + (q % VS_RING) * TILE_BYTES + piece * 1024), 16, lane * 16, soff + piece * 1024, 0, 0);
    }
  };
  f32x4 v[NBLK * TB];
  auto block_at = [&](int pos, int step) { return step < 0 ? pos : rr_idx(pos, step, NBLK); };
#pragma unroll
  for (int pos = 0; pos < NBLK; ++pos) {
    const int blk = block_at(pos, p.step_begin);
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) v[pos * TB + tb] = *reinterpret_cast<const f32x4*>(Vm + blk * B + tb * 16);
  }
  // (the strip's loads are OLDER than the DMAs on the in-order counter: the first tile's wait then covers the strip and tile 0 only)
  asm volatile("" ::: "memory");
#pragma unroll
  for (int q0 = 0; q0 < VS_RING - 1; ++q0) dma(q0);       // tiles 0 .. VS_RING - 2
  int q = 0;
  // one pair (the g-th of its step: g is a compile-time constant once the loops below are unrolled, and so are the
  // positions pa / pb and the register sets g % PD, (g + 1) % PD): tiles x = positions pa, pb;
  // out[mt] = sum over chunks of the three split-operand MFMAs.  The strip must stay in registers.
#define VSTRIP_PAIR(pa, pb, g)                                                                                       \
  {                                                                                                                  \
    /* this wave's pieces of tile q have landed; lgkmcnt(0): its ds_reads of tile q - 1 have RETIRED before the barrier behind which    \
       another wave refills that slot (the fragments were consumed by the previous pair's MFMAs, the wait is free) */       \
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((VS_RING - 2) * NDMA) : "memory");                           \
    __builtin_amdgcn_s_barrier();                          /* ... everybody's; and nobody reads tile q - 1 any more */ \
    asm volatile("" ::: "memory");                                                                                   \
    dma(q + VS_RING - 1);                                                                                            \
    const half_t* qb = reinterpret_cast<const half_t*>(vs_ring + (q % VS_RING) * TILE_BYTES);                        \
    f32x4 out[2 * TB];                                                                                               \
    _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt) out[mt] = f32x4{0.f, 0.f, 0.f, 0.f};                      \
    /* The fragments of a K-chunk are requested together, one chunk ahead of the MFMAs that use them (round 5: hipcc \
       read them one at a time, each ds_read_b128 followed by s_waitcnt lgkmcnt(0) and its MFMAs -- sixteen exposed   \
       LDS round trips per pair, and the three MFMAs of an accumulator back to back: 100 us of a block's 115).  Per   \
       accumulator the order of the six products is unchanged (chunk 0: lo.hi, hi.lo, hi.hi; chunk 1 likewise). */   \
    half8 fa[NCH][2 * TB][2];                                                                                        \
    _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt)                                                            \
      _Pragma("unroll") for (int part = 0; part < 2; ++part)                                                         \
        fa[0][mt][part] = *reinterpret_cast<const half8*>(qb + (((mt * NCH + 0) * 2 + part) * 64 + lane) * 8);       \
    __builtin_amdgcn_sched_barrier(0);                     /* (the order written here, not the scheduler's) */                        \
    half8 bh[NCH], bl[NCH];                                                                                          \
    _Pragma("unroll") for (int c = 0; c < NCH; ++c) {                                                                \
      /* tiles 2c, 2c+1 of the pair's 2 TB tiles: positions pa (tiles 0..TB-1) and pb (TB..2TB-1) */                 \
      const f32x4 x0 = 2 * c < TB ? v[(pa) * TB + 2 * c] : v[(pb) * TB + 2 * c - TB];                                \
      const f32x4 x1 = 2 * c + 1 < TB ? v[(pa) * TB + 2 * c + 1] : v[(pb) * TB + 2 * c + 1 - TB];                    \
      const float xx[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};                                  \
      split_f16x8(xx, bh[c], bl[c]);                                                                                 \
    }                                                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    _Pragma("unroll") for (int c = 0; c < NCH; ++c) {                                                                \
      if (c + 1 < NCH) {                                   /* the next chunk's fragments under this chunk's MFMAs */ \
        _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt)                                                        \
          _Pragma("unroll") for (int part = 0; part < 2; ++part)                                                     \
            fa[c + 1][mt][part] = *reinterpret_cast<const half8*>(qb + (((mt * NCH + c + 1) * 2 + part) * 64 + lane) * 8); \
      }                                                                                                              \
      _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt) out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[c][mt][1], bh[c], out[mt], 0, 0, 0); \
      _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt) out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[c][mt][0], bl[c], out[mt], 0, 0, 0); \
      _Pragma("unroll") for (int mt = 0; mt < 2 * TB; ++mt) out[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[c][mt][0], bh[c], out[mt], 0, 0, 0); \
      __builtin_amdgcn_sched_barrier(0);                                                                             \
    }                                                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    _Pragma("unroll") for (int t = 0; t < TB; ++t) { v[(pa) * TB + t] = out[t]; v[(pb) * TB + t] = out[TB + t]; }    \
    ++q;                                                                                                             \
  }
  // (the loops over g are spelled out with compile-time g: `#pragma unroll` alone leaves g a variable inside the macro)
  auto step_pairs = [&](auto INTRA) {
    constexpr bool intra = decltype(INTRA)::value;
#define VP(G) if constexpr ((G) < NPAIR) { if constexpr (intra) VSTRIP_PAIR(2 * (G), 2 * (G) + 1, G) else VSTRIP_PAIR(G, NBLK - 1 - (G), G) }
    VP(0) VP(1) VP(2) VP(3) VP(4) VP(5) VP(6) VP(7)
#undef VP
  };
#pragma unroll 1
  for (int step = p.step_begin; step < p.step_end; ++step) {
    if (step < 0) {
      step_pairs(std::true_type{});          // natural order
    } else {
      step_pairs(std::false_type{});
      if (step + 1 < p.step_end && NBLK > 2) {        // positions of the next step: pos <- pos + 1, NBLK - 1 <- 1
        f32x4 keep[TB];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) keep[tb] = v[1 * TB + tb];
#pragma unroll
        for (int pos = 1; pos < NBLK - 1; ++pos)
#pragma unroll
          for (int tb = 0; tb < TB; ++tb) v[pos * TB + tb] = v[(pos + 1) * TB + tb];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) v[(NBLK - 1) * TB + tb] = keep[tb];
      }
    }
  }
#undef VSTRIP_PAIR
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the refills past the end are still landing in this block's LDS
  const int last = p.step_end - 1;
#pragma unroll
  for (int pos = 0; pos < NBLK; ++pos) {
    const int blk = block_at(pos, last);
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) *reinterpret_cast<f32x4*>(Vm + blk * B + tb * 16) = v[pos * TB + tb];
  }
}

// after a solve: matrices whose final state sits in the second buffer are copied back into A
__global__ __launch_bounds__(256) void jacobi_gather_kernel(float* A, const float* P1, const JacobiState* st, int C, int cur_final) {
  const int m = blockIdx.y;
  const int buf = st[m].done ? st[m].pad : cur_final;
  if (buf == 0) return;
  const size_t cc = (size_t)C * C, n4 = cc / 4;
  const f32x4* src = reinterpret_cast<const f32x4*>(P1 + m * cc);
  f32x4* dst = reinterpret_cast<f32x4*>(A + m * cc);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

constexpr int JACOBI_ROWSUM_MAX = 1024;                // words of row sums per matrix (C <= 1024; see JACOBI_ROW_K below)
// mat0 = index of the first matrix in the 2P batch (0: a solve takes the whole batch); skipped style matrices start out `done`
__global__ __launch_bounds__(256) void jacobi_init_kernel(const float* A, float* V, JacobiState* st, int C, int mat0, int skip, unsigned* rowsum) {
  __shared__ float red[4];
  const int m = blockIdx.y;
  const bool dead = skip_style_mat(mat0 + m, skip);
  const size_t cc = (size_t)C * C;
  if (!dead)
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cc; i += (size_t)gridDim.x * blockDim.x)
      V[(size_t)m * cc + i] = (i / C == i % C) ? 1.f : 0.f;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < C; i += 256) rowsum[(size_t)m * JACOBI_ROWSUM_MAX + i] = 0u;      // (jacobi_resid_kernel adds, jacobi_check_kernel clears)
    float mx = 0.f;                          // NaN diagonals drop out of fmaxf; the pair kernels flag them
    if (!dead) for (int i = threadIdx.x; i < C; i += 256) mx = fmaxf(mx, fabsf(A[(size_t)m * cc + (size_t)i * C + i]));
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      JacobiState z;
      z.offmax = 0u; z.done = dead ? 1 : 0; z.sweeps = 0; z.offsig = 0u;
      z.floor = JACOBI_SIG_FLOOR * fminf(mx, 3.0e38f); z.last_sig = 0u; z.dmax = 0u; z.r2 = -1.f; z.r2l = -1.f; z.pad = 0;
      z.seg_stop = dead ? 0 : 0x7fffffff; z.pad2 = 0;
      st[m] = z;
    }
  }
}

// State of a matrix AFTER a sweep, measured on the matrix itself: means of squared cosines e^2 / (d_p d_q) of the
// off-diagonal residual E.  A squared cosine is at once the relative perturbation E still causes in the smaller
// eigenvalue of the pair (what decides on which side of the reference's 1e-5 cut-off it falls, and how accurate its
// gain is) and the size of the first-order term F o E of a spectral function against f(D) (spectral_open_all_kernel).
//   STRICT (decides when to stop; what the reference's spectral functions need): both diagonals above the cut-off:
//     the squared cosine; one above, one below: the squared angle e^2 / big^2 plus the contamination of the dropped
//     direction, 0.01 e^2 / (big 1e-5) (it has to stay below the cut-off); both below: nothing (both are dropped).
//     Normalised by the number of kept diagonals.
//   LENIENT (judges the status when the sweep budget runs out): the same with "inside the rounding noise of a matrix
//     of this norm" (below `floor`) in the place of "dropped": cosines against noise diagonals never settle -- N < C
//     pixels at a feature scale whose noise exceeds 1e-5 -- and do not matter (the content has no energy there).
// partial[m][chunk][0..3] = strict sum (half the sum over the ordered pairs of the chunk's rows), kept diagonals,
// lenient sum, significant diagonals.  Fixed thread -> element map and reduction order: bit-reproducible, so the
// sweep count -- and with it every output bit -- does not depend on scheduling.
// mixed_w: weight of the kept-x-dropped couplings in the STRICT measure.  The second-order completion covers the block of
// kept eigenvalues only, so when the stop threshold is raised for it (4e-2 instead of 1.5e-2) the couplings across the
// cut-off keep their old bound: their squared measure is weighted by (4 / 1.5)^2.
// Round 4: the measurement walks 64 x 64 TILES of the upper triangle (the matrix is symmetric: an off-diagonal tile counts for
// its mirror image as well, half the bytes and half the arithmetic of the row-chunk walk it replaces; the two diagonal segments
// of a tile are 128 gathered values instead of the whole diagonal per block).  partial[m][tile][0..5] = strict kept-x-kept sum,
// strict kept-x-dropped sum (weighted in jacobi_check_kernel: the `near` flag needs the whole diagonal), kept diagonals, lenient
// sum, significant diagonals, near flag; jacobi_check_kernel (one wave per matrix) sums them over the tiles with a fixed lane ->
// tile map and a fixed tree.  (Letting the block that finishes a matrix last evaluate the test -- a counter and a device-scope
// fence per block -- saves the second launch and cost 2.5 ms per 32-pair step: the fence writes the XCD's L2 back, and the
// tiles the update has just written are still dirty in it.)
constexpr int JACOBI_RESID_T = 64;
constexpr int JACOBI_RESID_MAXTILES = 136;             // C <= 1024: 16 x 17 / 2
constexpr int JACOBI_RESID_STRIDE = 8;                 // floats per (matrix, tile)
// Round 6: the stop test also bounds the WORST ROW.  r2 is a mean over the rows of a row's sum of squared cosines; the completion's
// error in ONE eigen-direction is set by that direction's own row, and a mean over C rows hides a row C times above it -- graded
// spectra do that (the rows of the smallest eigenvalues settle last): C = 64, 72 pixels, eigenvalues 4.5e3 .. 3.5e-2 stopped at
// sweep 5 with the mean under the threshold and the transform 1.35e-3 off; one sweep later 4e-6 (wide fuzz run,
// profiles/r06_fuzz_wide.txt).  Row sums: every tile adds its 64 row and 64 column sums into rowsum[m][C] as 2^-20 fixed point
// with integer atomics (associative: the sums, and with them the sweep counts and every output bit, do not depend on the order),
// jacobi_check_kernel takes the maximum, clears the words, and a matrix is done only if max_p rowsum_p / 2 < JACOBI_ROW_K tol^2 too.
// (a contribution is capped at 32 = 2^25 words: at most 2 x 16 tiles add to a row, so a word cannot wrap)
constexpr float JACOBI_ROW_K = 8.f;
constexpr float JACOBI_ROW_FIX = 1048576.f;            // 2^20
struct JacobiCheckArgs {
  int mid;                   // 1: the test in the middle of a sweep (jacobi_check_mid)
  float tol_max, tol_fn;
  int buf, segs, lenient_from;
  float row_k;               // JACOBI_ROW_K
};

// done: 0 = still rotating, 1 = converged, 2 = failed (a non-finite element reached a pair problem).
// Converged = the sweep saw no rotated pair above tol_max (the classical test: the matrix was already diagonal to
// tol_max BEFORE the sweep), or -- tol_fn > 0 -- the residual measured after the sweep is below tol_fn: the matrix
// function built from this state with the first-order completion is then accurate to O(tol_fn^2).
// lenient_from: from this many completed sweeps on, a matrix whose SIGNIFICANT pairs were all below tol_max in the sweep
// is done as well (what jacobi_finalize_kernel accepts when the budget runs out): the noise-level pairs of a
// rank-deficient matrix never settle, and without this such a matrix always burns the whole sweep budget.
__device__ __forceinline__ void jacobi_check_end(JacobiState& s, const float (&v)[5], const JacobiCheckArgs& a) {
  s.sweeps += 1;
  const float r2 = v[0] / fmaxf(v[1], 1.f);
  const bool rows_ok = v[4] < a.row_k * a.tol_fn * a.tol_fn;
  s.r2 = r2;
  s.r2l = v[2] / fmaxf(v[3], 1.f);
  const unsigned bits = s.offmax;                       // max of non-negative floats as bit patterns; >= 0x7f800000: inf / NaN
  if (bits >= 0x7f800000u || !(r2 < 3.0e38f)) s.done = 2;
  else if (__uint_as_float(bits) < a.tol_max || (a.tol_fn > 0.f && r2 < a.tol_fn * a.tol_fn && rows_ok)) s.done = 1;
  else if (s.sweeps >= a.lenient_from && __uint_as_float(s.offsig) < a.tol_max) s.done = 1;
  if (s.done) { s.pad = a.buf; s.seg_stop = a.segs; }
  s.last_sig = s.offsig;
  s.floor = fmaxf(s.floor, JACOBI_SIG_FLOOR * __uint_as_float(s.dmax));
  s.offmax = 0u;
  s.offsig = 0u;
  s.dmax = 0u;
}
// The same residual test in the MIDDLE of a sweep (tol_fn callers only): near the end the residual halves every third
// of a sweep (tools/jacobi_block_order_proto.py), so a matrix that a full sweep would take 10x below the stop threshold
// is usually below it half a sweep earlier; its remaining launches of the sweep turn into no-ops.  Touches nothing but
// `done`, r2 / r2l and the sweep count (the half sweep counts as one).
__device__ __forceinline__ void jacobi_check_mid(JacobiState& s, const float (&v)[5], const JacobiCheckArgs& a) {
  const float r2 = v[0] / fmaxf(v[1], 1.f);
  if (s.offmax < 0x7f800000u && r2 < a.tol_fn * a.tol_fn && v[4] < a.row_k * a.tol_fn * a.tol_fn) {       // finite so far and converged
    s.r2 = r2;
    s.r2l = v[2] / fmaxf(v[3], 1.f);
    s.last_sig = s.offsig;
    s.sweeps += 1;
    s.done = 1;
    s.pad = a.buf;
    s.seg_stop = a.segs;
  }
}

// grid (tiles of the upper triangle, matrices)
__global__ __launch_bounds__(256) void jacobi_resid_kernel(const float* A, const JacobiState* st, float* partial, int C, unsigned* rowsum, float mixed_w) {
  constexpr int T = JACOBI_RESID_T;
  __shared__ float dr[T], dc[T], ir[T], ic[T];
  __shared__ float red[5][4];
  __shared__ float colred[4][T];
  const int m = blockIdx.y, tid = threadIdx.x;
  if (st[m].done) return;                                // (jacobi_check_kernel skips the matrix as well)
  const int ntr = (C + T - 1) / T;
  int ti = 0, t = blockIdx.x;
  while (t >= ntr - ti) { t -= ntr - ti; ++ti; }
  const int tj = ti + t;
  const bool diag = ti == tj;
  const float* Am = A + (size_t)m * C * C;
  const float floor_m = st[m].floor;
  if (tid < 2 * T) {
    const int i = (tid < T ? ti * T + tid : tj * T + tid - T);
    const float d = i < C ? fabsf(Am[(size_t)i * C + i]) : 0.f;
    (tid < T ? dr : dc)[tid & (T - 1)] = d;
    (tid < T ? ir : ic)[tid & (T - 1)] = d > 0.f ? 1.f / d : 0.f;
  }
  __syncthreads();
  // v: kept x kept, kept x dropped, kept diagonals, lenient, significant diagonals; near flag beside them
  float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int near = 0;
  if (diag && tid < T && ti * T + tid < C) {
    const float d = dr[tid];
    v[2] = d > 1e-5f ? 1.f : 0.f;
    v[4] = d > floor_m ? 1.f : 0.f;
    // an eigenvalue within half a decade of the cut-off: its kept / dropped side can still change, and a pair of the kept
    // block may really be a pair across the cut-off -- such a matrix keeps the old bound on ALL its couplings
    near = (d > 3.3e-6f) & (d < 3e-5f);
  }
  // an ordered pair (p, q) weighs 1/2: an off-diagonal tile stands for its mirror image too
  const float w = diag ? 0.5f : 1.f;
  const int c4 = (tid & 15) * 4, gq = tj * T + c4;
  float sr[4] = {0.f, 0.f, 0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f};     // this thread's part of its 4 rows' / 4 columns' strict sums
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = (tid >> 4) + 16 * k, gp = ti * T + r;
    if (gp < C && gq < C) {                              // (C is a multiple of 32: a group of four columns is inside or outside)
      const f32x4 e4 = *reinterpret_cast<const f32x4*>(Am + (size_t)gp * C + gq);
      const float dp = dr[r], ip = ir[r];
      const bool kp = dp > 1e-5f, sp = dp > floor_m;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dq = dc[c4 + j], iq = ic[c4 + j];
        const bool kq = dq > 1e-5f, sq = dq > floor_m;
        const bool bigp = dp >= dq;
        const float small = bigp ? dq : dp, ibig = bigp ? ip : iq;
        const float e2 = (diag && r == c4 + j) ? 0.f : w * e4[j] * e4[j];
        const float cos2 = e2 * ip * iq;
        const float mixed = e2 * ibig * (ibig + (small < 1e-5f ? 0.01f * 1e5f : 0.f));
        // Round 6: ACROSS the cut-off f jumps, and what the residual does there is rotate the kept direction into the dropped one by
        // e / (d_k - d_d), not e / d_k: with a cluster of eigenvalues around 1e-5 (spacing of a few per cent: 8 of a 128-channel
        // covariance within +-20 % in the wide fuzz run, profiles/r06_fuzz_wide.txt) the old measure let the sweeps stop at angles of
        // 0.2 .. 0.4 between neighbours on either side, 1.1e-3 .. 1.4e-2 of the transform.  The gap is floored at 1e-3 of the larger
        // diagonal (closer pairs float32 cannot tell apart: either side is the reference's).
        const float big = bigp ? dp : dq;
        const float igap = __builtin_amdgcn_rcpf(fmaxf(big - small, 1e-3f * big));
        const float across = e2 * (igap * igap + ibig * (small < 1e-5f ? 0.01f * 1e5f : 0.f));
        v[0] += (kp & kq) ? cos2 : 0.f;
        v[1] += (kp ^ kq) ? across : 0.f;
        const float se = (kp & kq) ? cos2 : ((kp ^ kq) ? mixed_w * across : 0.f);
        sr[k] += se;
        sc[j] += se;
        v[3] += (sp & sq) ? cos2 : ((sp | sq) ? mixed : 0.f);
      }
    }
  }
  const int near_any = __syncthreads_or(near);
  // row sums: the 16 lanes of a row group hold a row's 64 columns; column sums: 4 rows per thread, 4 row groups per wave, 4 waves.
  // (a diagonal tile weighs an ordered pair 1/2 and holds both orders: its row and column sums add up to the whole)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float x = sr[k];
    for (int o = 1; o < 16; o <<= 1) x += __shfl_xor(x, o, 64);
    const int gp = ti * T + (tid >> 4) + 16 * k;
    if ((tid & 15) == 0 && gp < C) atomicAdd(rowsum + (size_t)m * JACOBI_ROWSUM_MAX + gp, (unsigned)(fminf(x, 32.f) * JACOBI_ROW_FIX + 0.5f));
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float x = sc[j];
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    if ((tid & 63) < 16) colred[tid >> 6][c4 + j] = x;
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if ((tid & 63) == 0) red[j][tid >> 6] = v[j];
  }
  __syncthreads();
  if (tid < T && tj * T + tid < C) {
    const float x = (colred[0][tid] + colred[1][tid]) + (colred[2][tid] + colred[3][tid]);
    atomicAdd(rowsum + (size_t)m * JACOBI_ROWSUM_MAX + tj * T + tid, (unsigned)(fminf(x, 32.f) * JACOBI_ROW_FIX + 0.5f));
  }
  float* out = partial + ((size_t)m * JACOBI_RESID_MAXTILES + blockIdx.x) * JACOBI_RESID_STRIDE;
  if (tid < 5) out[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
  if (tid == 5) out[5] = near_any ? 1.f : 0.f;
}

// grid (matrices), one wave: the measurement's sums over the tiles, then the test (ck.mid: the one in the middle of a sweep)
__global__ __launch_bounds__(64) void jacobi_check_kernel(JacobiState* st, const float* partial, int ntile, float mixed_w, JacobiCheckArgs ck,
                                                          int* done_host /* this group's mapped host words, or null */, unsigned* rowsum, int C) {
  const int m = blockIdx.x, tid = threadIdx.x;
  if (st[m].done) { if (tid == 0 && done_host) done_host[m] = st[m].done; return; }
  unsigned rmax = 0u;                                   // the worst row's sum (fixed point), and the words cleared for the next measurement
  for (int p = tid; p < C; p += 64) {
    unsigned* w = rowsum + (size_t)m * JACOBI_ROWSUM_MAX + p;
    rmax = max(rmax, *w);
    *w = 0u;
  }
  for (int o = 32; o > 0; o >>= 1) rmax = max(rmax, (unsigned)__shfl_xor((int)rmax, o, 64));
  float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* pm = partial + (size_t)m * JACOBI_RESID_MAXTILES * JACOBI_RESID_STRIDE;
  for (int tt = tid; tt < ntile; tt += 64)
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] += pm[tt * JACOBI_RESID_STRIDE + j];
#pragma unroll
  for (int j = 0; j < 6; ++j)
    for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o, 64);
  if (tid == 0) {
    const bool near_m = a[5] > 0.f;
    // remembered for jacobi_finalize_kernel: such a matrix has only the first-order completion to pay for a late acceptance
    st[m].pad2 = near_m ? 1 : 0;
    const float vv[5] = {(near_m ? mixed_w : 1.f) * a[0] + mixed_w * a[1], a[2], a[3], a[4], 0.5f * (float)rmax * (1.f / JACOBI_ROW_FIX)};
    if (ck.mid) jacobi_check_mid(st[m], vv, ck); else jacobi_check_end(st[m], vv, ck);
    if (done_host) done_host[m] = st[m].done;
  }
}

// End of a solve.  A matrix still rotating after the last allowed sweep has FAILED only if its last sweep still saw a
// significant pair above the tolerance; noise-level pairs alone (numerical null space of a rank-deficient covariance:
// N < C pixels, dead or duplicated channels) never settle and do not matter.
// sweeps_out[m] = sweeps used if matrix m is good, -sweeps if it failed to converge, -1000 - sweeps for non-finite
// input; fail[0] += matrices not converged, fail[1] += non-finite ones.
// fail: this group's slot of the caller's status words (host memory mapped into the device, one slot per stream
// group so that plain read-modify-writes of one thread suffice), read by the caller after its next stream sync --
// a failed solve is never silently dropped.
// stats (or null): this group's slot of the caller's solver statistics (host memory mapped into the device):
// [0] matrices solved, [1] sum of their sweeps, [2] the largest sweep count -- wct_eig_stats reads and clears them
__global__ void jacobi_finalize_kernel(const JacobiState* st, int* sweeps_out, int nmat, float tol_max, float tol_fn, volatile int* fail,
                                       volatile int* stats = nullptr) {
  const int m = threadIdx.x;
  int d = m < nmat ? st[m].done : 1;
  // out of sweeps: good enough after all if the last sweep's significant pairs were below tol_max, or if the lenient
  // residual is within 4x of the target (second-order error 16x the target's: still inside the 1e-3 budget)
  // (second-order completion: error ~ r^3, and its stop threshold is already 4e-2 -- twice that is the most the 1e-3 budget takes)
  // -- except for a matrix with an eigenvalue near the cut-off (pad2, jacobi_resid_kernel): it keeps the first-order completion
  // and with it the first-order bound 4 x 1.5e-2
  const bool near_cut = m < nmat && st[m].pad2 != 0;
  const float tol_l = tol_fn > 0.f ? (tol_fn > 2e-2f ? (near_cut ? 4.f * 1.5e-2f : 2.f * tol_fn) : 4.f * tol_fn) : tol_max;
  if (d == 0 && (__uint_as_float(st[m].last_sig) < tol_max || (st[m].r2l >= 0.f && st[m].r2l < tol_l * tol_l))) d = 1;
  if (m < nmat && sweeps_out) sweeps_out[m] = d == 1 ? st[m].sweeps : (d == 2 ? -1000 - st[m].sweeps : -st[m].sweeps);
  const int n_open = __builtin_popcountll(__ballot(d == 0)), n_nan = __builtin_popcountll(__ballot(d == 2));
  if (m == 0 && fail) {
    if (n_open) fail[0] = fail[0] + n_open;
    if (n_nan) fail[1] = fail[1] + n_nan;
  }
  if (stats) {
    int sw = m < nmat ? st[m].sweeps : 0;                  // 0: a matrix that was never rotated (shared style)
    int cnt = sw > 0 ? 1 : 0, mx = sw;
    for (int o = 32; o > 0; o >>= 1) { sw += __shfl_xor(sw, o, 64); cnt += __shfl_xor(cnt, o, 64); mx = max(mx, __shfl_xor(mx, o, 64)); }
    if (m == 0) { stats[0] = stats[0] + cnt; stats[1] = stats[1] + sw; if (mx > stats[2]) stats[2] = mx; }
  }
}

constexpr int JACOBI_MAX_SWEEPS = 16;   // round 3: 12 -> 16 (graded rank-deficient 512-channel spectra used 10-12; a failure stays loud)
// WCT_JACOBI_MAX_SWEEPS (read at every solve): LOWERS the sweep budget so that the non-convergence path can be tested.  It
// cannot raise it: a larger budget moves `lenient_from` and with it the sweep counts -- the output bits -- of slowly
// converging matrices.
static int jacobi_max_sweeps() {
  const char* e = getenv("WCT_JACOBI_MAX_SWEEPS");
  const int n = e ? atoi(e) : JACOBI_MAX_SWEEPS;
  return n < 1 ? 1 : (n > JACOBI_MAX_SWEEPS ? JACOBI_MAX_SWEEPS : n);
}

size_t jacobi_workspace_bytes(int C, int nmat) {
  // per matrix: the rotation log of two launch segments (2 x C/B steps x C/M2 tiles x M2^2 = 4 C^2 floats for both block
  // widths) and the same again as fp16 hi/lo fragments, two generations of rotated pair problems (2 x C x M2 <= 128 C), the second matrix buffer (C^2); then state
  // words and residual partials
  return (size_t)nmat * ((size_t)9 * C * C + (size_t)128 * C) * sizeof(float) + 1024 +
         (size_t)nmat * (sizeof(JacobiState) + JACOBI_RESID_MAXTILES * JACOBI_RESID_STRIDE * sizeof(float) + JACOBI_ROWSUM_MAX * sizeof(unsigned));
}

// One solve: a batch of matrices on one stream.  (Until round 3 a batch could be split over up to four streams so that one
// part's latency-bound pair problems hid under another's tile update -- profiles/r02_eig_groups.txt; with the look-ahead
// launches a solve's pair problems run beside its own tile update, and more streams only split the chip: Jacobi ms per step
// with 1 / 2 / 4 groups, batch 32: 20.6 / 21.0 / 22.5, batch 8: 9.3 / 11.9 / 10.0.)
struct JacobiGroup {
  float* A; float* V; int nmat; float* Qbuf; JacobiState* st; float* resid; hipStream_t stream; int* sweeps_out;
  half_t* Qlog16[2];                         // the same rotation logs as fp16 hi/lo fragments (V <- V Q)
  float* Qlog[2]; float* Sb[2]; float* P[2]; // look-ahead path: rotation logs of two segments, rotated pair problems of two
                                             // consecutive steps, the two matrix buffers (P[0] = A)
  int cur, par, lg, segs;                    // buffer holding the matrices; generation of the last pair problems; log in use;
                                             // segments completed
  int* done_host = nullptr;                  // JacobiHost::flags_dev (jacobi_check_kernel), or null
  int u_f16 = 0;                             // tile updates on split fp16 (the batched transform path) or fp32 MFMA (wct_eigh, style-swap)
  int vstrip;                                // V is updated per segment by jacobi_vstrip_kernel on the side stream `vs`
  hipStream_t vs; hipEvent_t ev_seg, ev_v[2];// main -> side (segment enqueued), side -> main (log buffer free again)
  bool v_busy[2];
  WctSkip skip;                // position in a WCT batch (skip_style_mat); WCT_SKIP_NONE for a plain batch
  float tol_fn;                // > 0: also stop on the measured residual (callers that complete f(A) to first order)
  int* fail;                   // device view of the caller's failure words [2], or null
  int* stats;                  // device view of the caller's statistics slot [3] for matrices of this size class, or null
  int check_from = 2;          // the host reads the done-flags after sweep check_from and every later one.  2: matrices solved from
                               // the identity are never done earlier; a warm solve (launch_eig_stage) sets 0
};

// per host thread (= per ctx user) and device: pinned copies of the convergence flags, the event behind them, and the V pass's
// stream and events (events belong to the device that was current when they were created: one set per device, so that a thread
// driving contexts on several GPUs never records an event of GPU 0 on a stream of GPU 1 -- ADVICE r2)
// flags: the `done` words of the solve's matrices, host memory MAPPED into the device ([64]): jacobi_check_kernel stores them
// there itself, and the host reads them after the sweep's event -- up to round 5 a device-to-host copy of the JacobiState array
// per sweep carried them (45 copy kernels of ~5 us per step in the solver's launch trains, at every batch size)
// (the V-pass stream has the default priority: the lowest or the highest made the eigensolver 12.2 -> 22 ms per 32-pair step --
//  profiles/r05_vprio.txt)
struct JacobiHost { int* flags; int* flags_dev; hipEvent_t ev; hipStream_t vs; hipEvent_t ev_seg, ev_v[2]; };
static JacobiHost* jacobi_host() {
  constexpr int MAXDEV = 16;
  static thread_local JacobiHost hs[MAXDEV] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
  JacobiHost& h = hs[dev];
  if (!h.flags) {
    if (hipHostMalloc((void**)&h.flags, 64 * sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h.flags_dev, h.flags, 0) != hipSuccess) { h.flags = nullptr; return nullptr; }
    const bool ok = hipEventCreateWithFlags(&h.ev, hipEventDisableTiming) == hipSuccess &&
                    hipStreamCreateWithFlags(&h.vs, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&h.ev_seg, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&h.ev_v[0], hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&h.ev_v[1], hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipHostFree(h.flags); h.flags = nullptr; return nullptr; }
  }
  return &h;
}

// ---- look-ahead orchestration -------------------------------------------------------------------------------------
// launch { D(step_d) writing log slot step_d - seg_begin, U(step_u) reading slot step_u - seg_begin }
template <int M2>
static void jacobi_fused_launch(JacobiGroup& G, int C, int seg_begin, bool has_d, int step_d, bool has_u, int step_u, bool first) {
  constexpr int B = M2 / 2;
  const int npair = C / B / 2;
  const int ntask = npair * (npair - 1) / 2 + npair + (G.vstrip ? 0 : npair * npair);
  const size_t slot = (size_t)G.nmat * npair * M2 * M2;
  JacobiFusedArgs a;
  a.Pr = G.P[G.cur]; a.Pw = G.P[G.cur ^ 1]; a.V = G.V;
  a.Qr = G.Qlog[G.lg] + (size_t)(step_u - seg_begin) * slot; a.Qw = G.Qlog[G.lg] + (size_t)(step_d - seg_begin) * slot;
  a.Qr16 = G.Qlog16[G.lg] + (size_t)(step_u - seg_begin) * slot * 2; a.Qw16 = G.Qlog16[G.lg] + (size_t)(step_d - seg_begin) * slot * 2;
  a.Sr = G.Sb[G.par]; a.Sw = G.Sb[G.par ^ 1];
  a.st = G.st; a.C = C; a.nmat = G.nmat; a.step_d = step_d; a.step_u = step_u;
  a.has_d = has_d; a.has_u = has_u; a.first = first; a.with_v = !G.vstrip; a.u_f16 = G.u_f16;
  const unsigned grid = (has_d ? G.nmat * npair : 0) + (has_u ? G.nmat * ntask : 0);
  // M2 = 64: pair problems resident in registers, strips over 4 waves (jacobi_pair64.h; against an 8-wave layout and the LDS
  // images of the 32-wide kernel at this width, eigensolver ms per step at batch 32 / 8 / 1: 14.4 / 7.6 / 6.0 vs 16.2 / 7.7 / 6.1
  // and 17.1 / 8.0 / 6.4 -- profiles/r04_jacobi_ab.txt); the 32-wide block pairs keep the LDS images
  if constexpr (M2 == 64) {
    hipLaunchKernelGGL(jacobi_fused4_kernel, dim3(grid), dim3(pair64::NT), pair64::lds_bytes(has_d, has_u, first, step_d), G.stream, a);
    LAUNCH_NOTE("jacobi_fused4_kernel");
  } else {
    hipLaunchKernelGGL(jacobi_fused_kernel, dim3(grid), dim3(pair32::NT), pair32::lds_bytes(has_d, has_u, first, step_d), G.stream, a);
    LAUNCH_NOTE("jacobi_fused_kernel");
  }
  if (has_d) G.par ^= 1;
  if (has_u) G.cur ^= 1;
}

// V pass of a segment: the 64-wide block pairs of C = 256 and 512, the block counts jacobi_vstrip_kernel is instantiated for
static void vstrip_launch(const JacobiGroup& G, int C, int step_begin, int step_end, hipStream_t s) {
  const int nblk = C / 32;
  VStripArgs a;
  a.V = G.V; a.Qlog = G.Qlog16[G.lg]; a.st = G.st; a.C = C; a.nmat = G.nmat; a.step_begin = step_begin; a.step_end = step_end; a.seg = G.segs;
  // Round 5: blocks are handed to the 8 XCDs round-robin by their linear index.  All the row strips of a matrix stream the SAME
  // rotation log (1 MB per 512-channel matrix and segment); with the strip index running fastest they sat on 8 different XCDs
  // and every one of the 8 L2s fetched every log from HBM.  With the MATRIX index running fastest (and a multiple of 8 matrices)
  // the strips of matrix m all run on XCD m % 8 and share its L2.
  a.mat_major = G.nmat % 8 == 0;
  constexpr int W = VS_WAVES;
#define VSTRIP_CASE(nb) \
  if (nblk == nb) {                                                                                                  \
    /* the ring is above the 64 KiB a kernel gets unasked (every launch: cheap, idempotent, no per-device flag to race on; a  \
       refusal is reported here) */                                                                                  \
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&jacobi_vstrip_kernel<nb>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)VS_LDS_BYTES) != hipSuccess) \
      LAUNCH_NOTE("jacobi_vstrip_kernel (hipFuncSetAttribute: dynamic LDS above 64 KiB)");                            \
    hipLaunchKernelGGL(jacobi_vstrip_kernel<nb>, a.mat_major ? dim3(G.nmat, C / 16 / W) : dim3(C / 16 / W, G.nmat), dim3(W * 64), VS_LDS_BYTES, s, a); \
    LAUNCH_NOTE("jacobi_vstrip_kernel");                                                                             \
  }
  VSTRIP_CASE(16) VSTRIP_CASE(8)
#undef VSTRIP_CASE
}

// before the first launch of a segment: its log buffer must not be in use by a V pass any more
static int jacobi_segment_begin(JacobiGroup& G) {
  if (G.vstrip && G.v_busy[G.lg]) { HIP_TRY(hipStreamWaitEvent(G.stream, G.ev_v[G.lg], 0)); G.v_busy[G.lg] = false; }
  return WCT_OK;
}
// after the last launch of a segment (steps [step_begin, step_end)): hand its log to the V pass, switch logs
static int jacobi_segment_end(JacobiGroup& G, int C, int step_begin, int step_end) {
  if (G.vstrip) {
    HIP_TRY(hipEventRecord(G.ev_seg, G.stream));
    HIP_TRY(hipStreamWaitEvent(G.vs, G.ev_seg, 0));
    vstrip_launch(G, C, step_begin, step_end, G.vs);
    HIP_TRY(hipEventRecord(G.ev_v[G.lg], G.vs));
    G.v_busy[G.lg] = true;
    G.lg ^= 1;
  }
  G.segs += 1;
  return WCT_OK;
}

// steps [step_begin, step_end) of one sweep as look-ahead launches: D(begin) | {D(s), U(s-1)} ... | U(end-1); afterwards
// the matrices are complete in P[cur].  [lo, hi) restricts the launches that are enqueued by this call to those of index
// lo..hi-1 (index = step of the D part; hi = step_end is the closing U).
template <int M2>
static void jacobi_enqueue_segment(JacobiGroup& G, int C, int step_begin, int step_end, int lo, int hi) {
  for (int step = lo; step < hi; ++step)
    jacobi_fused_launch<M2>(G, C, step_begin, step < step_end, step, step > step_begin, step - 1, step == step_begin);
}

// residual measurement of the matrices (in P[cur]), then the test `ck`
static void jacobi_measure(JacobiGroup& G, int C, const JacobiCheckArgs& ck) {
  const int ntr = (C + JACOBI_RESID_T - 1) / JACOBI_RESID_T;
  const int ntile = ntr * (ntr + 1) / 2;
  const float mixed_w = G.tol_fn > 2e-2f ? 7.1f : 1.f;
  unsigned* rowsum = reinterpret_cast<unsigned*>(G.resid + (size_t)G.nmat * JACOBI_RESID_MAXTILES * JACOBI_RESID_STRIDE);
  hipLaunchKernelGGL(jacobi_resid_kernel, dim3(ntile, G.nmat), dim3(256), 0, G.stream, G.P[G.cur], G.st, G.resid, C, rowsum, mixed_w);
  hipLaunchKernelGGL(jacobi_check_kernel, dim3(G.nmat), dim3(64), 0, G.stream, G.st, G.resid, ntile, mixed_w, ck, G.done_host, rowsum, C);
  LAUNCH_NOTE("jacobi_resid_kernel / jacobi_check_kernel");
}

constexpr int JACOBI_MID_FROM = 3;     // from this sweep on, a solve of 8 or more blocks with tol_fn > 0 also tests half-way through
constexpr int JACOBI_VSTRIP_MIN = 24;  // the V pass (jacobi_vstrip_kernel) takes V out of the tile update from this many matrices on

template <int M2>
static int jacobi_run_fused(JacobiGroup& G, int C) {
  constexpr int B = M2 / 2;
  const int nblk = C / B;
  const int half = -1 + nblk / 2;                 // steps [-1, half) | [half, nblk - 1)
  const int max_sweeps = jacobi_max_sweeps();
  const bool mid_test = nblk >= 8 && G.tol_fn > 0.f;
  JacobiHost* host = jacobi_host();
  G.cur = 0; G.par = 0; G.lg = 0; G.segs = 0; G.v_busy[0] = G.v_busy[1] = false;
  // V in registers, per segment: C = 256 and 512 (64-wide block pairs; the V pass is not instantiated for others)
  G.vstrip = host && M2 == 64 && (nblk == 8 || nblk == 16) && G.nmat >= JACOBI_VSTRIP_MIN;
  if (G.vstrip) { G.vs = host->vs; G.ev_seg = host->ev_seg; G.ev_v[0] = host->ev_v[0]; G.ev_v[1] = host->ev_v[1]; }
  G.done_host = host ? host->flags_dev : nullptr;
  hipLaunchKernelGGL(jacobi_init_kernel, dim3(64, G.nmat), dim3(256), 0, G.stream, G.A, G.V, G.st, C, 0, (int)G.skip,
                     reinterpret_cast<unsigned*>(G.resid + (size_t)G.nmat * JACOBI_RESID_MAXTILES * JACOBI_RESID_STRIDE));
  HIP_TRY(hipGetLastError());
  bool pending = false;
  int rc;
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    const bool mid = mid_test && sweep >= JACOBI_MID_FROM;
    // segments of this sweep: [-1, half) + [half, nblk - 1) around a residual test, or the whole sweep in one
    const int end1 = mid ? half : nblk - 1;
    if ((rc = jacobi_segment_begin(G))) return rc;
    // the flags of the previous sweep are looked at once half a sweep of launches is enqueued (the GPU never idles)
    jacobi_enqueue_segment<M2>(G, C, -1, end1, -1, half);
    if (pending) {
      HIP_TRY(hipEventSynchronize(host->ev));
      bool all = true;
      for (int m = 0; m < G.nmat; ++m) all = all && host->flags[m] != 0;
      pending = false;
      if (all) break;          // every matrix was done before this sweep began: its launches were no-ops
    }
    jacobi_enqueue_segment<M2>(G, C, -1, end1, half, end1 + 1);
    if ((rc = jacobi_segment_end(G, C, -1, end1))) return rc;
    if (mid) {
      jacobi_measure(G, C, JacobiCheckArgs{1, JACOBI_CONV_TOL, G.tol_fn, G.cur, G.segs, 1 << 30, JACOBI_ROW_K});
      if ((rc = jacobi_segment_begin(G))) return rc;
      jacobi_enqueue_segment<M2>(G, C, half, nblk - 1, half, nblk);
      if ((rc = jacobi_segment_end(G, C, half, nblk - 1))) return rc;
    }
    jacobi_measure(G, C, JacobiCheckArgs{0, JACOBI_CONV_TOL, G.tol_fn, G.cur, G.segs, max_sweeps - 3, JACOBI_ROW_K});
    if (host && sweep >= G.check_from && sweep + 1 < max_sweeps) {
      HIP_TRY(hipEventRecord(host->ev, G.stream));      // (behind the sweep's jacobi_check_kernel, which stored the flags)
      pending = true;
    }
  }
  for (int l = 0; l < 2; ++l)            // the V passes still in flight belong to this solve
    if (G.vstrip && G.v_busy[l]) { HIP_TRY(hipStreamWaitEvent(G.stream, G.ev_v[l], 0)); G.v_busy[l] = false; }
  hipLaunchKernelGGL(jacobi_gather_kernel, dim3(32, G.nmat), dim3(256), 0, G.stream, G.A, G.P[1], G.st, C, G.cur);
  HIP_TRY(hipGetLastError());
  if (G.sweeps_out || G.fail || G.stats) {
    hipLaunchKernelGGL(jacobi_finalize_kernel, dim3(1), dim3(64), 0, G.stream, G.st, G.sweeps_out, G.nmat, JACOBI_CONV_TOL, G.tol_fn, G.fail, G.stats);
    HIP_TRY(hipGetLastError());
  }
  return WCT_OK;
}

// statistics slot for matrices of order C inside the caller's status words: after the 2 failure words come [6 size classes][3]
// counters (size class = log2(C / 32), capped)
static int* jacobi_stats_slot(int* eig_fail, int C) {
  if (!eig_fail) return nullptr;
  int cls = 0;
  for (int c = C / 32; c > 1 && cls < 5; c >>= 1) ++cls;
  return eig_fail + 2 + cls * 3;
}

static int jacobi_make_group(JacobiGroup* G, float* A, float* V, int C, int nmat, void* workspace, size_t workspace_bytes,
                             int* sweeps_out, int* eig_fail, hipStream_t s) {
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 1024 && nmat >= 1 && nmat <= 64);
  ARG_CHECK(workspace_bytes >= jacobi_workspace_bytes(C, nmat));
  const size_t cc = (size_t)C * C;
  const size_t qbytes = (size_t)nmat * (9 * cc + (size_t)128 * C) * sizeof(float);
  G->A = A; G->V = V; G->nmat = nmat; G->Qbuf = reinterpret_cast<float*>(workspace);
  G->Qlog[0] = G->Qbuf; G->Qlog[1] = G->Qbuf + 2 * cc * nmat;
  G->Sb[0] = G->Qbuf + 4 * cc * nmat; G->Sb[1] = G->Sb[0] + (size_t)64 * C * nmat;
  G->P[0] = A; G->P[1] = G->Sb[1] + (size_t)64 * C * nmat; G->cur = 0; G->par = 0; G->lg = 0; G->segs = 0;
  G->Qlog16[0] = reinterpret_cast<half_t*>(G->P[1] + cc * nmat); G->Qlog16[1] = G->Qlog16[0] + 4 * cc * nmat;
  G->vstrip = 0; G->vs = nullptr; G->v_busy[0] = G->v_busy[1] = false;
  G->st = reinterpret_cast<JacobiState*>(reinterpret_cast<char*>(workspace) + ((qbytes + 255) / 256) * 256);
  G->resid = reinterpret_cast<float*>(reinterpret_cast<char*>(G->st) + (((size_t)nmat * sizeof(JacobiState) + 255) / 256) * 256);
  G->tol_fn = 0.f;
  G->stream = s; G->sweeps_out = sweeps_out; G->fail = eig_fail; G->stats = jacobi_stats_slot(eig_fail, C);
  G->skip = WCT_SKIP_NONE;
  return WCT_OK;
}

// measured (16 matrices): 64-wide pairs win from C = 256 up (half the tile traffic), 32-wide below
static bool jacobi_wide_pairs(int C) { return C % 64 == 0 && C >= 256; }

static int jacobi_dispatch(JacobiGroup& G, int C) {
  const bool m64 = jacobi_wide_pairs(C);
  const int rc = m64 ? jacobi_run_fused<64>(G, C) : jacobi_run_fused<32>(G, C);
  const int noted = launch_rc_take();  // a launch one of the train's void helpers saw refused (named there); cleared on every exit
  return rc ? rc : noted;
}

// Eigenpair j of a plain solve is the one that grew out of coordinate j.  The 32-wide path keeps that by construction; on the
// 64-wide path every sweep's intra step (pair64::intra_wave: odd-even transposition WITH EXCHANGE) leaves the 32 columns of each
// block in reverse order, so after an odd number of sweeps column b * 32 + j of V (and diagonal entry b * 32 + j of A) belongs to
// coordinate b * 32 + 31 - j -- a matrix that was diagonal to begin with came back with a permutation for V.  This puts the
// columns and the eigenvalues back (a pure exchange: no value changes; only the diagonal of A is an output, its off-diagonal
// residue is left).  Per matrix, from its own sweep count alone.  The transform's solves (launch_eig_stage) build V f(D) V^T,
// which has no order, and keep theirs.  grid (C / 32 column blocks, C / 16 row groups, matrices), 16 x 16 threads.
__global__ __launch_bounds__(256) void jacobi_unexchange_kernel(float* A, float* V, const JacobiState* st, int C) {
  const int m = blockIdx.z;
  if (!(st[m].sweeps & 1)) return;
  const size_t cc = (size_t)C * C;
  const int j = threadIdx.x & 15, lo = blockIdx.x * 32 + j, hi = blockIdx.x * 32 + 31 - j;
  float* row = V + m * cc + (size_t)(blockIdx.y * 16 + (threadIdx.x >> 4)) * C;
  const float a = row[lo], b = row[hi];
  row[lo] = b; row[hi] = a;
  if (blockIdx.y == 0 && threadIdx.x < 16) {
    float* Am = A + m * cc;
    const float da = Am[(size_t)lo * C + lo], db = Am[(size_t)hi * C + hi];
    Am[(size_t)lo * C + lo] = db; Am[(size_t)hi * C + hi] = da;
  }
}

int launch_jacobi_eigh(float* A, float* V, int C, int nmat, void* workspace, size_t workspace_bytes,
                       int* sweeps_done_dev, int* eig_fail, hipStream_t s) {
  JacobiGroup G;
  int rc = jacobi_make_group(&G, A, V, C, nmat, workspace, workspace_bytes, sweeps_done_dev, eig_fail, s);
  if (rc) return rc;
  if ((rc = jacobi_dispatch(G, C))) return rc;
  if (jacobi_wide_pairs(C)) {
    hipLaunchKernelGGL(jacobi_unexchange_kernel, dim3(C / 32, C / 16, nmat), dim3(256), 0, s, A, V, G.st, C);
    HIP_TRY(hipGetLastError());
  }
  return WCT_OK;
}

// the eigensolve stage of a transform: the 2P matrices of w in one batched solve, minus those the skip mode drops
int launch_eig_stage(const WctCarve& w, int C, int P, WctSkip skip, int u_f16, int* sweeps_dev, int* eig_fail, hipStream_t s, int check_from) {
  JacobiGroup G;
  int rc;
  if ((rc = jacobi_make_group(&G, w.A, w.V, C, 2 * P, w.jacobi_ws, w.jacobi_bytes, sweeps_dev, eig_fail, s))) return rc;
  G.skip = skip; G.tol_fn = JACOBI_TOL_FN_WCT; G.u_f16 = u_f16; G.check_from = check_from;
  return jacobi_dispatch(G, C);
}
