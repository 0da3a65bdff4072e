// Spatial control: the label partition of a level, and the masked transforms on the slot plan of wct.hip.
#include "wct_stages.h"
#include <algorithm>
#include <type_traits>

// ---------------------------------------------------------------------------
// Spatial control (Li et al. 2017, sec. 4.2 and Fig. 7): a label map splits the content into K regions, and region k is
// transformed with style k alone -- out[rows of k] = T(content[rows of k], style k, alpha) with region k's own mean, covariance
// (1 / (N_k - 1)) and cut-off.  The rows of a level are partitioned by label, stably (perm lists the rows of label 0 in pixel
// order, then those of label 1, ...; label k starts at seg_off[k]), and gathered into one [N][C] buffer.  Every label with
// N_k >= 2 rows is one (content, style) pair of the slot layout: pair p = the p-th such label, slot 2p its gathered rows, slot
// 2p + 1 its style, each with the slab / K-slice layout launch_wct gives (N_k, Ns_k).  The batched solver's results do not
// depend on the batch, so region k comes out bit for bit as launch_wct(rows of k, style k).  The apply reads the gathered
// rows and scatters them back to pixel order (apply_f16x2_kernel<ApplySegArgs>); the rows of a label with a single pixel are
// copied through unchanged (N_k - 1 = 0: no covariance).
// ---------------------------------------------------------------------------
// A batch of G frames (one label map each, g.mask [G][Hm][Wm]) is partitioned frame by frame in the same launches: the frame
// is a grid axis, and counts / blk_off [G][nblk][WCT_MIX_MAX], seg_off [G][WCT_MIX_MAX + 1], perm [G][N] are per frame, so the
// partition of a frame is the one it gets alone.
constexpr int MASK_ROWS = 2048;                  // rows per block of the two compaction passes (8 per thread)
constexpr int SEG_STRIDE = WCT_MIX_MAX + 1;      // seg_off words per frame

__device__ __forceinline__ int mask_label(const MaskGeom& g, int r) {
  const int i = r / g.w, j = r - i * g.w;
  return g.mask[(size_t)min(i * g.stride, g.Hm - 1) * g.Wm + min(j * g.stride, g.Wm - 1)];
}

// pass 1: counts[b][k] = rows of label k in block b's MASK_ROWS rows (wave64 ballots; no atomics, so the order is fixed)
__global__ __launch_bounds__(256) void mask_count_kernel(MaskGeom g, int N, int K, int* counts) {
  __shared__ int wc[4][WCT_MIX_MAX];
  g.mask += (size_t)blockIdx.y * g.Hm * g.Wm;    // frame blockIdx.y
  counts += (size_t)blockIdx.y * gridDim.x * WCT_MIX_MAX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt[WCT_MIX_MAX];
#pragma unroll
  for (int k = 0; k < WCT_MIX_MAX; ++k) cnt[k] = 0;
  const int base = blockIdx.x * MASK_ROWS;
  for (int it = 0; it < MASK_ROWS / 256; ++it) {
    const int r = base + it * 256 + threadIdx.x;
    const int lab = r < N ? mask_label(g, r) : -1;
#pragma unroll
    for (int k = 0; k < WCT_MIX_MAX; ++k)
      if (k < K) cnt[k] += __popcll(__ballot(lab == k));
  }
  if (lane == 0)
    for (int k = 0; k < K; ++k) wc[wave][k] = cnt[k];
  __syncthreads();
  const int k = threadIdx.x;
  if (k < K) counts[blockIdx.x * WCT_MIX_MAX + k] = wc[0][k] + wc[1][k] + wc[2][k] + wc[3][k];
}

// pass 2 (one block per frame): blk_off[b][k] = where block b's rows of label k start in perm; seg_off[k] = where label k starts
__global__ __launch_bounds__(256) void mask_scan_kernel(const int* counts, int nblk, int K, int* blk_off, int* seg_off) {
  __shared__ int part[256];
  __shared__ int start;
  const int t = threadIdx.x;
  counts += (size_t)blockIdx.x * nblk * WCT_MIX_MAX;
  blk_off += (size_t)blockIdx.x * nblk * WCT_MIX_MAX;
  seg_off += blockIdx.x * SEG_STRIDE;
  const int per = (nblk + 255) / 256, b0 = min(t * per, nblk), b1 = min(b0 + per, nblk);
  if (t == 0) start = 0;
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += counts[b * WCT_MIX_MAX + k];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {          // inclusive scan over the 256 block ranges
      const int v = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    int run = start + part[t] - sum;
    for (int b = b0; b < b1; ++b) {
      blk_off[b * WCT_MIX_MAX + k] = run;
      run += counts[b * WCT_MIX_MAX + k];
    }
    __syncthreads();
    if (t == 0) { seg_off[k] = start; start += part[255]; }
    __syncthreads();
  }
  if (t == 0) seg_off[K] = start;
}

// pass 3: perm[blk_off[b][k] + rank] = r, rank = the row's place among block b's rows of its label (row order: iteration,
// wave, lane -- a stable partition)
__global__ __launch_bounds__(256) void mask_rank_kernel(MaskGeom g, int N, int K, const int* blk_off, int* perm) {
  __shared__ int off[WCT_MIX_MAX];
  __shared__ int wc[4][WCT_MIX_MAX];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  g.mask += (size_t)blockIdx.y * g.Hm * g.Wm;    // frame blockIdx.y
  blk_off += (size_t)blockIdx.y * gridDim.x * WCT_MIX_MAX;
  perm += (size_t)blockIdx.y * N;
  if (t < K) off[t] = blk_off[blockIdx.x * WCT_MIX_MAX + t];
  const unsigned long long below = (1ull << lane) - 1ull;
  const int base = blockIdx.x * MASK_ROWS;
  for (int it = 0; it < MASK_ROWS / 256; ++it) {
    const int r = base + it * 256 + t;
    const int lab = r < N ? mask_label(g, r) : -1;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < WCT_MIX_MAX; ++k)
      if (k < K) {
        const unsigned long long b = __ballot(lab == k);
        if (lab == k) mine = b;
        if (lane == 0) wc[wave][k] = __popcll(b);
      }
    __syncthreads();
    if (lab >= 0 && lab < K) {
      int pos = off[lab] + __popcll(mine & below);
      for (int v = 0; v < wave; ++v) pos += wc[v][lab];
      perm[pos] = r;
    }
    __syncthreads();
    if (t < K) off[t] += wc[0][t] + wc[1][t] + wc[2][t] + wc[3][t];
    __syncthreads();
  }
}

// xg[r] = x[perm[r]] for the rows of the K segments, 16-B accesses; frame blockIdx.y of N rows
__global__ __launch_bounds__(256) void mask_gather_kernel(const float* x, const int* perm, const int* seg_off, int K, int C, int N, float* xg) {
  const int cq = C / 4;
  x += (size_t)blockIdx.y * N * C; xg += (size_t)blockIdx.y * N * C;
  perm += (size_t)blockIdx.y * N; seg_off += blockIdx.y * SEG_STRIDE;
  const size_t n4 = (size_t)seg_off[K] * cq;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cq), c = (int)(i % cq) * 4;
    *reinterpret_cast<f32x4*>(xg + (size_t)r * C + c) = *reinterpret_cast<const f32x4*>(x + (size_t)perm[r] * C + c);
  }
}

// xg[r] = x[perm[seg_off[k] + r]] for the rows of segment k ALONE, packed from row 0 of xg (a style region: n_k * C floats move,
// not the whole map), 16-B accesses
__global__ __launch_bounds__(256) void mask_gather_segment_kernel(const float* x, const int* perm, const int* seg_off, int k, int C, float* xg) {
  const int cq = C / 4;
  const int r0 = seg_off[k];
  const size_t n4 = (size_t)(seg_off[k + 1] - r0) * cq;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cq), c = (int)(i % cq) * 4;
    *reinterpret_cast<f32x4*>(xg + (size_t)r * C + c) = *reinterpret_cast<const f32x4*>(x + (size_t)perm[r0 + r] * C + c);
  }
}

// the rows of the labels in `labs` (byte f, bit k: label k of frame f, a single pixel) pass through unchanged: x[perm[r]] -> out16 /
// out32 row perm[r] of the frame
struct SingleLabels { unsigned char frame[WCT_PLAN_PAIRS]; };
__global__ __launch_bounds__(256) void mask_passthrough_kernel(const float* x, const int* seg_off, const int* perm, SingleLabels labs,
                                                               int C, int N, half_t* out16, float* out32) {
  const int k = blockIdx.x, f = blockIdx.y;
  if (!((labs.frame[f] >> k) & 1u)) return;
  seg_off += f * SEG_STRIDE; perm += (size_t)f * N;
  for (int r = seg_off[k]; r < seg_off[k + 1]; ++r) {
    const size_t row = ((size_t)f * N + perm[r]) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float v = x[row + c];
      if (out32) out32[row + c] = v;
      if (out16) out16[row + c] = (half_t)v;
    }
  }
}

static int mask_nblk(int N) { return cdiv(N, MASK_ROWS); }

size_t mask_compact_workspace_bytes(int N, int G) { return 2 * align_up((size_t)G * mask_nblk(N) * WCT_MIX_MAX * sizeof(int)); }

int launch_mask_compact_batch(const MaskGeom& g, int N, int K, int G, int* perm, int* seg_off, void* workspace, hipStream_t s) {
  ARG_CHECK(g.mask && g.Hm >= 1 && g.Wm >= 1 && g.w >= 1 && g.stride >= 1 && N >= 1 && K >= 1 && K <= WCT_MIX_MAX && perm && seg_off);
  ARG_CHECK(G >= 1 && G <= WCT_PLAN_PAIRS);
  const int nblk = mask_nblk(N);
  int* counts = (int*)workspace;
  int* blk_off = (int*)((char*)workspace + align_up((size_t)G * nblk * WCT_MIX_MAX * sizeof(int)));
  hipLaunchKernelGGL(mask_count_kernel, dim3(nblk, G), dim3(256), 0, s, g, N, K, counts);
  hipLaunchKernelGGL(mask_scan_kernel, dim3(G), dim3(256), 0, s, (const int*)counts, nblk, K, blk_off, seg_off);
  hipLaunchKernelGGL(mask_rank_kernel, dim3(nblk, G), dim3(256), 0, s, g, N, K, (const int*)blk_off, perm);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_mask_compact(const MaskGeom& g, int N, int K, int* perm, int* seg_off, void* workspace, hipStream_t s) {
  return launch_mask_compact_batch(g, N, K, 1, perm, seg_off, workspace, s);
}

// A style region: the nk rows of label k of x [N][C] (perm / seg_off: a compaction of the map with K > k labels) into xg [nk][C],
// in pixel order.  nk is the caller's host count (it sizes the grid; the kernel reads the segment's bounds from seg_off).
int launch_mask_gather_segment(const float* x, const int* perm, const int* seg_off, int k, int nk, int C, float* xg, hipStream_t s) {
  ARG_CHECK(x && perm && seg_off && xg && k >= 0 && k < WCT_MIX_MAX && nk >= 1 && C >= 4 && C % 4 == 0);
  hipLaunchKernelGGL(mask_gather_segment_kernel, dim3(rows_grid(nk, C)), dim3(256), 0, s, x, perm, seg_off, k, C, xg);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// The slot plan of a masked level: pair p = the p-th label with nk >= 2 rows, slot 2p its rows of the gathered buffer, slot
// 2p + 1 its style, both with the layout of the single pair (nk[k], Ns[k]).  C as in mix_plan; styles may be null (the
// workspace size alone).  False for arguments no masked transform takes.
struct MaskPlan : SlotPlan {
  int lab[WCT_MIX_MAX], nmax;                    // the label of pair p; the most rows of a pair
  SingleLabels single; bool any_single;          // frame 0, bit k: label k has 1 row
  float* xg; int *perm, *seg_off; void* compact_ws;
};

// what a masked plan of G frames lays out behind its transform workspace: the gathered rows, the partition, the compaction's scratch
template <typename Plan>
static void mask_carve(Plan* m, void* base, int Cw, int Nc, int G) {
  plan_carve(m, base, Cw);
  size_t off = m->total;
  char* b = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) { void* q = b ? b + off : nullptr; off += align_up(bytes); return q; };
  m->xg = (float*)take((size_t)G * Nc * Cw * sizeof(float));
  m->perm = (int*)take((size_t)G * Nc * sizeof(int));
  m->seg_off = (int*)take((size_t)G * SEG_STRIDE * sizeof(int));
  m->compact_ws = take(mask_compact_workspace_bytes(Nc, G));
  m->total = off;
}

static bool mask_plan(MaskPlan* m, void* base, int C, int Nc, const int* nk, const float* const* styles, const int* Ns, int K,
                      int nmin) {
  if (!nk || !Ns || K < 1 || K > WCT_MIX_MAX || Nc < 1) return false;
  long long sum = 0;
  for (int k = 0; k < K; ++k) {
    if (nk[k] < 0 || (nk[k] >= 2 && ((styles && !styles[k]) || Ns[k] < nmin))) return false;
    sum += nk[k];
  }
  if (sum != Nc) return false;                   // every row has a label < K (the caller counted them)
  const int Cw = std::max(C, 32);
  *m = MaskPlan{};
  int row0[WCT_MIX_MAX], row = 0;                // where label k starts (host counts)
  for (int k = 0; k < K; ++k) {
    row0[k] = row;
    row += nk[k];
    if (nk[k] == 1) { m->single.frame[0] |= (unsigned char)(1u << k); m->any_single = true; }
    if (nk[k] < 2) continue;
    const int p = m->P++;
    m->lab[p] = k;
    m->nmax = std::max(m->nmax, nk[k]);
    const PairLayout lay = pair_layout(Cw, nk[k], Ns[k]);
    m->slot[2 * p] = {nullptr, nk[k], lay};
    m->slot[2 * p + 1] = {styles ? styles[k] : nullptr, Ns[k], lay};
  }
  m->nwhite = m->P;
  mask_carve(m, base, Cw, Nc, 1);
  if (m->xg)
    for (int p = 0; p < m->P; ++p) m->slot[2 * p].x = m->xg + (size_t)row0[m->lab[p]] * C;
  return true;
}

size_t wct_masked_workspace_bytes(int C, int Nc, const int* nk, const int* Ns, int K) {
  MaskPlan m;
  return mask_plan(&m, nullptr, C, Nc, nk, nullptr, Ns, K, 1) ? m.total : 0;
}

// compaction and gather of the G frames of a masked level (the first stage of every masked transform)
template <typename Plan>
static int launch_mask_gather(const float* content, const MaskGeom& g, int Nc, int K, int C, const Plan& m, int G, hipStream_t s) {
  int rc;
  if ((rc = launch_mask_compact_batch(g, Nc, K, G, m.perm, m.seg_off, m.compact_ws, s))) return rc;
  hipLaunchKernelGGL(mask_gather_kernel, dim3(rows_grid(Nc, C), G), dim3(256), 0, s, content, (const int*)m.perm, (const int*)m.seg_off, K, C,
                     Nc, m.xg);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

// the single-pixel labels of the G frames of a masked plan pass through
template <typename Plan>
static int launch_mask_passthrough(const float* content, int Nc, int C, const Plan& m, int G, int K, half_t* out16, float* out32, hipStream_t s) {
  if (!m.any_single) return WCT_OK;
  hipLaunchKernelGGL(mask_passthrough_kernel, dim3(K, G), dim3(256), 0, s, content, (const int*)m.seg_off, (const int*)m.perm, m.single,
                     C, Nc, out16, out32);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_wct_masked(const float* content, int Nc, const MaskGeom& g, const int* nk, const float* const* styles, const int* Ns, int K,
                      int C, const WctCall& r) {
  const int mode = r.mode, stages = r.stages; hipStream_t s = r.stream;
  MaskPlan m;
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 1024 && content && styles && mask_plan(&m, r.workspace, C, Nc, nk, styles, Ns, K, 2));
  ARG_CHECK(mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  ARG_CHECK(launch_map_fits((size_t)Nc * C, 4) && plan_fits(m, C));
  ARG_CHECK(r.workspace_bytes >= m.total);
  const WctCarve& w = m.w;
  int rc;
  if (stages & WCT_STAGE_COV) {
    if ((rc = launch_mask_gather(content, g, Nc, K, C, m, 1, s))) return rc;
    if ((rc = launch_plan_stats(m, C, false, true, cov_eps(mode, r.eps), s))) return rc;
  }
  if ((stages & WCT_STAGE_EIG) && m.P > 0 && (rc = launch_eig_stage(w, C, m.P, m.skip, 1, r.sweeps_dev, r.eig_fail, s))) return rc;
  if (!(stages & WCT_STAGE_APPLY)) return WCT_OK;
  if (m.P > 0) {
    if ((rc = launch_spectral_tail(w, C, m.P, r.alpha, mode, r.eps, m.skip, m.nwhite, s))) return rc;
    if ((rc = launch_blend(w, C, m.P, r.alpha, m.skip, s))) return rc;
    ApplySegArgs a = apply_args<ApplySegArgs>(w, m.xg, 0, C, r.out16, r.out32);
    a.seg_off = m.seg_off; a.perm = m.perm;
    for (int p = 0; p < WCT_MIX_MAX; ++p) a.lab[p] = m.lab[p];           // (0 past the pairs)
    if ((rc = launch_apply_args(a, m.nmax, m.P, s))) return rc;
  }
  return launch_mask_passthrough(content, Nc, C, m, 1, K, r.out16, r.out32, s);
}

// AdaIN of the segments: as adain_apply_kernel (same expression, so the same bits) on pair p = label lab[p], rows read from the
// gathered buffer and stored to their pixel rows
struct SegLabels { int lab[WCT_MIX_MAX]; };
// a masked batch: pair p is label fl[p] & 7 of frame fl[p] >> 3, frames of N rows (ApplySegBatchArgs)
struct SegBatchLabels { unsigned char fl[WCT_PLAN_PAIRS]; int N; };
template <typename Labels>
__global__ void adain_seg_apply_kernel(const float* xg, const int* seg_off, const int* perm, Labels sl, int C, const float* mean,
                                       const float* var, float alpha, float eps, half_t* out16, float* out32) {
  const int pair = blockIdx.y;
  int lab;
  if constexpr (std::is_same<Labels, SegBatchLabels>::value) {
    const int f = seg_frame(sl.fl[pair]);
    lab = seg_label(sl.fl[pair]);
    const size_t row0 = (size_t)f * sl.N;
    xg += row0 * C; perm += row0; seg_off += f * SEG_STRIDE;
    if (out16) out16 += row0 * C;
    if (out32) out32 += row0 * C;
  } else
    lab = sl.lab[pair];
  const int cq = C / 4;
  const int r0 = seg_off[lab];
  const size_t n4 = (size_t)(seg_off[lab + 1] - r0) * cq;
  const float* mp = mean + (size_t)pair * 2 * C;
  const float* vp = var + (size_t)pair * 2 * C;
  const float* ms = mp + C;
  const float* vs = vp + C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / cq), c = (int)(i % cq) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(xg + (size_t)(r0 + r) * C + c);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float inv = 1.f / sqrtf(vp[c + j] + eps);
      const float sd = sqrtf(vs[c + j]);
      const float y = (v[j] - mp[c + j]) * inv * sd + ms[c + j];
      o[j] = alpha * y + (1.f - alpha) * v[j];
    }
    const size_t dst = (size_t)perm[r0 + r] * C + c;
    if (out32) *reinterpret_cast<f32x4*>(out32 + dst) = o;
    if (out16) {
      half4 h;
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = (half_t)o[j];
      *reinterpret_cast<half4*>(out16 + dst) = h;
    }
  }
}

int launch_adain_masked(const float* content, int Nc, const MaskGeom& g, const int* nk, const float* const* styles, const int* Ns, int K,
                        int C, const WctCall& r) {
  hipStream_t s = r.stream;
  MaskPlan m;
  ARG_CHECK(C % 4 == 0 && C <= 1024 && content && styles && mask_plan(&m, r.workspace, C, Nc, nk, styles, Ns, K, 1));
  ARG_CHECK(r.workspace_bytes >= m.total);
  const WctCarve& w = m.w;
  int rc;
  if ((rc = launch_mask_gather(content, g, Nc, K, C, m, 1, s))) return rc;
  if ((rc = launch_plan_stats(m, C, true, false, 0.f, s))) return rc;
  if (m.P > 0) {
    SegLabels sl;
    for (int p = 0; p < WCT_MIX_MAX; ++p) sl.lab[p] = m.lab[p];
    hipLaunchKernelGGL(adain_seg_apply_kernel<SegLabels>, dim3(rows_grid(m.nmax, C), m.P), dim3(256), 0, s, (const float*)m.xg, (const int*)m.seg_off,
                       (const int*)m.perm, sl, C, (const float*)w.mean, (const float*)w.var, r.alpha, r.eps, r.out16, r.out32);
    HIP_TRY(hipGetLastError());
  }
  return launch_mask_passthrough(content, Nc, C, m, 1, K, r.out16, r.out32, s);
}

// ---------------------------------------------------------------------------
// Masked batch on prepared styles.  G frames, each with its own label map; pair p = the p-th (frame, label) with >= 2 rows,
// frame-major.  Slot 2p: the region's rows of the gathered buffer xg [G][Nc][C], with the layout pair_layout(C, nk, Ns[label]) --
// what mask_plan gives the region in a single-frame call; slot 2p + 1 is dead (WCT_SKIP_STYLES) and takes the state of style
// `label` under that layout's key (launch_style_load_slots) in front of the spectral tail.  One compaction, one gather, one
// batched eigensolve of the P live matrices, one tail, one blend and one segmented apply for all G frames; the statistics and
// covariance of a region are the launches of its single-frame call (launch_plan_stats), so a matrix's bits do not move, and the
// solver's results do not depend on the batch: frame f comes out as launch_wct_masked gives it alone.
// ---------------------------------------------------------------------------
struct MaskBatchPlan : SlotPlan {
  int G, nmax; bool any_single;
  unsigned char fl[WCT_PLAN_PAIRS];              // pair p: frame << 3 | label
  SingleLabels single;                           // frame f, bit k: label k has 1 row
  float* xg; int *perm, *seg_off; void* compact_ws;
};

int wct_masked_batch_pairs(int G, const int* nk, int K) {
  int P = 0;
  for (int f = 0; f < G; ++f)
    for (int k = 0; k < K; ++k) P += nk[f * WCT_MIX_MAX + k] >= 2;
  return P;
}

static bool mask_batch_plan(MaskBatchPlan* m, void* base, int C, int Nc, int G, const int* nk, const int* Ns, int K, int nmin) {
  if (!nk || !Ns || K < 1 || K > WCT_MIX_MAX || Nc < 1 || G < 1 || G > WCT_PLAN_PAIRS) return false;
  if (wct_masked_batch_pairs(G, nk, K) > WCT_PLAN_PAIRS) return false;
  const int Cw = std::max(C, 32);
  *m = MaskBatchPlan{};
  m->G = G;
  int row0[WCT_PLAN_PAIRS];                      // where the rows of pair p start in its frame (host counts)
  for (int f = 0; f < G; ++f) {
    long long sum = 0;
    for (int k = 0; k < K; ++k) {
      const int n = nk[f * WCT_MIX_MAX + k];
      if (n < 0 || (n >= 2 && Ns[k] < nmin)) return false;
      if (n == 1) { m->single.frame[f] |= (unsigned char)(1u << k); m->any_single = true; }
      if (n >= 2) {
        const int p = m->P++;
        m->fl[p] = (unsigned char)(f << 3 | k);
        row0[p] = (int)sum;
        m->nmax = std::max(m->nmax, n);
        const PairLayout lay = pair_layout(Cw, n, Ns[k]);
        m->slot[2 * p] = {nullptr, n, lay};
        m->slot[2 * p + 1] = {nullptr, 0, lay};  // dead: a prepared state
      }
      sum += n;
    }
    if (sum != Nc) return false;                 // every row of the frame has a label < K (the caller counted them)
  }
  m->skip = WCT_SKIP_STYLES;
  m->nwhite = m->P;
  mask_carve(m, base, Cw, Nc, G);
  if (m->xg)
    for (int p = 0; p < m->P; ++p) m->slot[2 * p].x = m->xg + ((size_t)seg_frame(m->fl[p]) * Nc + row0[p]) * C;
  return true;
}

size_t wct_masked_batch_workspace_bytes(int C, int Nc, int G, const int* nk, const int* Ns, int K) {
  MaskBatchPlan m;
  return mask_batch_plan(&m, nullptr, C, Nc, G, nk, Ns, K, 1) ? m.total : 0;
}

int launch_wct_masked_batch(const float* content, int Nc, int G, const MaskGeom& g, const int* nk, const int* Ns, int K, int C,
                            const WctCall& r, const WctStyleSlots& states) {
  const int mode = r.mode, stages = r.stages; hipStream_t s = r.stream;
  MaskBatchPlan m;
  ARG_CHECK(C % 32 == 0 && C >= 32 && C <= 1024 && content && mask_batch_plan(&m, r.workspace, C, Nc, G, nk, Ns, K, 2));
  ARG_CHECK(mode == WCT_MODE_NP || mode == WCT_MODE_TF);
  ARG_CHECK(launch_map_fits((size_t)Nc * C, 4) && plan_fits(m, C));
  ARG_CHECK((size_t)G * Nc < ((size_t)1 << 31));                        // (row indices are ints)
  ARG_CHECK(r.workspace_bytes >= m.total);
  const WctCarve& w = m.w;
  int rc;
  if (stages & WCT_STAGE_COV) {
    if ((rc = launch_mask_gather(content, g, Nc, K, C, m, m.G, s))) return rc;
    if ((rc = launch_plan_stats(m, C, false, true, cov_eps(mode, r.eps), s))) return rc;
  }
  if ((stages & WCT_STAGE_EIG) && m.P > 0 && (rc = launch_eig_stage(w, C, m.P, m.skip, 1, nullptr, r.eig_fail, s))) return rc;
  if (!(stages & WCT_STAGE_APPLY)) return WCT_OK;
  if (m.P > 0) {
    if ((rc = launch_style_load_slots(states, m.P, w, C, true, s))) return rc;
    if ((rc = launch_spectral_tail(w, C, m.P, r.alpha, mode, r.eps, m.skip, m.nwhite, s))) return rc;
    if ((rc = launch_blend(w, C, m.P, r.alpha, m.skip, s))) return rc;
    ApplySegBatchArgs a = apply_args<ApplySegBatchArgs>(w, m.xg, Nc, C, r.out16, r.out32);
    a.seg_off = m.seg_off; a.perm = m.perm;
    for (int p = 0; p < WCT_PLAN_PAIRS; ++p) a.fl[p] = m.fl[p];          // (0 past the pairs)
    if ((rc = launch_apply_args(a, m.nmax, m.P, s))) return rc;
  }
  return launch_mask_passthrough(content, Nc, C, m, m.G, K, r.out16, r.out32, s);
}

int launch_adain_masked_batch(const float* content, int Nc, int G, const MaskGeom& g, const int* nk, const int* Ns, int K, int C,
                              const WctCall& r, const WctStyleSlots& states) {
  hipStream_t s = r.stream;
  MaskBatchPlan m;
  ARG_CHECK(C % 32 == 0 && C <= 1024 && content && mask_batch_plan(&m, r.workspace, C, Nc, G, nk, Ns, K, 1));
  ARG_CHECK((size_t)G * Nc < ((size_t)1 << 31));
  ARG_CHECK(r.workspace_bytes >= m.total);
  const WctCarve& w = m.w;
  int rc;
  if ((rc = launch_mask_gather(content, g, Nc, K, C, m, m.G, s))) return rc;
  if ((rc = launch_plan_stats(m, C, true, false, 0.f, s))) return rc;
  if (m.P > 0) {
    if ((rc = launch_style_load_slots(states, m.P, w, C, false, s))) return rc;
    SegBatchLabels sl = {};
    for (int p = 0; p < WCT_PLAN_PAIRS; ++p) sl.fl[p] = m.fl[p];
    sl.N = Nc;
    hipLaunchKernelGGL(adain_seg_apply_kernel<SegBatchLabels>, dim3(rows_grid(m.nmax, C), m.P), dim3(256), 0, s, (const float*)m.xg,
                       (const int*)m.seg_off, (const int*)m.perm, sl, C, (const float*)w.mean, (const float*)w.var, r.alpha, r.eps, r.out16,
                       r.out32);
    HIP_TRY(hipGetLastError());
  }
  return launch_mask_passthrough(content, Nc, C, m, m.G, K, r.out16, r.out32, s);
}
