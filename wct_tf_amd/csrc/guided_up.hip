// Guided upsampling (guided_up_rule.h; He, Sun, "Fast Guided Filter"): small stylized frames delivered at the size of the full
// contents -- three launches for up to 32 frames.
//   pass 1 (guided.hip, launch_guided_ab): s [B][h][w][3] + c [B][hc][wc][3] -> ab [B][h][w][3][2] int32
//   means:  ab -> mean [B][h][w][3][2] int32, (am, bm) of every small pixel and channel: the tiling of pass 2 of guided.hip
//           (window_sums_ab of guided_tile.h), the rule's two divisions per channel in place of the byte
//   full:   mean + C [B][H][W][3] (uint8, or fp32 in [0,1] quantised by wct_quantise_u8) -> out [B][H][W][3] uint8
// The full-size kernel.  A wave owns a tile of UTW = 256 columns x URW = 16 rows of one frame; a lane owns UPX = 4 consecutive
// columns of it, so that with W % 4 == 0 (and dword-aligned bases) the 12 content bytes and the 12 frame bytes of a lane and row
// are three whole dwords.  The x-axis taps of the lane's four columns are formed once per tile; lane i forms the y-axis taps of
// row ya + i, and every row reads its own with a readlane (one pair of divisions per lane and tile on either axis).
// The small map is read through the cache, not staged in LDS: per small row and pixel the lane blends its two x-neighbours
// (A = (256 - fx) am0 + fx am1 < 2^26, B likewise < 1.8e10) and KEEPS the two blended small rows y0, y1 in registers; the next full
// row reuses them, and when y0 moves on (by one: the ratio is at least 1) row y1 becomes row y0 and one small row is read.  The
// reads of the map per full row so shrink with the ratio as an LDS footprint would, without a barrier and without a bound on the
// tile at ratio 1.  Per pixel and channel:  v = ((256 - fy) A0 + fy A1) I + ((256 - fy) B0 + fy B1), the rule's sum in another
// order (exact integers: |.| < 2^34, < 4.5e12, |v| < 8.9e12).  No division at full size.  Offsets are size_t.
#include "guided_tile.h"
#include "guided_up_rule.h"

namespace {
__global__ __launch_bounds__(NT) void guided_up_mean_kernel(const int32_t* ab, int32_t* mean, int H, int W, int r, int strips, int segs) {
  __shared__ long long P[6][NT];
  __shared__ long long tot[6][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int x = pl.x;
  window_sums_ab(ab + (size_t)pl.b * H * W * 6, pl, H, W, r, P, tot, [&](int y, const int64_t (&S)[6]) {
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    int2* op = reinterpret_cast<int2*>(mean + (((size_t)pl.b * H + y) * W + x) * 6);      // 24 B per pixel from an 8-byte aligned base
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int32_t am, bm;
      wct_guided_up_mean(n, S[2 * ch], S[2 * ch + 1], &am, &bm);
      op[ch] = make_int2(am, bm);
    }
  });
}

constexpr int UPX = 4;                // consecutive columns of a lane
constexpr int UTW = 64 * UPX;         // columns of a wave's tile
constexpr int URW = 16;               // rows of a wave's tile (at most 64: lane i holds the taps of row i)
constexpr int UTH = NW * URW;         // rows of a block: its waves are stacked
constexpr int ONE = WCT_GUIDED_UP_ONE;

struct __attribute__((packed, aligned(4))) Bytes12 { uint32_t d[3]; };
struct __attribute__((packed, aligned(4))) Floats12 { float f[12]; };

// the guides of four consecutive content pixels that start at a dword boundary
__device__ __forceinline__ void guides4(const uint8_t* p, int (&I)[UPX]) {
  const Bytes12 v = *reinterpret_cast<const Bytes12*>(p);
  int c[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) c[k] = (int)((v.d[k >> 2] >> (8 * (k & 3))) & 255u);
#pragma unroll
  for (int j = 0; j < UPX; ++j) I[j] = wct_guided_guide(c[3 * j], c[3 * j + 1], c[3 * j + 2]);
}
__device__ __forceinline__ void guides4(const float* p, int (&I)[UPX]) {
  const Floats12 v = *reinterpret_cast<const Floats12*>(p);
#pragma unroll
  for (int j = 0; j < UPX; ++j)
    I[j] = wct_guided_guide(wct_quantise_u8(v.f[3 * j]), wct_quantise_u8(v.f[3 * j + 1]), wct_quantise_u8(v.f[3 * j + 2]));
}

// VEC: W % 4 == 0 and dword-aligned bases -- whole-dword content loads and frame stores.  A32: both axes satisfy
// wct_guided_up_axis32_ok -- the taps in 32-bit arithmetic.
template <typename CT, bool VEC, bool A32>
__global__ __launch_bounds__(NT) void guided_up_kernel(const int32_t* mean, const CT* C, uint8_t* out, int H, int W, int h, int w, int hc,
                                                       int wc, int tiles_x, int tiles_y) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int id = blockIdx.x;
  const int tx = id % tiles_x; id /= tiles_x;
  const int ty = id % tiles_y;
  const int b = id / tiles_y;
  const int ya = ty * UTH + wave * URW;
  if (ya >= H) return;                                        // (the whole wave; the kernel has no barrier)
  const int rows = URW < H - ya ? URW : H - ya;
  const int x4 = tx * UTW + lane * UPX;
  const bool active = x4 < W;                                 // an idle lane still serves its row's taps below
  const int npx = !active ? 0 : (UPX < W - x4 ? UPX : W - x4);
  auto axis = [](int P, int N, int m, int* p0, int* p1, int* f) {
    if (A32) wct_guided_up_axis32(P, N, m, p0, p1, f);
    else wct_guided_up_axis(P, N, m, p0, p1, f);
  };
  int xp0[UPX], xp1[UPX], xf[UPX];
#pragma unroll
  for (int j = 0; j < UPX; ++j) axis(x4 + j < W ? x4 + j : W - 1, W, wc, &xp0[j], &xp1[j], &xf[j]);
  int my0, my1, myf;
  axis(ya + lane < H ? ya + lane : H - 1, H, hc, &my0, &my1, &myf);

  const int2* mb = reinterpret_cast<const int2*>(mean + (size_t)b * h * w * 6);
  int32_t A[2][UPX][3];                                       // the two small rows in use, blended along x: |A| < 2^18 * 256
  int64_t Bq[2][UPX][3];                                      // |B| < 6.8e7 * 256
  auto load = [&](int32_t (&a)[UPX][3], int64_t (&bq)[UPX][3], int ys) {     // ys < hc, the columns < wc: inside the map
    if (!active) return;
#pragma unroll
    for (int j = 0; j < UPX; ++j) {
      const int2* m0 = mb + ((size_t)ys * w + xp0[j]) * 3;
      const int2* m1 = mb + ((size_t)ys * w + xp1[j]) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int2 u = m0[ch], v = m1[ch];
        a[j][ch] = (ONE - xf[j]) * u.x + xf[j] * v.x;
        bq[j][ch] = (int64_t)(ONE - xf[j]) * u.y + (int64_t)xf[j] * v.y;
      }
    }
  };
  auto copy = [&](int32_t (&a)[UPX][3], int64_t (&bq)[UPX][3], const int32_t (&a2)[UPX][3], const int64_t (&bq2)[UPX][3]) {
#pragma unroll
    for (int j = 0; j < UPX; ++j)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) { a[j][ch] = a2[j][ch]; bq[j][ch] = bq2[j][ch]; }
  };

  // the guides of the lane's pixels of row y; the next row's are loaded before this row's arithmetic
  auto guides = [&](int y, int (&I)[UPX]) {
    const size_t pix = ((size_t)b * H + y) * W + x4;          // B * H * W * 3 < 2^31 is checked; size_t all the same
    if (VEC) { guides4(C + pix * 3, I); return; }
#pragma unroll
    for (int j = 0; j < UPX; ++j) {
      I[j] = 0;
      if (j < npx) { const CT* cp = C + (pix + j) * 3; I[j] = wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2)); }
    }
  };
  int In[UPX] = {0, 0, 0, 0};
  if (active) guides(ya, In);
  int r0 = -1, r1 = -1;                                       // the small rows that A[0], A[1] hold
#pragma unroll 1
  for (int i = 0; i < rows; ++i) {
    const int y = ya + i;
    const int y0 = __builtin_amdgcn_readlane(my0, i), y1 = __builtin_amdgcn_readlane(my1, i), fy = __builtin_amdgcn_readlane(myf, i);
    if (y0 != r0) {
      if (y0 == r1) copy(A[0], Bq[0], A[1], Bq[1]);
      else load(A[0], Bq[0], y0);
      r0 = y0;
    }
    if (y1 != r1) {
      if (y1 == r0) copy(A[1], Bq[1], A[0], Bq[0]);
      else load(A[1], Bq[1], y1);
      r1 = y1;
    }
    if (!active) continue;
    const size_t pix = ((size_t)b * H + y) * W + x4;
    int I[UPX];
#pragma unroll
    for (int j = 0; j < UPX; ++j) I[j] = In[j];
    if (i + 1 < rows) guides(y + 1, In);
    uint8_t o[3 * UPX];
#pragma unroll
    for (int j = 0; j < UPX; ++j)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t Av = (int64_t)A[0][j][ch] * (ONE - fy) + (int64_t)A[1][j][ch] * fy;      // |Av| < 2^34
        const int64_t Bv = Bq[0][j][ch] * (ONE - fy) + Bq[1][j][ch] * fy;                    // |Bv| < 4.5e12
        o[3 * j + ch] = wct_guided_up_out(Av * I[j] + Bv);
      }
    if (VEC) {
      Bytes12 v;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        v.d[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
      *reinterpret_cast<Bytes12*>(out + pix * 3) = v;
    } else {
#pragma unroll
      for (int j = 0; j < UPX; ++j)
        if (j < npx) { uint8_t* op = out + (pix + j) * 3; op[0] = o[3 * j]; op[1] = o[3 * j + 1]; op[2] = o[3 * j + 2]; }
    }
  }
}

template <typename CT, bool VEC, bool A32>
void launch_full(const int32_t* mean, const CT* C, uint8_t* out, int B, int H, int W, int h, int w, int hc, int wc, hipStream_t st) {
  const int tiles_x = cdiv(W, UTW), tiles_y = cdiv(H, UTH);
  hipLaunchKernelGGL((guided_up_kernel<CT, VEC, A32>), dim3((unsigned)B * tiles_x * tiles_y), dim3(NT), 0, st, mean, C, out, H, W, h, w,
                     hc, wc, tiles_x, tiles_y);
}

// the full-size launch over mean [B][h][w][3][2] and C [B][H][W][3], the variant chosen by W, the bases and the axes
template <typename CT>
int select_full(const int32_t* mean, const CT* C, uint8_t* out, int B, int H, int W, int h, int w, int hc, int wc, hipStream_t st) {
  const bool vec = W % 4 == 0 && (uintptr_t)C % 4 == 0 && (uintptr_t)out % 4 == 0;
  const bool a32 = wct_guided_up_axis32_ok(W, wc) && wct_guided_up_axis32_ok(H, hc);
  if (vec && a32) launch_full<CT, true, true>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else if (vec) launch_full<CT, true, false>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else if (a32) launch_full<CT, false, true>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else launch_full<CT, false, false>(mean, C, out, B, H, W, h, w, hc, wc, st);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

template <typename CT>
int launch(const uint8_t* s, const CT* c, const CT* C, int B, int h, int w, int hc, int wc, int H, int W, int r, int eps_q, void* workspace,
           uint8_t* out, hipStream_t st) {
  int32_t* ab = (int32_t*)workspace;
  int32_t* mean = ab + (size_t)B * h * w * 6;
  int rc = launch_guided_ab(s, c, sizeof(CT) == 4, B, h, w, hc, wc, r, eps_q, ab, st);
  if (rc) return rc;
  const int strips = cdiv(w, NT - 2 * r), segs = cdiv(h, SEG);
  hipLaunchKernelGGL(guided_up_mean_kernel, dim3((unsigned)B * strips * segs), dim3(NT), 0, st, (const int32_t*)ab, mean, h, w, r, strips,
                     segs);
  HIP_TRY(hipGetLastError());
  return select_full(mean, C, out, B, H, W, h, w, hc, wc, st);
}
}  // namespace

int launch_guided_up_full(const int32_t* mean, const uint8_t* content_full, uint8_t* out, int B, int H, int W, int h, int w, int hc, int wc,
                          hipStream_t s) {
  ARG_CHECK(mean && content_full && out);
  return select_full(mean, content_full, out, B, H, W, h, w, hc, wc, s);
}

int guided_up_check(int B, int h, int w, int hc, int wc, int H, int W, int radius, int eps_q) {
  if (B < 1 || B > 32) { wct_set_error("guided upsample: B = %d frames, must be 1 .. 32", B); return WCT_ERR_ARG; }
  if (hc < 1 || wc < 1 || h < hc || w < wc) {
    wct_set_error("guided upsample: h x w = %dx%d, a small stylized frame for a %dx%d small content (the frame is never the smaller one)",
                  h, w, hc, wc);
    return WCT_ERR_ARG;
  }
  if (H < hc || W < wc) {
    wct_set_error("guided upsample: H x W = %dx%d, a full content smaller than the %dx%d small content (down-scaling is not served)", H, W,
                  hc, wc);
    return WCT_ERR_ARG;
  }
  if (!wct_guided_params_ok(radius, eps_q)) {
    wct_set_error("guided upsample: radius %d, eps_q %d; the radius is 1 .. %d and eps_q 1 .. %d (grey levels squared)", radius, eps_q,
                  WCT_GUIDED_MAX_RADIUS, WCT_GUIDED_MAX_EPS);
    return WCT_ERR_ARG;
  }
  if ((unsigned long long)B * (unsigned long long)H * (unsigned long long)W * 3ull >= (1ull << 31)) {
    wct_set_error("guided upsample: H x W: %d full frames of %dx%dx3 pass 2^31 bytes in one call", B, H, W);
    return WCT_ERR_ARG;
  }
  if ((unsigned long long)B * (unsigned long long)h * (unsigned long long)w * 3ull >= (1ull << 31)) {
    wct_set_error("guided upsample: h x w: %d small frames of %dx%dx3 pass 2^31 bytes in one call", B, h, w);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

size_t guided_up_workspace_bytes(int B, int h, int w) { return (size_t)B * h * w * 6 * sizeof(int32_t) * 2; }

int launch_guided_upsample(const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B, int h,
                           int w, int hc, int wc, int H, int W, int radius, int eps_q, void* workspace, uint8_t* out, hipStream_t s) {
  ARG_CHECK(stylized && content_small && content_full && workspace && out);
  int rc = guided_up_check(B, h, w, hc, wc, H, W, radius, eps_q);
  if (rc) return rc;
  if (content_f32)
    return launch(stylized, (const float*)content_small, (const float*)content_full, B, h, w, hc, wc, H, W, radius, eps_q, workspace, out, s);
  return launch(stylized, (const uint8_t*)content_small, (const uint8_t*)content_full, B, h, w, hc, wc, H, W, radius, eps_q, workspace, out, s);
}
