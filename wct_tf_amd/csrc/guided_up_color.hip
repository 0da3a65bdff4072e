// Guided upsampling under the colour guide (guided_up_color_rule.h): small stylized frames delivered at the size of the full
// contents, every output channel linear in the three channels of the full content -- three launches for up to 32 frames.
//   pass 1 (guided_color.hip, launch_guided_color_ab): s [B][h][w][3] + c [B][hc][wc][3] -> ab [B][h][w][12] int32
//   means:  ab -> mean [B][h][w][12] int32, the twelve means of every small pixel in the layout of ab: the tiling of pass 2 of
//           guided_color.hip (window_sums_ab12 of guided_tile.h), the rule's twelve divisions in place of the byte, three 16-byte
//           stores per pixel
//   full:   mean + C [B][H][W][3] (uint8, or fp32 in [0,1] quantised by wct_quantise_u8) -> out [B][H][W][3] uint8
// The full-size kernel is the scheme of guided_up.hip with twelve coefficients per small pixel in place of six.  A wave owns a tile
// of CTW = 128 columns x CRW = 16 rows of one frame; a lane owns CPX = 2 consecutive columns of it: the two blended small rows it
// keeps cost 30 registers per owned column, and the four columns of guided_up.hip do not fit beside them.  With W even
// and 2-byte aligned bases the 6 content bytes and the 6 frame bytes of a lane and row are three whole 16-bit words; one general
// path with byte accesses serves any W and any base.  The x-axis taps of the lane's columns are formed once per tile; lane i forms
// the y-axis taps of row ya + i, and every row reads its own with a readlane.
// Per small row and pixel the lane blends its two x-neighbours -- nine A = (256 - fx) am0 + fx am1, |A| <= 256 * 288400 < 2^27
// (int32), three B likewise, |B| <= 256 * 2.22e8 < 5.7e10 (int64) -- and KEEPS the two blended small rows y0, y1 in registers; the
// next full row reuses them, and when y0 moves on (by one: the ratio is at least 1) row y1 becomes row y0 and one small row is
// read.  Per pixel and channel p:  v = sum_i ((256 - fy) A0[i][p] + fy A1[i][p]) I_i + ((256 - fy) B0[p] + fy B1[p]), the rule's sum
// in another order (exact integers: each bracket within 2^35, times 255 and summed with the last within 2.91e13).  No division at
// full size.  Offsets are size_t.
#include "guided_tile.h"
#include "guided_up_color_rule.h"

namespace {
constexpr int KC = WCT_GUIDED_COLOR_COEFFS;

__global__ __launch_bounds__(NT) void guided_up_color_mean_kernel(const int32_t* ab, int32_t* mean, int H, int W, int r, int strips,
                                                                  int segs) {
  __shared__ long long P[KC][NT];
  __shared__ long long tot[KC][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int x = pl.x;
  window_sums_ab12(ab + (size_t)pl.b * H * W * KC, pl, H, W, r, P, tot, [&](int y, auto win) {
    const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
    int64_t S[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) S[k] = win(k);
    int32_t m[KC];
    wct_guided_up_color_mean(n, S, m);
    int4* op = reinterpret_cast<int4*>(mean + (((size_t)pl.b * H + y) * W + x) * KC);        // 48 B per pixel: 16-byte aligned
#pragma unroll
    for (int k = 0; k < KC / 4; ++k) op[k] = make_int4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
  });
}

constexpr int CPX = 2;                // consecutive columns of a lane
constexpr int CTW = 64 * CPX;         // columns of a wave's tile
constexpr int CRW = 16;               // rows of a wave's tile (at most 64: lane i holds the taps of row i)
constexpr int CTH = NW * CRW;         // rows of a block: its waves are stacked
constexpr int ONE = WCT_GUIDED_UP_ONE;

struct __attribute__((packed, aligned(2))) Bytes6 { uint16_t d[3]; };
struct __attribute__((packed, aligned(4))) Floats6 { float f[3 * CPX]; };

// the three channels of CPX consecutive content pixels that start at a 2-byte boundary
__device__ __forceinline__ void pixels2(const uint8_t* p, int (&I)[CPX][3]) {
  const Bytes6 v = *reinterpret_cast<const Bytes6*>(p);
#pragma unroll
  for (int k = 0; k < 3 * CPX; ++k) I[k / 3][k % 3] = (int)((v.d[k >> 1] >> (8 * (k & 1))) & 255u);
}
__device__ __forceinline__ void pixels2(const float* p, int (&I)[CPX][3]) {
  const Floats6 v = *reinterpret_cast<const Floats6*>(p);
#pragma unroll
  for (int k = 0; k < 3 * CPX; ++k) I[k / 3][k % 3] = wct_quantise_u8(v.f[k]);
}

// VEC: W even and 2-byte aligned bases -- whole-word content loads and frame stores.  A32: both axes satisfy
// wct_guided_up_axis32_ok -- the taps in 32-bit arithmetic.
template <typename CT, bool VEC, bool A32>
__global__ __launch_bounds__(NT) void guided_up_color_kernel(const int32_t* mean, const CT* C, uint8_t* out, int H, int W, int h, int w,
                                                             int hc, int wc, int tiles_x, int tiles_y) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int id = blockIdx.x;
  const int tx = id % tiles_x; id /= tiles_x;
  const int ty = id % tiles_y;
  const int b = id / tiles_y;
  const int ya = ty * CTH + wave * CRW;
  if (ya >= H) return;                                        // (the whole wave; the kernel has no barrier)
  const int rows = CRW < H - ya ? CRW : H - ya;
  const int x2 = tx * CTW + lane * CPX;
  const bool active = x2 < W;                                 // an idle lane still serves its row's taps below
  const int npx = !active ? 0 : (CPX < W - x2 ? CPX : W - x2);
  auto axis = [](int P, int N, int m, int* p0, int* p1, int* f) {
    if (A32) wct_guided_up_axis32(P, N, m, p0, p1, f);
    else wct_guided_up_axis(P, N, m, p0, p1, f);
  };
  int xp0[CPX], xp1[CPX], xf[CPX];
#pragma unroll
  for (int j = 0; j < CPX; ++j) axis(x2 + j < W ? x2 + j : W - 1, W, wc, &xp0[j], &xp1[j], &xf[j]);
  int my0, my1, myf;
  axis(ya + lane < H ? ya + lane : H - 1, H, hc, &my0, &my1, &myf);

  const int4* mb = reinterpret_cast<const int4*>(mean + (size_t)b * h * w * KC);
  int32_t A[2][CPX][9];                                       // the two small rows in use, blended along x: |A| < 2^27
  int64_t Bq[2][CPX][3];                                      // |B| < 5.7e10
  auto load = [&](int32_t (&a)[CPX][9], int64_t (&bq)[CPX][3], int ys) {      // ys < hc, the columns < wc: inside the map
    if (!active) return;
#pragma unroll
    for (int j = 0; j < CPX; ++j) {
      const int4* m0 = mb + ((size_t)ys * w + xp0[j]) * (KC / 4);
      const int4* m1 = mb + ((size_t)ys * w + xp1[j]) * (KC / 4);
      const int4 u0 = m0[0], u1 = m0[1], u2 = m0[2], v0 = m1[0], v1 = m1[1], v2 = m1[2];
      const int32_t u[KC] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, u2.x, u2.y, u2.z, u2.w};
      const int32_t v[KC] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
      for (int k = 0; k < 9; ++k) a[j][k] = (ONE - xf[j]) * u[k] + xf[j] * v[k];
#pragma unroll
      for (int p = 0; p < 3; ++p) bq[j][p] = (int64_t)(ONE - xf[j]) * u[9 + p] + (int64_t)xf[j] * v[9 + p];
    }
  };
  auto copy = [&](int32_t (&a)[CPX][9], int64_t (&bq)[CPX][3], const int32_t (&a2)[CPX][9], const int64_t (&bq2)[CPX][3]) {
#pragma unroll
    for (int j = 0; j < CPX; ++j) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a[j][k] = a2[j][k];
#pragma unroll
      for (int p = 0; p < 3; ++p) bq[j][p] = bq2[j][p];
    }
  };

  // the content pixels of the lane's columns of row y; the next row's are loaded before this row's arithmetic
  auto pixels = [&](int y, int (&I)[CPX][3]) {
    const size_t pix = ((size_t)b * H + y) * W + x2;          // B * H * W * 3 < 2^31 is checked; size_t all the same
    if (VEC) { pixels2(C + pix * 3, I); return; }
#pragma unroll
    for (int j = 0; j < CPX; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) I[j][i] = j < npx ? sample(C + (pix + j) * 3 + i) : 0;
  };
  int In[CPX][3] = {};
  if (active) pixels(ya, In);
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
    const size_t pix = ((size_t)b * H + y) * W + x2;
    int I[CPX][3];
#pragma unroll
    for (int j = 0; j < CPX; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) I[j][k] = In[j][k];
    if (i + 1 < rows) pixels(y + 1, In);
    uint8_t o[3 * CPX];
#pragma unroll
    for (int j = 0; j < CPX; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        int64_t v = Bq[0][j][p] * (ONE - fy) + Bq[1][j][p] * fy;                                   // within 1.46e13
#pragma unroll
        for (int k = 0; k < 3; ++k)                                                                // each bracket within 2^35
          v += ((int64_t)A[0][j][3 * k + p] * (ONE - fy) + (int64_t)A[1][j][3 * k + p] * fy) * I[j][k];
        o[3 * j + p] = wct_guided_up_out(v);
      }
    if (VEC) {
      Bytes6 v;
#pragma unroll
      for (int k = 0; k < 3; ++k) v.d[k] = (uint16_t)((uint32_t)o[2 * k] | ((uint32_t)o[2 * k + 1] << 8));
      *reinterpret_cast<Bytes6*>(out + pix * 3) = v;
    } else {
#pragma unroll
      for (int j = 0; j < CPX; ++j)
        if (j < npx) { uint8_t* op = out + (pix + j) * 3; op[0] = o[3 * j]; op[1] = o[3 * j + 1]; op[2] = o[3 * j + 2]; }
    }
  }
}

template <typename CT, bool VEC, bool A32>
void launch_full(const int32_t* mean, const CT* C, uint8_t* out, int B, int H, int W, int h, int w, int hc, int wc, hipStream_t st) {
  const int tiles_x = cdiv(W, CTW), tiles_y = cdiv(H, CTH);
  hipLaunchKernelGGL((guided_up_color_kernel<CT, VEC, A32>), dim3((unsigned)B * tiles_x * tiles_y), dim3(NT), 0, st, mean, C, out, H, W, h,
                     w, hc, wc, tiles_x, tiles_y);
}

template <typename CT>
int launch(const uint8_t* s, const CT* c, const CT* C, int B, int h, int w, int hc, int wc, int H, int W, int r, int eps_q, void* workspace,
           uint8_t* out, hipStream_t st) {
  int32_t* ab = (int32_t*)workspace;
  int32_t* mean = ab + (size_t)B * h * w * KC;                // 48 B per small pixel behind pass 1's 48 B: 16-byte aligned as ab is
  int rc = launch_guided_color_ab(s, c, sizeof(CT) == 4, B, h, w, hc, wc, r, eps_q, ab, st);
  if (rc) return rc;
  const int strips = cdiv(w, NT - 2 * r), segs = cdiv(h, SEG);
  hipLaunchKernelGGL(guided_up_color_mean_kernel, dim3((unsigned)B * strips * segs), dim3(NT), 0, st, (const int32_t*)ab, mean, h, w, r,
                     strips, segs);
  HIP_TRY(hipGetLastError());
  const bool vec = W % CPX == 0 && (uintptr_t)C % CPX == 0 && (uintptr_t)out % CPX == 0;
  const bool a32 = wct_guided_up_axis32_ok(W, wc) && wct_guided_up_axis32_ok(H, hc);
  if (vec && a32) launch_full<CT, true, true>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else if (vec) launch_full<CT, true, false>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else if (a32) launch_full<CT, false, true>(mean, C, out, B, H, W, h, w, hc, wc, st);
  else launch_full<CT, false, false>(mean, C, out, B, H, W, h, w, hc, wc, st);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

size_t guided_up_color_workspace_bytes(int B, int h, int w) { return (size_t)B * h * w * KC * sizeof(int32_t) * 2; }

int launch_guided_upsample_color(const uint8_t* stylized, const void* content_small, const void* content_full, int content_f32, int B,
                                 int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, void* workspace, uint8_t* out,
                                 hipStream_t s) {
  ARG_CHECK(stylized && content_small && content_full && workspace && out);
  int rc = guided_up_check(B, h, w, hc, wc, H, W, radius, eps_q);
  if (rc) return rc;
  if (content_f32)
    return launch(stylized, (const float*)content_small, (const float*)content_full, B, h, w, hc, wc, H, W, radius, eps_q, workspace, out, s);
  return launch(stylized, (const uint8_t*)content_small, (const uint8_t*)content_full, B, h, w, hc, wc, H, W, radius, eps_q, workspace, out, s);
}
