// Temporal guided upsampling (guided_up_time_rule.h): guided upsampling with the temporal box, optionally along camera motion, where
// the coefficients are formed -- three launches for frames f0 .. f1 - 1 of a clip of up to 32 resident SMALL frames:
//   pass 1 (guided_time.hip, launch_guided_time_ab, or guided_motion.hip, launch_guided_motion_ab, under positions):
//           s [F][h][w][3] + c [F][hc][wc][3] -> ab [F][h][w][3][2] int32, the frames max(0, f0 - T) .. min(F, f1 + T) - 1, each at
//           its own position in the clip
//   means:  ab -> mean [f1 - f0][h][w][3][2] int32, (am, bm) of every small pixel and channel of the delivered frames over the 3-D,
//           optionally shifted, window: the kernel below
//   full:   mean + C [f1 - f0][H][W][3] -> out [f1 - f0][H][W][3] uint8 (guided_up.hip, launch_guided_up_full, unchanged): frame f
//           reads its own means and its own full content only
// The means kernel is pass 2 of guided_motion.hip (the tiling of guided_tile.h: 256 threads, strips of 256 - 2r columns, SEG-row
// segments; a thread keeps its column's vertical window sums, int64, over the frames of the span in registers; per row a block-wide
// prefix and a window difference) with the rule's two divisions per channel in place of the byte, written as 8-byte stores like
// guided_up_mean_kernel.  The positions travel by value, relative to frame 0; without motion they are all zero, and the same
// kernel then forms the sums of guided_time.hip's pass 2 (integer sums do not depend on the order).  Every read sits behind its own
// frame's bounds test: no position can read outside a frame.  Offsets are size_t.
#include "guided_tile.h"
#include "guided_up_time_rule.h"

namespace {
struct UpPos { int32_t p[32][2]; };

struct Span { int lo, hi; };
__device__ __forceinline__ Span span(int f, int F, int T) { return Span{f - T < 0 ? 0 : f - T, f + T > F - 1 ? F - 1 : f + T}; }

// The shifts (Dy, Dx) of the frames of the span of f: the same for every thread of a block, so they sit in scalar registers, and
// the loops over them are unrolled (NF is the longest span).
constexpr int NF = 2 * WCT_GUIDED_TIME_MAX_FRAMES + 1;
struct Shifts { int n, dy[NF], dx[NF]; };
__device__ __forceinline__ Shifts shifts(const UpPos& mp, int f, Span sp) {
  Shifts sh;
  sh.n = sp.hi - sp.lo + 1;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int g = sp.lo + k <= sp.hi ? sp.lo + k : sp.hi;
    sh.dy[k] = mp.p[g][0] - mp.p[f][0];
    sh.dx[k] = mp.p[g][1] - mp.p[f][1];
  }
  return sh;
}

// g0 = f0: block frame b is clip frame f0 + b and frame b of mean
__global__ __launch_bounds__(NT) void guided_up_time_mean_kernel(const int32_t* ab, int32_t* mean, UpPos mp, int F, int T, int g0, int H,
                                                                 int W, int r, int strips, int segs) {
  __shared__ long long P[6][NT];
  __shared__ long long tot[6][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const Shifts sh = shifts(mp, f, sp_f);
  const size_t aframe = (size_t)H * W * 6;
  long long v[6] = {0, 0, 0, 0, 0, 0};                      // the column's window sums of (a_q, b_q) per channel over the span
  auto row = [&](int y, bool add) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int yy = y + sh.dy[k], xx = x + sh.dx[k];
      if (k >= sh.n || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;     // not a pixel of frame lo + k
      const int2* p = reinterpret_cast<const int2*>(ab + (sp_f.lo + k) * aframe + ((size_t)yy * W + xx) * 6);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int2 q = p[ch];
        v[2 * ch] += add ? (long long)q.x : -(long long)q.x;
        v[2 * ch + 1] += add ? (long long)q.y : -(long long)q.y;
      }
    }
  };
  for (int y = pl.y0 - r; y < pl.y0 + r; ++y) row(y, true);                  // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    row(y + r, true);
    if (y > pl.y0) row(y - r - 1, false);
    long long w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = v[k];
    block_prefix<long long, 6>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t n = 0;                                          // wct_guided_motion_n on the shifts
#pragma unroll
    for (int k = 0; k < NF; ++k)
      if (k < sh.n) n += (int64_t)(wct_motion_extent(y + sh.dy[k], H, r) * wct_motion_extent(x + sh.dx[k], W, r));
    int2* op = reinterpret_cast<int2*>(mean + (((size_t)pl.b * H + y) * W + x) * 6);      // 24 B per pixel from an 8-byte aligned base
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t SA = P[2 * ch][t + r] - (t - r - 1 >= 0 ? P[2 * ch][t - r - 1] : 0);
      const int64_t SB = P[2 * ch + 1][t + r] - (t - r - 1 >= 0 ? P[2 * ch + 1][t - r - 1] : 0);
      int32_t am, bm;
      wct_guided_up_mean(n, SA, SB, &am, &bm);
      op[ch] = make_int2(am, bm);
    }
  }
}
}  // namespace

int guided_up_time_check(int F, int h, int w, int hc, int wc, int H, int W, int radius, int eps_q, int frames_t, int f0, int f1,
                         const int32_t* pos) {
  int rc = guided_time_check(F, h, w, hc, wc, radius, eps_q, frames_t, f0, f1);
  if (rc) return rc;
  rc = guided_up_check(f1 - f0, h, w, hc, wc, H, W, radius, eps_q);
  if (rc) return rc;
  if (!pos) return WCT_OK;
  const int bad = wct_motion_bad_step(pos, F);
  if (bad >= 0) {
    wct_set_error("guided upsample along time: the step from frame %d to %d is (%lld, %lld), must be within %d on both axes", bad, bad + 1,
                  (long long)pos[2 * bad + 2] - pos[2 * bad], (long long)pos[2 * bad + 3] - pos[2 * bad + 1], WCT_MOTION_MAX_RANGE);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

size_t guided_up_time_workspace_bytes(int F, int h, int w, int f0, int f1) {
  return ((size_t)F + (size_t)(f1 - f0)) * h * w * 6 * sizeof(int32_t);
}

int launch_guided_upsample_time(const uint8_t* stylized, const uint8_t* content_small, const uint8_t* content_full, int F, int h, int w,
                                int hc, int wc, int H, int W, int radius, int eps_q, int frames_t, const int32_t* pos, int f0, int f1,
                                void* workspace, uint8_t* out, hipStream_t st) {
  ARG_CHECK(stylized && content_small && content_full && workspace && out);
  int rc = guided_up_time_check(F, h, w, hc, wc, H, W, radius, eps_q, frames_t, f0, f1, pos);
  if (rc) return rc;
  int32_t* ab = (int32_t*)workspace;
  int32_t* mean = ab + (size_t)F * h * w * 6;
  rc = pos ? launch_guided_motion_ab(stylized, content_small, F, h, w, hc, wc, radius, eps_q, frames_t, pos, f0, f1, ab, st)
           : launch_guided_time_ab(stylized, content_small, F, h, w, hc, wc, radius, eps_q, frames_t, f0, f1, ab, st);
  if (rc) return rc;
  UpPos mp;
  for (int f = 0; f < 32; ++f)                                // relative to frame 0: |p| <= 16 * 31; all zero without positions
    for (int k = 0; k < 2; ++k) mp.p[f][k] = pos && f < F ? (int32_t)((int64_t)pos[2 * f + k] - pos[k]) : 0;
  const int strips = cdiv(w, NT - 2 * radius), segs = cdiv(h, SEG);
  hipLaunchKernelGGL(guided_up_time_mean_kernel, dim3((unsigned)(f1 - f0) * strips * segs), dim3(NT), 0, st, (const int32_t*)ab, mean, mp, F,
                     frames_t, f0, h, w, radius, strips, segs);
  HIP_TRY(hipGetLastError());
  return launch_guided_up_full(mean, content_full, out, f1 - f0, H, W, h, w, hc, wc, st);
}
