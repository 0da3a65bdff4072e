// Temporal guided smoothing along camera motion (guided_motion_rule.h): the two passes of guided_time.hip with the window of every
// neighbouring frame shifted by one global integer translation per frame, and the estimator of those translations.
// The filter, two launches for frames f0 .. f1 - 1 of a clip of up to 32 resident frames, on the tiling of guided_time.hip
// (guided_tile.h: 256 threads, strips of 256 - 2r columns, 64-row segments; the same two frame ranges):
//   pass 1: s [F][H][W][3] uint8 + c [F][Hc][Wc][3] uint8 -> ab [F][H][W][3][2] int32
//   pass 2: ab + c -> out [f1 - f0][H][W][3] uint8; out may be s + f0 H W 3
// The positions travel by value (MotionPos).  What differs from guided_time.hip: thread column x reads column x + Dx of frame g, so
// "is a column of the frame" is a test per frame and a thread whose own x is outside [0, W) still accumulates; the row step runs
// over every y of [y0 - r, y1 + r) and each frame tests its own y + Dy against [0, H); n is a sum over the frames.  Every read is
// behind its frame's bounds test: no position can read outside a frame.  Pass-1 sums mod 2^32, pass-2 sums int64, as there.
// The estimator, three launches for a clip:
//   guide planes: c -> I [F][Hc][Wc] uint8
//   SAD: a block per (pair, dy, row band) stages a chunk of row y of I_f and of row y + dy of I_{f+1} in LDS; every thread serves
//        all dx candidates for its own even columns; int64 (SAD, cnt) per (pair, candidate, band).  No atomics.
//   finish: a block per pair sums the bands and takes the arg-min by wct_motion_better -> the step d [F - 1][2] int32
#include "guided_tile.h"
#include "guided_motion_rule.h"

namespace {
struct MotionPos { int32_t p[32][2]; };

struct Span { int lo, hi; };
__device__ __forceinline__ Span span(int f, int F, int T) { return Span{f - T < 0 ? 0 : f - T, f + T > F - 1 ? F - 1 : f + T}; }

// The shifts (Dy, Dx) of the frames of the span of f, read from the by-value positions once per block: the same for every thread,
// so they sit in scalar registers, and the loops over them are unrolled (NF is the longest span).
constexpr int NF = 2 * WCT_GUIDED_TIME_MAX_FRAMES + 1;
struct Shifts { int n, dy[NF], dx[NF]; };
__device__ __forceinline__ Shifts shifts(const MotionPos& mp, int f, Span sp) {
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

// n of (f, y, x): wct_guided_motion_n on those shifts
__device__ __forceinline__ int64_t window_n(const Shifts& sh, int y, int H, int x, int W, int r) {
  int64_t n = 0;
#pragma unroll
  for (int k = 0; k < NF; ++k)
    if (k < sh.n) n += (int64_t)(wct_motion_extent(y + sh.dy[k], H, r) * wct_motion_extent(x + sh.dx[k], W, r));
  return n;
}

// g0: the clip frame of the grid's first blocks (place() counts frames from it)
__global__ __launch_bounds__(NT) void guided_motion_ab_kernel(const uint8_t* s, const uint8_t* c, int32_t* ab, MotionPos mp, int F, int T,
                                                              int g0, int H, int W, int Hc, int Wc, int r, int eps_q, int strips, int segs) {
  __shared__ unsigned P[8][NT];
  __shared__ unsigned tot[8][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const Shifts sh = shifts(mp, f, sp_f);
  const size_t sframe = (size_t)H * W * 3, cframe = (size_t)Hc * Wc * 3;
  // the column's window sums SI, SII, Sp[3], SIp[3] over the shifted columns of the span: true values below 2^31, kept mod 2^32
  unsigned v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto row = [&](int y, bool add) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int yy = y + sh.dy[k], xx = x + sh.dx[k];
      if (k >= sh.n || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;     // not a pixel of frame lo + k
      const uint8_t* sp = s + (sp_f.lo + k) * sframe + ((size_t)yy * W + xx) * 3;
      const uint8_t* cp = c + (sp_f.lo + k) * cframe + ((size_t)(yy < Hc ? yy : Hc - 1) * Wc + (xx < Wc ? xx : Wc - 1)) * 3;
      const unsigned I = (unsigned)wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
      unsigned d[8] = {I, I * I, sp[0], sp[1], sp[2], I * sp[0], I * sp[1], I * sp[2]};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += add ? d[j] : 0u - d[j];
    }
  };
  for (int y = pl.y0 - r; y < pl.y0 + r; ++y) row(y, true);                  // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    row(y + r, true);
    if (y > pl.y0) row(y - r - 1, false);
    unsigned w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = v[k];
    block_prefix<unsigned, 8>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = (int64_t)(P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0u));
    const int64_t n = window_n(sh, y, H, x, W, r);
    int32_t o[6];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) wct_guided_ab(n, S[0], S[1], S[2 + ch], S[5 + ch], eps_q, &o[2 * ch], &o[2 * ch + 1]);
    int32_t* op = ab + (((size_t)f * H + y) * W + x) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) op[k] = o[k];
  }
}

// g0 = f0: block frame b is clip frame f0 + b and frame b of out
__global__ __launch_bounds__(NT) void guided_motion_out_kernel(const int32_t* ab, const uint8_t* c, uint8_t* out, MotionPos mp, int F, int T,
                                                               int g0, int H, int W, int Hc, int Wc, int r, int strips, int segs) {
  __shared__ long long P[6][NT];
  __shared__ long long tot[6][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const Shifts sh = shifts(mp, f, sp_f);
  const size_t aframe = (size_t)H * W * 6;
  const uint8_t* cb = c + (size_t)f * Hc * Wc * 3;
  long long v[6] = {0, 0, 0, 0, 0, 0};                      // the column's window sums of (a_q, b_q) per channel over the span
  auto row = [&](int y, bool add) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int yy = y + sh.dy[k], xx = x + sh.dx[k];
      if (k >= sh.n || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const int32_t* p = ab + (sp_f.lo + k) * aframe + ((size_t)yy * W + xx) * 6;
#pragma unroll
      for (int j = 0; j < 6; ++j) v[j] += add ? (long long)p[j] : -(long long)p[j];
    }
  };
  for (int y = pl.y0 - r; y < pl.y0 + r; ++y) row(y, true);
  for (int y = pl.y0; y < pl.y1; ++y) {
    row(y + r, true);
    if (y > pl.y0) row(y - r - 1, false);
    long long w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = v[k];
    block_prefix<long long, 6>(w, P, tot);
    if (!pl.owner) continue;
    const uint8_t* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + (x < Wc ? x : Wc - 1)) * 3;
    const int I = wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
    const int64_t n = window_n(sh, y, H, x, W, r);
    uint8_t* op = out + (((size_t)pl.b * H + y) * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t SA = P[2 * ch][t + r] - (t - r - 1 >= 0 ? P[2 * ch][t - r - 1] : 0);
      const int64_t SB = P[2 * ch + 1][t + r] - (t - r - 1 >= 0 ? P[2 * ch + 1][t - r - 1] : 0);
      op[ch] = wct_guided_out(n, SA, SB, I);
    }
  }
}

// ---- the estimator ------------------------------------------------------------------------------------------------------------
constexpr int CH = 1024;                                    // columns of a staged chunk: 2 even columns per thread
constexpr int ND = 2 * WCT_MOTION_MAX_RANGE + 1;            // dx candidates at the largest range

__global__ __launch_bounds__(NT) void motion_guide_kernel(const uint8_t* c, uint8_t* planes, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= pixels) return;
  const uint8_t* p = c + i * 3;
  planes[i] = (uint8_t)wct_guided_guide(p[0], p[1], p[2]);
}

// the even y of [lo, hi] (0 <= lo), 0 when empty
__device__ __forceinline__ int evens(int lo, int hi) { return hi >= lo ? hi / 2 - (lo + 1) / 2 + 1 : 0; }

// part [pairs][(2R + 1)^2][nbands][2] int64: (SAD, cnt) of the band's rows; band_rows is even.  A thread's sums are below 2^32: it
// sees at most (band_rows / 2)(Wc / 512 + 1) samples of at most 255 (motion_band_rows keeps that under 2^24 samples)
__global__ __launch_bounds__(NT) void motion_sad_kernel(const uint8_t* planes, long long* part, int Hc, int Wc, int R, int band_rows,
                                                        int nbands) {
  __shared__ uint8_t A[CH], B[CH + 2 * WCT_MOTION_MAX_RANGE];
  __shared__ unsigned red[ND][NW];
  const int t = threadIdx.x, nd = 2 * R + 1;
  int id = blockIdx.x;
  const int band = id % nbands; id /= nbands;
  const int dyi = id % nd, pair = id / nd, dy = dyi - R;
  const size_t plane = (size_t)Hc * Wc;
  const uint8_t* I0 = planes + pair * plane;
  const uint8_t* I1 = I0 + plane;
  const int y_lo = band * band_rows, y_hi = y_lo + band_rows < Hc ? y_lo + band_rows : Hc;
  unsigned acc[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) acc[k] = 0;
  for (int y = y_lo; y < y_hi; y += 2) {
    const int yy = y + dy;
    if (yy < 0 || yy >= Hc) continue;                       // (the same for the whole block)
    const uint8_t* r0 = I0 + (size_t)y * Wc;
    const uint8_t* r1 = I1 + (size_t)yy * Wc;
    for (int x0 = 0; x0 < Wc; x0 += CH) {
      __syncthreads();                                      // the chunk before this one has been read
      for (int i = t; i < CH; i += NT) A[i] = x0 + i < Wc ? r0[x0 + i] : 0;
      for (int i = t; i < CH + 2 * R; i += NT) {            // B[i] is column x0 - R + i
        const int xx = x0 - R + i;
        B[i] = xx >= 0 && xx < Wc ? r1[xx] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < CH / 2 / NT; ++j) {
        const int xl = 2 * (t + NT * j), x = x0 + xl;
        if (x >= Wc) continue;
        const int a = A[xl];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          const int xx = x + k - R;
          if (k < nd && xx >= 0 && xx < Wc) {
            const int v = a - (int)B[xl + k];
            acc[k] += (unsigned)(v < 0 ? -v : v);
          }
        }
      }
    }
  }
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    unsigned a = acc[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
    if (lane == 0) red[k][wave] = a;
  }
  __syncthreads();
  if (t < nd) {
    long long sad = 0;
    for (int w = 0; w < NW; ++w) sad += red[t][w];
    const int lo = y_lo > -dy ? y_lo : -dy, hi = y_hi - 1 < Hc - 1 - dy ? y_hi - 1 : Hc - 1 - dy;
    long long* o = part + (((size_t)pair * nd * nd + (size_t)dyi * nd + t) * nbands + band) * 2;
    o[0] = sad;
    o[1] = (long long)evens(lo, hi) * wct_motion_samples(t - R, Wc);
  }
}

// steps [pairs][2] int32: the winner of every pair
__global__ __launch_bounds__(NT) void motion_finish_kernel(const long long* part, int32_t* steps, int R, int nbands) {
  __shared__ long long bs[NT], bc[NT];
  __shared__ int by[NT], bx[NT];
  const int t = threadIdx.x, nd = 2 * R + 1, pair = blockIdx.x;
  // every thread starts from candidate (0, 0) -- its own best is that or one that wins over it
  long long s0 = 0, c0 = 0;
  {
    const long long* p = part + (((size_t)pair * nd * nd + (size_t)R * nd + R) * nbands) * 2;
    for (int b = 0; b < nbands; ++b) { s0 += p[2 * b]; c0 += p[2 * b + 1]; }
  }
  long long s = s0, n = c0;
  int dy = 0, dx = 0;
  for (int k = t; k < nd * nd; k += NT) {
    const long long* p = part + (((size_t)pair * nd * nd + k) * nbands) * 2;
    long long ks = 0, kc = 0;
    for (int b = 0; b < nbands; ++b) { ks += p[2 * b]; kc += p[2 * b + 1]; }
    const int ky = k / nd - R, kx = k % nd - R;
    if (wct_motion_better(ks, kc, ky, kx, s, n, dy, dx)) { s = ks; n = kc; dy = ky; dx = kx; }
  }
  bs[t] = s; bc[t] = n; by[t] = dy; bx[t] = dx;
  __syncthreads();
  for (int h = NT / 2; h >= 1; h >>= 1) {
    if (t < h && wct_motion_better(bs[t + h], bc[t + h], by[t + h], bx[t + h], bs[t], bc[t], by[t], bx[t])) {
      bs[t] = bs[t + h]; bc[t] = bc[t + h]; by[t] = by[t + h]; bx[t] = bx[t + h];
    }
    __syncthreads();
  }
  if (t == 0) { steps[2 * pair] = by[0]; steps[2 * pair + 1] = bx[0]; }
}

// rows of a band: 64 up to 4096 rows, then as many (even) as keep the bands at 64
int motion_band_rows(int Hc) { return Hc <= 64 * SEG ? SEG : 2 * cdiv(Hc, 2 * 64); }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
}  // namespace

int guided_motion_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1, const int32_t* pos) {
  int rc = guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1);
  if (rc) return rc;
  if (!pos) { wct_set_error("guided filter along motion: null positions"); return WCT_ERR_ARG; }
  const int bad = wct_motion_bad_step(pos, F);
  if (bad >= 0) {
    wct_set_error("guided filter along motion: the step from frame %d to %d is (%lld, %lld), must be within %d on both axes", bad, bad + 1,
                  (long long)pos[2 * bad + 2] - pos[2 * bad], (long long)pos[2 * bad + 3] - pos[2 * bad + 1], WCT_MOTION_MAX_RANGE);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

int launch_guided_motion(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                         int frames_t, const int32_t* pos, int f0, int f1, void* workspace, uint8_t* out, hipStream_t st) {
  ARG_CHECK(stylized && content && workspace && out);
  int rc = guided_motion_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos);
  if (rc) return rc;
  MotionPos mp;
  for (int f = 0; f < 32; ++f)                                // relative to frame 0: |p| <= 16 * 31
    for (int k = 0; k < 2; ++k) mp.p[f][k] = f < F ? (int32_t)((int64_t)pos[2 * f + k] - pos[k]) : 0;
  const int H = Ho, W = Wo, r = radius, T = frames_t;
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const int g0 = f0 - T < 0 ? 0 : f0 - T, g1 = f1 + T > F ? F : f1 + T;    // the frames whose coefficients pass 2 reads
  hipLaunchKernelGGL(guided_motion_ab_kernel, dim3((unsigned)(g1 - g0) * strips * segs), dim3(NT), 0, st, stylized, content,
                     (int32_t*)workspace, mp, F, T, g0, H, W, Hc, Wc, r, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(guided_motion_out_kernel, dim3((unsigned)(f1 - f0) * strips * segs), dim3(NT), 0, st, (const int32_t*)workspace, content,
                     out, mp, F, T, f0, H, W, Hc, Wc, r, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_guided_motion_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                            int frames_t, const int32_t* pos, int f0, int f1, int32_t* ab, hipStream_t st) {
  ARG_CHECK(stylized && content && ab);
  int rc = guided_motion_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos);
  if (rc) return rc;
  MotionPos mp;
  for (int f = 0; f < 32; ++f)
    for (int k = 0; k < 2; ++k) mp.p[f][k] = f < F ? (int32_t)((int64_t)pos[2 * f + k] - pos[k]) : 0;
  const int strips = cdiv(Wo, NT - 2 * radius), segs = cdiv(Ho, SEG);
  const int g0 = f0 - frames_t < 0 ? 0 : f0 - frames_t, g1 = f1 + frames_t > F ? F : f1 + frames_t;
  hipLaunchKernelGGL(guided_motion_ab_kernel, dim3((unsigned)(g1 - g0) * strips * segs), dim3(NT), 0, st, stylized, content, ab, mp, F,
                     frames_t, g0, Ho, Wo, Hc, Wc, radius, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int motion_check(int F, int Hc, int Wc, int range) {
  if (F < 1 || F > 32) { wct_set_error("global motion: a clip of F = %d frames, must be 1 .. 32", F); return WCT_ERR_ARG; }
  if (range < 1 || range > WCT_MOTION_MAX_RANGE) {
    wct_set_error("global motion: a search range of %d, must be 1 .. %d", range, WCT_MOTION_MAX_RANGE);
    return WCT_ERR_ARG;
  }
  if (Hc < 4 * range || Wc < 4 * range) {
    wct_set_error("global motion: %dx%d content for a search range of %d, both sides must be at least 4 range = %d", Hc, Wc, range,
                  4 * range);
    return WCT_ERR_ARG;
  }
  if ((long long)Hc * Wc > WCT_MOTION_MAX_PIXELS) {
    wct_set_error("global motion: %dx%d content passes 2^28 pixels", Hc, Wc);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

size_t motion_workspace_bytes(int F, int Hc, int Wc, int range) {
  const size_t nd = 2 * (size_t)range + 1, nbands = cdiv(Hc, motion_band_rows(Hc)), pairs = F - 1;
  return align16((size_t)F * Hc * Wc) + pairs * nd * nd * nbands * 16 + pairs * 8;
}

int launch_motion_global(const uint8_t* content, int F, int Hc, int Wc, int range, void* workspace, const int32_t** steps, hipStream_t st) {
  ARG_CHECK(content && workspace && steps);
  int rc = motion_check(F, Hc, Wc, range);
  if (rc) return rc;
  const int nd = 2 * range + 1, band_rows = motion_band_rows(Hc), nbands = cdiv(Hc, band_rows), pairs = F - 1;
  const size_t pixels = (size_t)F * Hc * Wc;
  uint8_t* planes = (uint8_t*)workspace;
  long long* part = (long long*)(planes + align16(pixels));
  int32_t* d = (int32_t*)(part + (size_t)pairs * nd * nd * nbands * 2);
  *steps = d;
  if (!pairs) return WCT_OK;
  hipLaunchKernelGGL(motion_guide_kernel, dim3((unsigned)((pixels + NT - 1) / NT)), dim3(NT), 0, st, content, planes, pixels);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(motion_sad_kernel, dim3((unsigned)(pairs * nd * nbands)), dim3(NT), 0, st, (const uint8_t*)planes, part, Hc, Wc, range,
                     band_rows, nbands);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)pairs), dim3(NT), 0, st, (const long long*)part, d, range, nbands);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
