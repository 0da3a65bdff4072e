// Temporal guided smoothing with the colour guide (guided_color_time_rule.h): the 21 sums and the 3 x 3 solve of guided_color.hip
// over the 3-D shifted window of guided_motion.hip.  Two launches for frames f0 .. f1 - 1 of a clip of up to 32 resident frames, on
// the tiling of guided_tile.h (256 threads, strips of 256 - 2r columns, 64-row segments):
//   pass 1: s [F][H][W][3] uint8 + c [F][Hc][Wc][3] uint8 -> ab [F][H][W][12] int32 (48 B per pixel, three 16-byte stores, a
//           16-byte aligned base), for the frames max(0, f0 - T) .. min(F, f1 + T) - 1 whose coefficients pass 2 reads
//   pass 2: ab + c -> out [f1 - f0][H][W][3] uint8; out may be s + f0 H W 3 (pass 1 has consumed every frame before pass 2 writes)
// Structure as guided_motion.hip: the positions travel by value (MotionPos), the shifts of a block's span sit in scalar registers,
// thread column x reads column x + Dx of frame g, the row step runs over every y of [y0 - r, y1 + r) and every read is behind its
// own frame's bounds test, so no position can read outside a frame.  Pass 1 keeps the 21 unsigned column sums mod 2^32 (the true
// window sums are below 2^31, guided_color_time_rule.h), pass 2 twelve int64 sums read as int4; halo threads leave the row before
// the solve.  One pair of kernels serves "no motion" (all positions zero) and motion: equal positions are the no-motion rule by
// construction.
#include "guided_tile.h"
#include "guided_color_time_rule.h"

namespace {
constexpr int KS = WCT_GUIDED_COLOR_SUMS, KC = WCT_GUIDED_COLOR_COEFFS;

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
__global__ __launch_bounds__(NT) void guided_color_time_ab_kernel(const uint8_t* s, const uint8_t* c, int32_t* ab, MotionPos mp, int F, int T,
                                                                  int g0, int H, int W, int Hc, int Wc, int r, int eps_q, int strips,
                                                                  int segs) {
  __shared__ unsigned P[KS][NT];
  __shared__ unsigned tot[KS][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const Shifts sh = shifts(mp, f, sp_f);
  const size_t sframe = (size_t)H * W * 3, cframe = (size_t)Hc * Wc * 3;
  unsigned v[KS];                                           // the column's window sums over the span: true values below 2^31, mod 2^32
#pragma unroll
  for (int k = 0; k < KS; ++k) v[k] = 0;
  auto row = [&](int y, bool add) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int yy = y + sh.dy[k], xx = x + sh.dx[k];
      if (k >= sh.n || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;     // not a pixel of frame lo + k
      const uint8_t* sp = s + (sp_f.lo + k) * sframe + ((size_t)yy * W + xx) * 3;
      const uint8_t* cp = c + (sp_f.lo + k) * cframe + ((size_t)(yy < Hc ? yy : Hc - 1) * Wc + (xx < Wc ? xx : Wc - 1)) * 3;
      const int I[3] = {sample(cp), sample(cp + 1), sample(cp + 2)}, p[3] = {sp[0], sp[1], sp[2]};
      unsigned d[KS];
      wct_guided_color_terms(I, p, d);
#pragma unroll
      for (int j = 0; j < KS; ++j) v[j] += add ? d[j] : 0u - d[j];
    }
  };
  for (int y = pl.y0 - r; y < pl.y0 + r; ++y) row(y, true);                  // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    row(y + r, true);
    if (y > pl.y0) row(y - r - 1, false);
    unsigned w[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) w[k] = v[k];
    block_prefix<unsigned, KS>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) S[k] = (int64_t)(P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0u));
    const int64_t n = window_n(sh, y, H, x, W, r);
    int32_t o[KC];
    wct_guided_color_ab(n, S, eps_q, o, nullptr);
    int4* op = reinterpret_cast<int4*>(ab + (((size_t)f * H + y) * W + x) * KC);               // 48 B per pixel: 16-byte aligned
#pragma unroll
    for (int k = 0; k < KC / 4; ++k) op[k] = make_int4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
  }
}

// g0 = f0: block frame b is clip frame f0 + b and frame b of out
__global__ __launch_bounds__(NT) void guided_color_time_out_kernel(const int32_t* ab, const uint8_t* c, uint8_t* out, MotionPos mp, int F,
                                                                   int T, int g0, int H, int W, int Hc, int Wc, int r, int strips,
                                                                   int segs) {
  __shared__ long long P[KC][NT];
  __shared__ long long tot[KC][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const Shifts sh = shifts(mp, f, sp_f);
  const size_t aframe = (size_t)H * W * KC;
  const uint8_t* cb = c + (size_t)f * Hc * Wc * 3;
  long long v[KC];                                          // the column's window sums of the twelve coefficients over the span
#pragma unroll
  for (int k = 0; k < KC; ++k) v[k] = 0;
  auto row = [&](int y, bool add) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int yy = y + sh.dy[k], xx = x + sh.dx[k];
      if (k >= sh.n || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const int4* p = reinterpret_cast<const int4*>(ab + (sp_f.lo + k) * aframe + ((size_t)yy * W + xx) * KC);
#pragma unroll
      for (int q = 0; q < KC / 4; ++q) {
        const int4 a = p[q];
        const int e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * q + j] += add ? (long long)e[j] : -(long long)e[j];
      }
    }
  };
  for (int y = pl.y0 - r; y < pl.y0 + r; ++y) row(y, true);
  for (int y = pl.y0; y < pl.y1; ++y) {
    row(y + r, true);
    if (y > pl.y0) row(y - r - 1, false);
    long long w[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) w[k] = v[k];
    block_prefix<long long, KC>(w, P, tot);
    if (!pl.owner) continue;
    const uint8_t* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + (x < Wc ? x : Wc - 1)) * 3;
    const int I[3] = {sample(cp), sample(cp + 1), sample(cp + 2)};
    const int64_t n = window_n(sh, y, H, x, W, r);
    auto win = [&](int k) -> int64_t { return P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0); };
    uint8_t* op = out + (((size_t)pl.b * H + y) * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t SA[3] = {win(ch), win(3 + ch), win(6 + ch)};
      op[ch] = wct_guided_color_out(n, SA, win(9 + ch), I);
    }
  }
}

// pos == nullptr: no motion, every position zero
MotionPos positions(const int32_t* pos, int F) {
  MotionPos mp;
  for (int f = 0; f < 32; ++f)                                // relative to frame 0: |p| <= 16 * 31
    for (int k = 0; k < 2; ++k) mp.p[f][k] = pos && f < F ? (int32_t)((int64_t)pos[2 * f + k] - pos[k]) : 0;
  return mp;
}
}  // namespace

int guided_color_time_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1, const int32_t* pos) {
  return pos ? guided_motion_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos)
             : guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1);
}

int launch_guided_color_time_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                                int frames_t, const int32_t* pos, int f0, int f1, int32_t* ab, hipStream_t st) {
  ARG_CHECK(stylized && content && ab);
  if (((uintptr_t)ab & 15) != 0) {
    wct_set_error("guided filter along time: the colour guide's workspace must be 16-byte aligned");
    return WCT_ERR_ARG;
  }
  int rc = guided_color_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, pos);
  if (rc) return rc;
  const MotionPos mp = positions(pos, F);
  const int strips = cdiv(Wo, NT - 2 * radius), segs = cdiv(Ho, SEG);
  const int g0 = f0 - frames_t < 0 ? 0 : f0 - frames_t, g1 = f1 + frames_t > F ? F : f1 + frames_t;    // the frames pass 2 reads
  hipLaunchKernelGGL(guided_color_time_ab_kernel, dim3((unsigned)(g1 - g0) * strips * segs), dim3(NT), 0, st, stylized, content, ab, mp, F,
                     frames_t, g0, Ho, Wo, Hc, Wc, radius, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_guided_color_time(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                             int frames_t, const int32_t* pos, int f0, int f1, void* workspace, uint8_t* out, hipStream_t st) {
  ARG_CHECK(stylized && content && workspace && out);
  int rc = launch_guided_color_time_ab(stylized, content, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, pos, f0, f1, (int32_t*)workspace, st);
  if (rc) return rc;
  const MotionPos mp = positions(pos, F);
  const int strips = cdiv(Wo, NT - 2 * radius), segs = cdiv(Ho, SEG);
  hipLaunchKernelGGL(guided_color_time_out_kernel, dim3((unsigned)(f1 - f0) * strips * segs), dim3(NT), 0, st, (const int32_t*)workspace,
                     content, out, mp, F, frames_t, f0, Ho, Wo, Hc, Wc, radius, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
