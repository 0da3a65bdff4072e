// Temporal guided smoothing (guided_time_rule.h): the guided filter of guided.hip with its box extended over the T frames on each
// side of a frame of a clip resident on the device -- two launches for frames f0 .. f1 - 1 of a clip of up to 32 frames.
//   pass 1: s [F][H][W][3] uint8 + c [F][Hc][Wc][3] (uint8, or fp32 in [0,1] quantised by wct_quantise_u8) -> ab [F][H][W][3][2]
//           int32, the (a_q, b_q) of every pixel and channel of frames max(0, f0 - T) .. min(F, f1 + T) - 1: those pass 2 reads,
//           each at its own position in the clip
//   pass 2: ab + c -> out [f1 - f0][H][W][3] uint8; out may be s + f0 H W 3 (pass 1 has consumed s before pass 2 writes)
// The tiling, the prefix sums and the window difference are those of guided.hip (guided_tile.h): a block owns SEG rows of a strip
// of one frame and a thread keeps its column's vertical window sums in registers.  Here the sums run over the frames of the
// block's time window as well: the row step adds (or subtracts) row y of each of them into the same registers, so the scans and
// the divisions of a pixel do not grow with T, only the loads do (the luma of a content pixel is recomputed 2T + 1 times).
// Pass 1's sums are below 2^31 per window (wct_guided_time_params_ok) and are kept mod 2^32; pass 2's are int64.
#include "guided_tile.h"
#include "guided_time_rule.h"

namespace {
// the frames of the time window of clip frame f
struct Span { int lo, hi; };
__device__ __forceinline__ Span span(int f, int F, int T) { return Span{f - T < 0 ? 0 : f - T, f + T > F - 1 ? F - 1 : f + T}; }

// g0: the clip frame of the grid's first blocks (place() counts frames from it)
template <typename CT>
__global__ __launch_bounds__(NT) void guided_time_ab_kernel(const uint8_t* s, const CT* c, int32_t* ab, int F, int T, int g0, int H, int W,
                                                            int Hc, int Wc, int r, int eps_q, int strips, int segs) {
  __shared__ unsigned P[8][NT];
  __shared__ unsigned tot[8][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const size_t sframe = (size_t)H * W * 3, cframe = (size_t)Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  // the column's window sums SI, SII, Sp[3], SIp[3] over the frames of the span: true values below 2^31, kept mod 2^32
  unsigned v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const uint8_t* sp = s + sp_f.lo * sframe + ((size_t)y * W + x) * 3;
    const CT* cp = c + sp_f.lo * cframe + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    for (int g = sp_f.lo; g <= sp_f.hi; ++g, sp += sframe, cp += cframe) {
      const unsigned I = (unsigned)wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
      unsigned d[8] = {I, I * I, sp[0], sp[1], sp[2], I * sp[0], I * sp[1], I * sp[2]};
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += add ? d[k] : 0u - d[k];
    }
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);    // the window of y0 but its last row
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    unsigned w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = v[k];
    block_prefix<unsigned, 8>(w, P, tot);
    if (!pl.owner) continue;                                // (every thread has passed both barriers of the row)
    int64_t S[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = (int64_t)(P[k][t + r] - (t - r - 1 >= 0 ? P[k][t - r - 1] : 0u));
    const int64_t n = wct_guided_time_n(f, F, T, y, H, x, W, r);
    int32_t o[6];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) wct_guided_ab(n, S[0], S[1], S[2 + ch], S[5 + ch], eps_q, &o[2 * ch], &o[2 * ch + 1]);
    int32_t* op = ab + (((size_t)f * H + y) * W + x) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) op[k] = o[k];
  }
}

// g0 = f0: block frame b is clip frame f0 + b and frame b of out
template <typename CT>
__global__ __launch_bounds__(NT) void guided_time_out_kernel(const int32_t* ab, const CT* c, uint8_t* out, int F, int T, int g0, int H, int W,
                                                             int Hc, int Wc, int r, int strips, int segs) {
  __shared__ long long P[6][NT];
  __shared__ long long tot[6][NW];
  const Place pl = place(H, W, r, strips, segs);
  const int t = threadIdx.x, x = pl.x, f = g0 + pl.b;
  const Span sp_f = span(f, F, T);
  const size_t aframe = (size_t)H * W * 6;
  const CT* cb = c + (size_t)f * Hc * Wc * 3;
  const int xc = x < Wc ? x : Wc - 1;
  long long v[6] = {0, 0, 0, 0, 0, 0};                      // the column's window sums of (a_q, b_q) per channel over the span
  auto row = [&](int y, bool add) {
    if (!pl.col) return;
    const int32_t* p = ab + sp_f.lo * aframe + ((size_t)y * W + x) * 6;
    for (int g = sp_f.lo; g <= sp_f.hi; ++g, p += aframe) {
#pragma unroll
      for (int k = 0; k < 6; ++k) v[k] += add ? (long long)p[k] : -(long long)p[k];
    }
  };
  for (int y = pl.y0 - r < 0 ? 0 : pl.y0 - r; y < pl.y0 + r && y < H; ++y) row(y, true);
  for (int y = pl.y0; y < pl.y1; ++y) {
    if (y + r < H) row(y + r, true);
    if (y > pl.y0 && y - r - 1 >= 0) row(y - r - 1, false);
    long long w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = v[k];
    block_prefix<long long, 6>(w, P, tot);
    if (!pl.owner) continue;
    const CT* cp = cb + ((size_t)(y < Hc ? y : Hc - 1) * Wc + xc) * 3;
    const int I = wct_guided_guide(sample(cp), sample(cp + 1), sample(cp + 2));
    const int64_t n = wct_guided_time_n(f, F, T, y, H, x, W, r);
    uint8_t* op = out + (((size_t)pl.b * H + y) * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t SA = P[2 * ch][t + r] - (t - r - 1 >= 0 ? P[2 * ch][t - r - 1] : 0);
      const int64_t SB = P[2 * ch + 1][t + r] - (t - r - 1 >= 0 ? P[2 * ch + 1][t - r - 1] : 0);
      op[ch] = wct_guided_out(n, SA, SB, I);
    }
  }
}

template <typename CT>
int launch(const uint8_t* s, const CT* c, int32_t* ab, int F, int H, int W, int Hc, int Wc, int r, int eps_q, int T, int f0, int f1,
           uint8_t* out, hipStream_t st) {
  const int strips = cdiv(W, NT - 2 * r), segs = cdiv(H, SEG);
  const int g0 = f0 - T < 0 ? 0 : f0 - T, g1 = f1 + T > F ? F : f1 + T;    // the frames whose coefficients pass 2 reads
  hipLaunchKernelGGL((guided_time_ab_kernel<CT>), dim3((unsigned)(g1 - g0) * strips * segs), dim3(NT), 0, st, s, c, ab, F, T, g0, H, W, Hc,
                     Wc, r, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((guided_time_out_kernel<CT>), dim3((unsigned)(f1 - f0) * strips * segs), dim3(NT), 0, st, (const int32_t*)ab, c, out, F,
                     T, f0, H, W, Hc, Wc, r, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

int guided_time_check(int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q, int frames_t, int f0, int f1) {
  if (F < 1 || F > 32) { wct_set_error("guided filter along time: a clip of F = %d frames, must be 1 .. 32", F); return WCT_ERR_ARG; }
  if (f0 < 0 || f1 <= f0 || f1 > F) {
    wct_set_error("guided filter along time: frames [%d, %d) of a clip of %d, must be 0 <= f0 < f1 <= F", f0, f1, F);
    return WCT_ERR_ARG;
  }
  if (Hc < 1 || Wc < 1 || Ho < Hc || Wo < Wc) {
    wct_set_error("guided filter along time: a %dx%d stylized frame for a %dx%d content (the frame is never the smaller one)", Ho, Wo, Hc,
                  Wc);
    return WCT_ERR_ARG;
  }
  if (frames_t < 0 || frames_t > WCT_GUIDED_TIME_MAX_FRAMES) {
    wct_set_error("guided filter along time: %d frames on each side, must be 0 .. %d", frames_t, WCT_GUIDED_TIME_MAX_FRAMES);
    return WCT_ERR_ARG;
  }
  if (!wct_guided_time_params_ok(radius, eps_q, frames_t)) {
    wct_set_error("guided filter along time: radius %d, eps_q %d with %d frames on each side; the radius is 1 .. %d for that many frames "
                  "((2 radius + 1)^2 (2 frames + 1) <= %d) and eps_q 1 .. %d (grey levels squared)", radius, eps_q, frames_t,
                  wct_guided_time_radius_limit(frames_t), WCT_GUIDED_TIME_MAX_WINDOW, WCT_GUIDED_MAX_EPS);
    return WCT_ERR_ARG;
  }
  if ((unsigned long long)F * (unsigned long long)Ho * (unsigned long long)Wo * 3ull >= (1ull << 31)) {
    wct_set_error("guided filter along time: %d frames of %dx%dx3 pass 2^31 bytes in one call", F, Ho, Wo);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

int guided_time_max_radius(int frames_t) { return wct_guided_time_radius_limit(frames_t); }

int launch_guided_time_ab(const uint8_t* stylized, const uint8_t* content, int F, int Ho, int Wo, int Hc, int Wc, int radius, int eps_q,
                          int frames_t, int f0, int f1, int32_t* ab, hipStream_t s) {
  ARG_CHECK(stylized && content && ab);
  int rc = guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1);
  if (rc) return rc;
  const int strips = cdiv(Wo, NT - 2 * radius), segs = cdiv(Ho, SEG);
  const int g0 = f0 - frames_t < 0 ? 0 : f0 - frames_t, g1 = f1 + frames_t > F ? F : f1 + frames_t;
  hipLaunchKernelGGL((guided_time_ab_kernel<uint8_t>), dim3((unsigned)(g1 - g0) * strips * segs), dim3(NT), 0, s, stylized, content, ab, F,
                     frames_t, g0, Ho, Wo, Hc, Wc, radius, eps_q, strips, segs);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}

int launch_guided_time(const uint8_t* stylized, const void* content, int content_f32, int F, int Ho, int Wo, int Hc, int Wc, int radius,
                       int eps_q, int frames_t, int f0, int f1, void* workspace, uint8_t* out, hipStream_t s) {
  ARG_CHECK(stylized && content && workspace && out);
  int rc = guided_time_check(F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1);
  if (rc) return rc;
  if (content_f32)
    return launch(stylized, (const float*)content, (int32_t*)workspace, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, out, s);
  return launch(stylized, (const uint8_t*)content, (int32_t*)workspace, F, Ho, Wo, Hc, Wc, radius, eps_q, frames_t, f0, f1, out, s);
}
