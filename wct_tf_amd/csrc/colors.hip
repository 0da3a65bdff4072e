// Luminance-only colour preservation (colors_rule.h): the stylized luminance on the content's chrominance, per pixel.
//   fused:       fp32 decoded frame [B][Ho][Wo][3] + content (uint8 or fp32 in [0,1]) [B][Hc][Wc][3] -> uint8 frame -- the chain's
//                last launch in the place of f32_to_u8_kernel (WCT_FLAG_CONTENT_COLORS); both inputs are quantised by that
//                kernel's rule first, so the frame equals the stand-alone op on the unflagged frame, bit for bit
//   stand-alone: uint8 stylized + uint8 content -> uint8, in place if asked (a lane reads its pixels before it writes them)
//                (behind the guided filter of a stylize call the content is the call's: uint8, or fp32 quantised as above)
// Output pixel (y, x) takes content pixel (min(y, Hc - 1), min(x, Wc - 1)): the clamp of the label maps (a frame can be larger
// than its content, wct_output_size).  HBM-bound byte streams: a lane owns PX = 4 consecutive pixels of one row = 12 samples
// = three 16-byte loads of the fp32 frame (three dwords of a uint8 one) and three dword stores, when the rows keep that
// alignment (W % 4 == 0 and an aligned base); otherwise, and for a group that reaches past the row or past the content's last
// column, sample by sample.  A row below the content's last one reads that row: contiguous, so it keeps the wide path.
#include "common.h"
#include "colors_rule.h"

namespace {
constexpr int PX = 4;                 // pixels per lane
constexpr int NS = 3 * PX;            // samples per lane
constexpr int MAX_BLOCKS = 1024;      // grid cap (4 blocks of 256 per CU); the rest is grid-strided

__device__ __forceinline__ int sample(const uint8_t* p) { return *p; }
__device__ __forceinline__ int sample(const float* p) { return wct_quantise_u8(*p); }

// NS consecutive samples from p; wide: p is 16-byte (fp32) / 4-byte (uint8) aligned
__device__ __forceinline__ void load_group(const float* p, bool wide, int v[NS]) {
  if (wide) {
#pragma unroll
    for (int k = 0; k < NS / 4; ++k) {
      const f32x4 t = ((const f32x4*)p)[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = wct_quantise_u8(t[j]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = sample(p + i);
  }
}
__device__ __forceinline__ void load_group(const uint8_t* p, bool wide, int v[NS]) {
  if (wide) {
#pragma unroll
    for (int k = 0; k < NS / 4; ++k) {
      const unsigned t = ((const unsigned*)p)[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = (t >> (8 * j)) & 255u;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i] = p[i];
  }
}

// s [B][Ho][Wo][3], c [B][Hc][Wc][3], out [B][Ho][Wo][3]; Ho >= Hc, Wo >= Wc.  s_wide / c_wide / o_wide: the rows of that
// array keep the alignment of the wide accesses (the same in every lane: the branches are uniform)
template <typename ST, typename CT>
__global__ __launch_bounds__(256) void content_colors_kernel(const ST* s, const CT* c, uint8_t* out, int B, int Ho, int Wo, int Hc,
                                                             int Wc, int s_wide, int c_wide, int o_wide) {
  const int G = (Wo + PX - 1) / PX;                       // groups per row
  const size_t items = (size_t)B * Ho * G;
  for (size_t it = blockIdx.x * (size_t)blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(it % G);
    const size_t row = it / G;                            // b * Ho + y
    const int y = (int)(row % Ho);
    const size_t b = row / Ho;
    const int x0 = g * PX;
    const size_t so = (row * Wo + x0) * 3;
    const CT* crow = c + (b * Hc + (y < Hc ? y : Hc - 1)) * (size_t)Wc * 3;
    if (x0 + PX <= Wc) {                                  // PX whole pixels with their own content pixels (Wc <= Wo)
      int sv[NS], cv[NS];
      load_group(s + so, s_wide != 0, sv);
      load_group(crow + (size_t)x0 * 3, c_wide != 0, cv);
      uint8_t o[NS];
#pragma unroll
      for (int j = 0; j < PX; ++j)
        wct_content_colors_px(sv[3 * j], sv[3 * j + 1], sv[3 * j + 2], cv[3 * j], cv[3 * j + 1], cv[3 * j + 2], o + 3 * j);
      if (o_wide) {
#pragma unroll
        for (int k = 0; k < NS / 4; ++k)
          ((unsigned*)(out + so))[k] = (unsigned)o[4 * k] | ((unsigned)o[4 * k + 1] << 8) | ((unsigned)o[4 * k + 2] << 16) |
                                       ((unsigned)o[4 * k + 3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) out[so + i] = o[i];
      }
    } else {                                              // the row's tail and the columns past the content's last one
      const int n = Wo - x0 < PX ? Wo - x0 : PX;
      for (int j = 0; j < n; ++j) {
        const int x = x0 + j;
        const ST* sp = s + so + 3 * j;
        const CT* cp = crow + (size_t)(x < Wc ? x : Wc - 1) * 3;
        uint8_t o[3];
        wct_content_colors_px(sample(sp), sample(sp + 1), sample(sp + 2), sample(cp), sample(cp + 1), sample(cp + 2), o);
        out[so + 3 * j] = o[0]; out[so + 3 * j + 1] = o[1]; out[so + 3 * j + 2] = o[2];
      }
    }
  }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename ST, typename CT>
int launch(const ST* s, const CT* c, uint8_t* out, int B, int Ho, int Wo, int Hc, int Wc, hipStream_t st) {
  ARG_CHECK(s && c && out && B >= 1 && Hc >= 1 && Wc >= 1 && Ho >= Hc && Wo >= Wc);
  const size_t items = (size_t)B * Ho * ((Wo + PX - 1) / PX);
  size_t blocks = (items + 255) / 256;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  // a row starts Wo * 3 samples after the one before: every row keeps the base's alignment iff W % 4 == 0
  const int s_wide = Wo % 4 == 0 && aligned(s, sizeof(ST) * 4);
  const int c_wide = Wc % 4 == 0 && aligned(c, sizeof(CT) * 4);
  const int o_wide = Wo % 4 == 0 && aligned(out, 4);
  hipLaunchKernelGGL((content_colors_kernel<ST, CT>), dim3((unsigned)blocks), dim3(256), 0, st, s, c, out, B, Ho, Wo, Hc, Wc,
                     s_wide, c_wide, o_wide);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
}  // namespace

int launch_content_colors_f32(const float* frame, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                              uint8_t* out, hipStream_t s) {
  if (content_f32) return launch(frame, (const float*)content, out, B, Ho, Wo, Hc, Wc, s);
  return launch(frame, (const uint8_t*)content, out, B, Ho, Wo, Hc, Wc, s);
}

int launch_content_colors_u8(const uint8_t* stylized, const uint8_t* content, int B, int Ho, int Wo, int Hc, int Wc, uint8_t* out,
                             hipStream_t s) {
  return launch(stylized, content, out, B, Ho, Wo, Hc, Wc, s);
}

int launch_content_colors_u8_any(const uint8_t* stylized, const void* content, int content_f32, int B, int Ho, int Wo, int Hc, int Wc,
                                 uint8_t* out, hipStream_t s) {
  if (content_f32) return launch(stylized, (const float*)content, out, B, Ho, Wo, Hc, Wc, s);
  return launch(stylized, (const uint8_t*)content, out, B, Ho, Wo, Hc, Wc, s);
}
