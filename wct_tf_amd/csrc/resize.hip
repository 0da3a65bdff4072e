// Bilinear resize of B uint8 frames [B][H][W][3] -> [B][h][w][3] by the integer rule of resize_rule.h (Pillow's 8-bit resampler:
// along x into a uint8 intermediate, then along y), in ONE launch and without the intermediate ever reaching HBM.
// One block owns one frame's tile of `th` output rows x TILE_W output columns.  It first writes the horizontally resized bytes of
// the input rows its output rows tap -- ymin(first row) .. ymin(last row) + n(last row), the bounds being monotone -- into LDS,
// [row][column][channel] at a pitch of the tile's own 3 * columns bytes, then runs the vertical pass out of LDS.  Neighbouring
// row tiles recompute the few intermediate rows they share (the vertical support: 7 of ~71 rows at 1080 -> 512 with th = 32).
// The launcher picks th from TILE_HEIGHTS, the first whose tallest tile fits LDS_BYTES at the pitch of a full tile; a vertical
// reduction so strong that one output row's taps do not fit is refused.  LDS_BYTES is 16 KB, not the 64 KB a block could have:
// ten blocks then share a CU's 160 KB, and the frames this is for (1080 x 1920 -> 512 x 910: 71 rows of 192 bytes) keep th = 32.
// Pass 1 writes LDS bytes at consecutive addresses across a wave (four lanes a bank word); pass 2 reads, tap by tap, the 16
// consecutive bytes of a lane's group, the lanes of a row 16 bytes apart.
// A tile's output row is a span of 3 * columns bytes at any address: it is cut at the 16-byte boundaries of its ADDRESSES as
// noise.hip cuts its stream -- a lane whose group lies inside the span stores it with one aligned 16-byte vector store, the
// head and the tail of the span go out byte by byte, and only the bytes that are theirs.
// Microseconds beside the chain it feeds: the point is every byte right at every size, then not being wasteful.
#include "common.h"
#include "resize_rule.h"

#include <vector>

namespace {
constexpr int TILE_W = 64;                 // output columns of a tile: rows of 192 bytes, twelve whole groups
constexpr int LDS_BYTES = 16384;
constexpr int THREADS = 256;
constexpr int TILE_HEIGHTS[] = {32, 16, 8, 4, 2, 1};
constexpr int GROUP = 16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// tabs (device, int32): xb [w][2] | kx [w][ksx] | yb [h][2] | ky [h][ksy]
__global__ __launch_bounds__(THREADS) void resize_bilinear_kernel(const uint8_t* in, uint8_t* out, int H, int W, int h, int w,
                                                                  const int* tabs, int ksx, int ksy, int th, int tiles_x) {
  __shared__ __attribute__((aligned(16))) uint8_t mid[LDS_BYTES];
  const int* xb = tabs;
  const int* kx = xb + 2 * w;
  const int* yb = kx + w * ksx;
  const int* ky = yb + 2 * h;
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x), b = (int)blockIdx.y;
  const int x0 = tx * TILE_W, cols = min(TILE_W, w - x0);
  const int y0 = ty * th, rows_out = min(th, h - y0);
  const int span = cols * 3;                                 // bytes of an intermediate row, and of an output row, of this tile
  const int r0 = yb[2 * y0], y_last = y0 + rows_out - 1;
  const int rows = yb[2 * y_last] + yb[2 * y_last + 1] - r0;  // intermediate rows r0 .. r0 + rows - 1 (<= H); rows * span <= LDS_BYTES
  const uint8_t* src = in + b * H * W * 3;                   // (every product below 2^31: the launcher's check)

  // along x: the tile's columns of input rows r0 .. into LDS
  for (int i = threadIdx.x; i < rows * span; i += THREADS) {
    const int r = i / span, j = i - r * span, col = j / 3, ch = j - col * 3;
    const int xo = x0 + col, xmin = xb[2 * xo], n = xb[2 * xo + 1];
    mid[i] = wct_resize_byte(kx + xo * ksx, n, src + ((r0 + r) * W + xmin) * 3 + ch, 3);
  }
  __syncthreads();

  // along y: a lane owns the 16 bytes at (row span's address rounded down to 16) + 16 g, cut to the span
  const int groups = (span + 2 * GROUP - 2) / GROUP;         // what a span can touch at its worst alignment
  for (int it = threadIdx.x; it < rows_out * groups; it += THREADS) {
    const int ry = it / groups, g = it - ry * groups, y = y0 + ry;
    uint8_t* row = out + ((b * h + y) * w + x0) * 3;
    const int first = g * GROUP - (int)((uintptr_t)row & (GROUP - 1));
    const int lo = max(first, 0), hi = min(first + GROUP, span);
    if (lo >= hi) continue;
    const int n = yb[2 * y + 1];
    const int* k = ky + y * ksy;
    const uint8_t* m = mid + (yb[2 * y] - r0) * span;        // byte j of the span under tap x: m[x * span + j]
    if (hi - lo == GROUP) {                                  // a whole group: row + lo is 16-byte aligned
      unsigned word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < GROUP; ++q) word[q >> 2] |= (unsigned)wct_resize_byte(k, n, m + lo + q, span) << (8 * (q & 3));
      const u32x4 v = {word[0], word[1], word[2], word[3]};
      *(u32x4*)(row + lo) = v;
    } else {                                                 // the head or the tail: its own bytes, one by one
      for (int j = lo; j < hi; ++j) row[j] = wct_resize_byte(k, n, m + j, span);
    }
  }
}
}  // namespace

// every index of the kernel is a 32-bit one: a call whose input or output bytes pass 2^31 is refused, not wrapped
int resize_check_bytes(int B, int H, int W, int h, int w) {
  ARG_CHECK(B >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1);
  const unsigned long long limit = 1ull << 31;
  const unsigned long long px_in = (unsigned long long)H * (unsigned long long)W, px_out = (unsigned long long)h * (unsigned long long)w;
  if (px_in >= limit || px_out >= limit || px_in * 3ull * (unsigned)B >= limit || px_out * 3ull * (unsigned)B >= limit) {
    wct_set_error("resize: %d frames of %dx%dx3 to %dx%dx3 pass 2^31 bytes in one call", B, H, W, h, w);
    return WCT_ERR_ARG;
  }
  if (resize_table_ints(H, W, h, w) >= ((size_t)1 << 28)) {          // (an axis of hundreds of millions of pixels: the tables' own indices)
    wct_set_error("resize: the tap tables of %dx%d to %dx%d pass 2^28 words", H, W, h, w);
    return WCT_ERR_ARG;
  }
  return WCT_OK;
}

// the int32 words of a geometry's tables (about 2 W + 3 w + 2 H + 3 h)
size_t resize_table_ints(int H, int W, int h, int w) {
  return (size_t)w * (2 + wct_resize_ksize(W, w)) + (size_t)h * (2 + wct_resize_ksize(H, h));
}

// The plan of a geometry: the tables of both axes into tabs (resize_table_ints of them, the kernel's layout) and the tile height
int resize_plan(int H, int W, int h, int w, ResizeGeom* g, int* tabs) {
  ARG_CHECK(g && tabs && H >= 1 && W >= 1 && h >= 1 && w >= 1);
  const int ksx = wct_resize_ksize(W, w), ksy = wct_resize_ksize(H, h);
  std::vector<double> scratch((size_t)std::max(ksx, ksy));
  int* xb = tabs;
  int* kx = xb + 2 * (size_t)w;
  int* yb = kx + (size_t)w * ksx;
  int* ky = yb + 2 * (size_t)h;
  wct_resize_taps(W, w, xb, kx, scratch.data());
  wct_resize_taps(H, h, yb, ky, scratch.data());
  const int pitch = std::min(TILE_W, w) * 3;
  int th = 0;
  for (int cand : TILE_HEIGHTS) {
    long long tallest = 0;
    for (int y0 = 0; y0 < h; y0 += cand) {
      const int yl = std::min(y0 + cand, h) - 1;
      tallest = std::max(tallest, (long long)yb[2 * yl] + yb[2 * yl + 1] - yb[2 * y0]);
    }
    if (tallest * pitch <= LDS_BYTES) { th = cand; break; }
  }
  if (!th) {
    wct_set_error("resize: %d rows to %d at %d columns a tile: one output row taps more input rows than the %d bytes of LDS hold "
                  "(at most %d)", H, h, std::min(TILE_W, w), LDS_BYTES, LDS_BYTES / pitch);
    return WCT_ERR_ARG;
  }
  *g = ResizeGeom{H, W, h, w, ksx, ksy, th};
  return WCT_OK;
}

int launch_resize(const uint8_t* in, uint8_t* out, int B, const ResizeGeom& g, const int* tabs_dev, hipStream_t s) {
  ARG_CHECK(in && out && tabs_dev && g.th >= 1);
  const int rc = resize_check_bytes(B, g.H, g.W, g.h, g.w);
  if (rc) return rc;
  const int tiles_x = cdiv(g.w, TILE_W);
  const unsigned long long tiles = (unsigned long long)tiles_x * (unsigned long long)cdiv(g.h, g.th);
  ARG_CHECK(tiles < (1ull << 31));
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(THREADS), 0, s, in, out, g.H, g.W, g.h, g.w, tabs_dev,
                     g.ksx, g.ksy, g.th, tiles_x);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
