// Seeded noise images for texture synthesis (noise_rule.h): B images [B][H][W][3] uint8 in ONE launch, image b the sample
// first_sample + b of `seed`.  The output is one flat stream of B * H * W * 3 bytes cut at the 16-byte boundaries of its
// ADDRESSES: lane i owns the 16 bytes at (out rounded down to 16) + 16 i.  A lane whose 16 bytes all lie inside the stream
// computes them and stores them with one 16-byte vector store (its address is aligned by construction, whatever the base); the
// lane that holds the stream's first bytes when the base is not 16-byte aligned (the head) and the one that holds its last
// bytes (the tail) store byte by byte, and only the bytes that are theirs.  A lane walks (image, y, x, channel) forwards from its
// first byte, so a group may run across the end of a row or of an image.  Microseconds next to the chain that consumes the
// images: the point is every byte right at every size, not a rate.
#include "common.h"
#include "noise_rule.h"

namespace {
constexpr unsigned LANE_BYTES = 16;
constexpr unsigned MAX_BLOCKS = 1024;      // grid cap (4 blocks of 256 per CU); the rest is grid-strided
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the position of a byte of the stream, and the step to the next one
struct Cursor {
  int H, W, y, x, ch;
  unsigned seed, sample, key;
  __device__ __forceinline__ void next() {
    if (++ch < 3) return;
    ch = 0;
    if (++x < W) return;
    x = 0;
    if (++y < H) return;
    y = 0;
    key = wct_noise_key(seed, ++sample);
  }
};

// out: `total` bytes = B images of H * W * 3; lead = out & 15, lanes = ceil((total + lead) / 16); total + lead + 15 < 2^32
__global__ __launch_bounds__(256) void texture_noise_kernel(uint8_t* out, int H, int W, unsigned total, unsigned lead, unsigned lanes,
                                                            unsigned seed, unsigned first_sample, int smooth) {
  const unsigned per = (unsigned)H * (unsigned)W * 3u;
  for (unsigned it = blockIdx.x * blockDim.x + threadIdx.x; it < lanes; it += gridDim.x * blockDim.x) {
    // the lane's bytes lo .. hi - 1 of the stream: 16 it - lead .. + 15, cut to 0 .. total - 1
    const unsigned first = it * LANE_BYTES;
    const unsigned lo = first < lead ? 0u : first - lead;
    const unsigned hi = first + LANE_BYTES - lead < total ? first + LANE_BYTES - lead : total;
    const unsigned b = lo / per, n = lo - b * per, pix = n / 3u;
    Cursor cur;
    cur.H = H; cur.W = W;
    cur.ch = (int)(n - pix * 3u); cur.y = (int)(pix / (unsigned)W); cur.x = (int)(pix - (unsigned)cur.y * (unsigned)W);
    cur.seed = seed; cur.sample = first_sample + b; cur.key = wct_noise_key(seed, cur.sample);
    if (hi - lo == LANE_BYTES) {                           // a whole group: out + lo is 16-byte aligned
      unsigned word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (unsigned k = 0; k < LANE_BYTES; ++k) {
        word[k >> 2] |= (unsigned)wct_noise_byte(cur.key, H, W, cur.y, cur.x, cur.ch, smooth) << (8 * (k & 3));
        cur.next();
      }
      const u32x4 v = {word[0], word[1], word[2], word[3]};
      *(u32x4*)(out + lo) = v;
    } else {                                               // the head or the tail: its own bytes, one by one
      for (unsigned j = lo; j < hi; ++j) {
        out[j] = wct_noise_byte(cur.key, H, W, cur.y, cur.x, cur.ch, smooth);
        cur.next();
      }
    }
  }
}
}  // namespace

int launch_texture_noise(uint8_t* out, int B, int H, int W, unsigned seed, unsigned first_sample, int smooth, hipStream_t s) {
  ARG_CHECK(out && B >= 1 && H >= 1 && W >= 1);
  // every index of the kernel is a 32-bit one: a call whose bytes pass 2^31 is refused, not wrapped
  const unsigned long long limit = 1ull << 31;
  const unsigned long long total = (unsigned long long)H * (unsigned long long)W >= limit
                                       ? limit : (unsigned long long)H * W * 3ull * (unsigned long long)B;
  if (total >= limit) {
    wct_set_error("texture noise: %d images of %dx%dx3 pass 2^31 bytes in one call", B, H, W);
    return WCT_ERR_ARG;
  }
  const unsigned lead = (unsigned)((uintptr_t)out & (LANE_BYTES - 1));
  const unsigned lanes = ((unsigned)total + lead + LANE_BYTES - 1) / LANE_BYTES;
  unsigned blocks = (lanes + 255) / 256;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  hipLaunchKernelGGL(texture_noise_kernel, dim3(blocks), dim3(256), 0, s, out, H, W, (unsigned)total, lead, lanes, seed, first_sample,
                     smooth ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return WCT_OK;
}
