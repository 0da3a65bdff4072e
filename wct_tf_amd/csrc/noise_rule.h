// Seeded noise images for texture synthesis (Li et al. 2017, sec. 4.3: a noise image through the multi-level pipeline; the
// reference's webcam.py:191-192 `np.random.randint(0, 256, shape, np.uint8)` and the recipe of stylize.py:95-97, the same noise
// under gaussian_filter(sigma=0.5)): the rule of one byte, integers only, shared by the kernel of noise.hip and by any host
// program (plain C++: nothing of HIP is needed to include this file).  All arithmetic is mod 2^32.
//   fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (murmur3's finaliser)
//   key = fmix(seed ^ (sample * 0x9E3779B9))               one key per image: sample is the image's index
//   n   = (y * W + x) * 3 + ch                             the byte's index in its [H][W][3] image
//   raw = fmix(fmix(n ^ key) + key) >> 24                  one uniform byte
// smooth: the 3-tap filter 27 202 27 (sigma = 0.5 to 8 bits; the taps at +-2 round to 0) along y and along x, not across R, G, B:
//   out = (sum_dy sum_dx w[dy] w[dx] raw(sym(y + dy, H), sym(x + dx, W), ch) + 32768) >> 16,   sym(-1, n) = 0, sym(n, n) = n - 1
// (scipy's mode='reflect', NumPy's 'symmetric' -- not the tf.pad REFLECT of the convolutions).  A byte's nine raw neighbours come
// from their indices: no halo, no intermediate image.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WCT_NOISE_HD __host__ __device__
#else
#define WCT_NOISE_HD
#endif

WCT_NOISE_HD inline uint32_t wct_noise_fmix(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

WCT_NOISE_HD inline uint32_t wct_noise_key(uint32_t seed, uint32_t sample) { return wct_noise_fmix(seed ^ (sample * 0x9E3779B9u)); }

// the raw byte n of the image of `key`
WCT_NOISE_HD inline uint32_t wct_noise_raw(uint32_t key, uint32_t n) { return wct_noise_fmix(wct_noise_fmix(n ^ key) + key) >> 24; }

WCT_NOISE_HD inline int wct_noise_sym(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// byte (y, x, ch) of the H x W image of `key`; H * W * 3 < 2^31
WCT_NOISE_HD inline uint8_t wct_noise_byte(uint32_t key, int H, int W, int y, int x, int ch, int smooth) {
  if (!smooth) return (uint8_t)wct_noise_raw(key, ((uint32_t)y * (uint32_t)W + (uint32_t)x) * 3u + (uint32_t)ch);
  const uint32_t w[3] = {27u, 202u, 27u};
  uint32_t acc = 32768u;                            // <= 256 * 256 * 255 + 32768: no overflow
  for (int dy = -1; dy <= 1; ++dy) {
    const uint32_t row = (uint32_t)wct_noise_sym(y + dy, H) * (uint32_t)W;
    for (int dx = -1; dx <= 1; ++dx)
      acc += w[dy + 1] * w[dx + 1] * wct_noise_raw(key, (row + (uint32_t)wct_noise_sym(x + dx, W)) * 3u + (uint32_t)ch);
  }
  return (uint8_t)(acc >> 16);
}
