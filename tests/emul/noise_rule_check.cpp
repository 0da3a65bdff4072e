// Host check of wct_tf_amd/csrc/noise_rule.h (the byte rule the kernel of noise.hip calls), built with
// -fsanitize=address,undefined by tests/test_texture_cpu.py and run as a program of its own.
// usage: noise_rule_check FILE.  FILE: int32 N cases, each int32 H, int32 W, uint32 seed, uint32 sample, int32 smooth and the
// H * W * 3 expected bytes of that image (tests/texture_oracle.py).
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/noise_rule.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int cases = 0;
  if (fread(&cases, 4, 1, f) != 1 || cases < 0) return 2;
  long long bytes = 0;
  int bad = 0;
  for (int i = 0; i < cases; ++i) {
    int hdr[5];
    if (fread(hdr, 4, 5, f) != 5) return 2;
    const int H = hdr[0], W = hdr[1], smooth = hdr[4];
    const uint32_t seed = (uint32_t)hdr[2], sample = (uint32_t)hdr[3];
    if (H < 1 || W < 1 || (long long)H * W * 3 > (1 << 24)) return 2;
    std::vector<uint8_t> want((size_t)H * W * 3);
    if (fread(want.data(), 1, want.size(), f) != want.size()) return 2;
    const uint32_t key = wct_noise_key(seed, sample);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        for (int ch = 0; ch < 3; ++ch) {
          const uint8_t got = wct_noise_byte(key, H, W, y, x, ch, smooth);
          const uint8_t exp = want[((size_t)y * W + x) * 3 + ch];
          if (got != exp && bad++ < 10)
            printf("FAIL case %d (%dx%d seed %u sample %u smooth %d) byte (%d, %d, %d): %d, expected %d\n", i, H, W, seed, sample,
                   smooth, y, x, ch, got, exp);
        }
    bytes += (long long)H * W * 3;
  }
  fclose(f);
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld bytes\n", cases, bytes);
  return 0;
}
