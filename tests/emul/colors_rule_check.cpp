// Host check of wct_tf_amd/csrc/colors_rule.h (the pixel rule the kernels of colors.hip share), built with
// -fsanitize=address,undefined by tests/test_colors_cpu.py and run as a program of its own.
// usage: colors_rule_check FILE.  FILE: int32 N, N x 9 bytes (stylized RGB, content RGB, expected RGB), int32 M, M floats,
// M expected bytes of the output rule uint8(clip(x, 0, 1) * 255.f).
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/colors_rule.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int n = 0, m = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<uint8_t> px((size_t)n * 9);
  if (n && fread(px.data(), 9, n, f) != (size_t)n) return 2;
  if (fread(&m, 4, 1, f) != 1 || m < 0) return 2;
  std::vector<float> x(m);
  std::vector<uint8_t> q(m);
  if (m && (fread(x.data(), 4, m, f) != (size_t)m || fread(q.data(), 1, m, f) != (size_t)m)) return 2;
  fclose(f);
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    const uint8_t* r = &px[(size_t)i * 9];
    uint8_t o[3];
    wct_content_colors_px(r[0], r[1], r[2], r[3], r[4], r[5], o);
    if (o[0] != r[6] || o[1] != r[7] || o[2] != r[8]) {
      if (bad++ < 10)
        printf("FAIL pixel %d: s (%d %d %d) p (%d %d %d) -> (%d %d %d), expected (%d %d %d)\n", i, r[0], r[1], r[2], r[3], r[4], r[5],
               o[0], o[1], o[2], r[6], r[7], r[8]);
    }
  }
  for (int i = 0; i < m; ++i)
    if (wct_quantise_u8(x[i]) != q[i]) {
      if (bad++ < 10) printf("FAIL sample %d: %.9g -> %d, expected %d\n", i, (double)x[i], wct_quantise_u8(x[i]), q[i]);
    }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d pixels, %d samples\n", n, m);
  return 0;
}
