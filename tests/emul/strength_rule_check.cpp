// Host check of wct_tf_amd/csrc/strength_rule.h (the blend rule the apply kernels of wct.hip share), built with
// -fsanitize=address,undefined by tests/test_strength_cpu.py and run as a program of its own.
// usage: strength_rule_check FILE.  FILE: int32 N, then N records of 24 bytes -- float alpha, uint32 v (0 .. 255), float y,
// float x, float a expected, float out expected -- compared bit for bit (a NaN matches any NaN); then int32 M and M records of
// 7 int32 -- i, j, stride, Hm, Wm, expected row, expected column -- of the map addressing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../wct_tf_amd/csrc/strength_rule.h"

static bool same_bits(float got, float want) {
  if (got != got && want != want) return true;
  return memcmp(&got, &want, 4) == 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int n = 0, m = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<float> rec((size_t)n * 6);
  if (n && fread(rec.data(), 24, n, f) != (size_t)n) return 2;
  if (fread(&m, 4, 1, f) != 1 || m < 0) return 2;
  std::vector<int> idx((size_t)m * 7);
  if (m && fread(idx.data(), 28, m, f) != (size_t)m) return 2;
  fclose(f);
  int bad = 0;
  for (int i = 0; i < n; ++i) {
    const float* r = &rec[(size_t)i * 6];
    unsigned v;
    memcpy(&v, &r[1], 4);
    if (v > 255) return 2;
    const float a = wct_strength_a(r[0], (uint8_t)v);
    const float o = wct_strength_blend(a, r[2], r[3]);
    if (!same_bits(a, r[4]) || !same_bits(o, r[5])) {
      if (bad++ < 10)
        printf("FAIL record %d: alpha %.9g v %u y %.9g x %.9g -> a %.9g out %.9g, expected a %.9g out %.9g\n", i, (double)r[0], v,
               (double)r[2], (double)r[3], (double)a, (double)o, (double)r[4], (double)r[5]);
    }
  }
  for (int i = 0; i < m; ++i) {
    const int* q = &idx[(size_t)i * 7];
    const size_t at = wct_strength_index(q[0], q[1], q[2], q[3], q[4]);
    if (at != (size_t)q[5] * q[4] + q[6]) {
      if (bad++ < 10) printf("FAIL index %d: pixel (%d, %d) stride %d of a %dx%d map -> %zu, expected (%d, %d)\n", i, q[0], q[1], q[2], q[3], q[4], at, q[5], q[6]);
    }
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d blends, %d indices\n", n, m);
  return 0;
}
