// Host check of wct_tf_amd/csrc/resize_rule.h (the tap tables the launcher of resize.hip uploads and the byte rule its kernel
// calls), built with -fsanitize=address,undefined by tests/test_resize_cpu.py and run as a program of its own.
// usage: resize_rule_check FILE.  FILE: int32 N cases, each int32 H, W, h, w, then the expected tables as int32 -- bounds of x
// [w][2], taps of x [w][ksx], bounds of y [h][2], taps of y [h][ksy] -- the H * W * 3 input bytes and the h * w * 3 expected
// output bytes (tests/resize_oracle.py).
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/resize_rule.h"

static bool read_ints(FILE* f, std::vector<int>& v) { return fread(v.data(), 4, v.size(), f) == v.size(); }

static int compare(const char* what, int idx, const std::vector<int>& got, const std::vector<int>& want, int* bad) {
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i] != want[i] && (*bad)++ < 10) printf("FAIL case %d %s[%zu]: %d, expected %d\n", idx, what, i, got[i], want[i]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int cases = 0;
  if (fread(&cases, 4, 1, f) != 1 || cases < 0) return 2;
  long long bytes = 0, words = 0;
  int bad = 0;
  for (int i = 0; i < cases; ++i) {
    int hdr[4];
    if (fread(hdr, 4, 4, f) != 4) return 2;
    const int H = hdr[0], W = hdr[1], h = hdr[2], w = hdr[3];
    if (H < 1 || W < 1 || h < 1 || w < 1 || (long long)H * W * 3 > (1 << 24) || (long long)h * w * 3 > (1 << 24)) return 2;
    const int ksx = wct_resize_ksize(W, w), ksy = wct_resize_ksize(H, h);
    std::vector<int> xb_want((size_t)w * 2), kx_want((size_t)w * ksx), yb_want((size_t)h * 2), ky_want((size_t)h * ksy);
    if (!read_ints(f, xb_want) || !read_ints(f, kx_want) || !read_ints(f, yb_want) || !read_ints(f, ky_want)) return 2;
    std::vector<uint8_t> img((size_t)H * W * 3), want((size_t)h * w * 3);
    if (fread(img.data(), 1, img.size(), f) != img.size() || fread(want.data(), 1, want.size(), f) != want.size()) return 2;

    std::vector<int> xb(xb_want.size()), kx(kx_want.size()), yb(yb_want.size()), ky(ky_want.size());
    std::vector<double> scratch((size_t)(ksx > ksy ? ksx : ksy));
    wct_resize_taps(W, w, xb.data(), kx.data(), scratch.data());
    wct_resize_taps(H, h, yb.data(), ky.data(), scratch.data());
    compare("x bounds", i, xb, xb_want, &bad);
    compare("x taps", i, kx, kx_want, &bad);
    compare("y bounds", i, yb, yb_want, &bad);
    compare("y taps", i, ky, ky_want, &bad);
    words += (long long)(xb.size() + kx.size() + yb.size() + ky.size());

    // along x into the uint8 intermediate [H][w][3], then along y: the two passes of the kernel
    std::vector<uint8_t> mid((size_t)H * w * 3);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < w; ++x)
        for (int ch = 0; ch < 3; ++ch)
          mid[((size_t)y * w + x) * 3 + ch] =
              wct_resize_byte(kx.data() + (size_t)x * ksx, xb[2 * x + 1], img.data() + ((size_t)y * W + xb[2 * x]) * 3 + ch, 3);
    for (int y = 0; y < h; ++y)
      for (int j = 0; j < w * 3; ++j) {
        const uint8_t got = wct_resize_byte(ky.data() + (size_t)y * ksy, yb[2 * y + 1], mid.data() + (size_t)yb[2 * y] * w * 3 + j, w * 3);
        const uint8_t exp = want[(size_t)y * w * 3 + j];
        if (got != exp && bad++ < 10) printf("FAIL case %d (%dx%d to %dx%d) byte (%d, %d): %d, expected %d\n", i, H, W, h, w, y, j, got, exp);
      }
    bytes += (long long)h * w * 3;
  }
  fclose(f);
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld table words, %lld bytes\n", cases, words, bytes);
  return 0;
}
