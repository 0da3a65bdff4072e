// Host check of wct_tf_amd/csrc/guided_color_rule.h (the rule the kernels of guided_color.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_color_cpu.py and run as a program of its own: the signed-overflow check is
// the proof of the bounds the header states.  The window sums are formed naively here (a loop over every pixel of every window).
// usage: guided_color_rule_check FILE.  FILE: int32 N, then N cases: int32 H, W, Hc, Wc, r, eps_q; H*W*3 stylized bytes, Hc*Wc*3
// content bytes, H*W*3 expected bytes.  Prints the largest |a_q|, |b_q| and bit length of det met.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_color_rule.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, f) != 1 || ncases < 0) return 2;
  int bad = 0, max_bits = 0;
  long long pixels = 0, max_a = 0, max_b = 0;
  const int KS = WCT_GUIDED_COLOR_SUMS, KC = WCT_GUIDED_COLOR_COEFFS;
  for (int k = 0; k < ncases; ++k) {
    int hd[6];
    if (fread(hd, 4, 6, f) != 6) return 2;
    const int H = hd[0], W = hd[1], Hc = hd[2], Wc = hd[3], r = hd[4], eps_q = hd[5];
    if (H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > H || Wc > W || !wct_guided_params_ok(r, eps_q)) return 2;
    std::vector<uint8_t> s((size_t)H * W * 3), c((size_t)Hc * Wc * 3), want(s.size());
    if (fread(s.data(), 1, s.size(), f) != s.size() || fread(c.data(), 1, c.size(), f) != c.size() ||
        fread(want.data(), 1, want.size(), f) != want.size())
      return 2;
    std::vector<int> I((size_t)H * W * 3);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const uint8_t* p = &c[((size_t)(y < Hc ? y : Hc - 1) * Wc + (x < Wc ? x : Wc - 1)) * 3];
        for (int i = 0; i < 3; ++i) I[((size_t)y * W + x) * 3 + i] = p[i];
      }
    // the 21 terms of every pixel once (wct_guided_color_terms, what a kernel thread adds per row), then summed window by window
    std::vector<int32_t> T((size_t)H * W * KS);
    for (size_t q = 0; q < (size_t)H * W; ++q) {
      const int px[3] = {s[q * 3], s[q * 3 + 1], s[q * 3 + 2]};
      unsigned d[KS];
      wct_guided_color_terms(&I[q * 3], px, d);
      for (int j = 0; j < KS; ++j) T[q * KS + j] = (int32_t)d[j];
    }
    std::vector<int32_t> ab((size_t)H * W * KC);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
        const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > W - 1 ? W - 1 : x + r;
        int32_t S32[KS] = {};                                            // int32 on purpose: the header says each stays below 2^31
        for (int yy = y0; yy <= y1; ++yy)
          for (int xx = x0; xx <= x1; ++xx) {
            const int32_t* d = &T[((size_t)yy * W + xx) * KS];
            for (int j = 0; j < KS; ++j) S32[j] += d[j];
          }
        const int64_t n = (int64_t)wct_guided_extent(y, H, r) * wct_guided_extent(x, W, r);
        if (n != (int64_t)(y1 - y0 + 1) * (x1 - x0 + 1)) { printf("FAIL case %d: extent at (%d, %d)\n", k, y, x); return 1; }
        int64_t S[KS];
        for (int j = 0; j < KS; ++j) S[j] = S32[j];
        int32_t* o = &ab[((size_t)y * W + x) * KC];
        int bits = 0;
        wct_guided_color_ab(n, S, eps_q, o, &bits);
        if (bits > max_bits) max_bits = bits;
        for (int j = 0; j < KC; ++j) {
          const long long v = o[j] < 0 ? -(long long)o[j] : o[j];
          if (j < 9 && v > max_a) max_a = v;
          if (j >= 9 && v > max_b) max_b = v;
        }
      }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
        const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > W - 1 ? W - 1 : x + r;
        int64_t Q[KC] = {};
        for (int yy = y0; yy <= y1; ++yy)
          for (int xx = x0; xx <= x1; ++xx) {
            const int32_t* p = &ab[((size_t)yy * W + xx) * KC];
            for (int j = 0; j < KC; ++j) Q[j] += p[j];
          }
        const int64_t n = (int64_t)(y1 - y0 + 1) * (x1 - x0 + 1);
        for (int ch = 0; ch < 3; ++ch) {
          const int64_t SA[3] = {Q[ch], Q[3 + ch], Q[6 + ch]};
          const uint8_t got = wct_guided_color_out(n, SA, Q[9 + ch], &I[((size_t)y * W + x) * 3]);
          const uint8_t w = want[((size_t)y * W + x) * 3 + ch];
          if (got != w && bad++ < 10) printf("FAIL case %d (%dx%d r %d eps_q %d) pixel (%d, %d, %d): %d, expected %d\n", k, H, W, r, eps_q, y, x, ch, got, w);
        }
      }
    pixels += (long long)H * W;
  }
  fclose(f);
  if (max_a >= WCT_GUIDED_COLOR_MAX_A || max_b >= WCT_GUIDED_COLOR_MAX_B || max_bits > 61) {
    printf("FAIL bounds: max |a_q| %lld, max |b_q| %lld, det bits %d\n", max_a, max_b, max_bits);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld pixels, max |a_q| %lld, max |b_q| %lld, det bits %d\n", ncases, pixels, max_a, max_b, max_bits);
  return 0;
}
