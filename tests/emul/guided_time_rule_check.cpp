// Host check of wct_tf_amd/csrc/guided_time_rule.h (the rule the kernels of guided_time.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_time_cpu.py and run as a program of its own: the signed-overflow check is the
// proof of the bounds the header states.  The window sums are formed axis by axis (time, then x, then y): every partial sum of
// non-negative terms is at most the full window's, so pass 1's stay in int32 if the header's limit is right.
// usage: guided_time_rule_check FILE.  FILE: int32 N, then N cases: int32 F, H, W, Hc, Wc, r, eps_q, T; F*H*W*3 stylized bytes,
// F*Hc*Wc*3 content bytes, F*H*W*3 expected bytes.  Prints the largest n, pass-1 sum, |a_q| and |b_q| met.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_time_rule.h"

// window sums of a [F][H][W] over the box of (r, T) cut at the borders, one axis at a time, all in V
template <typename V>
static std::vector<V> box3(const std::vector<V>& a, int F, int H, int W, int r, int T) {
  std::vector<V> t(a.size()), u(a.size()), o(a.size());
  for (int f = 0; f < F; ++f)
    for (size_t i = 0; i < (size_t)H * W; ++i) {
      V acc = 0;
      for (int g = f - T < 0 ? 0 : f - T; g <= (f + T > F - 1 ? F - 1 : f + T); ++g) acc += a[(size_t)g * H * W + i];
      t[(size_t)f * H * W + i] = acc;
    }
  for (size_t row = 0; row < (size_t)F * H; ++row)
    for (int x = 0; x < W; ++x) {
      V acc = 0;
      for (int xx = x - r < 0 ? 0 : x - r; xx <= (x + r > W - 1 ? W - 1 : x + r); ++xx) acc += t[row * W + xx];
      u[row * W + x] = acc;
    }
  for (int f = 0; f < F; ++f)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        V acc = 0;
        for (int yy = y - r < 0 ? 0 : y - r; yy <= (y + r > H - 1 ? H - 1 : y + r); ++yy) acc += u[((size_t)f * H + yy) * W + x];
        o[((size_t)f * H + y) * W + x] = acc;
      }
  return o;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, fp) != 1 || ncases < 0) return 2;
  for (int T = -1; T <= 4; ++T) {                               // the limit table, and its agreement with params_ok
    const int want[4] = {64, 51, 40, 33}, got = wct_guided_time_radius_limit(T);
    if (got != (T >= 0 && T <= 3 ? want[T] : 0)) { printf("FAIL radius limit at T = %d: %d\n", T, got); return 1; }
    for (int r = 0; r <= 66; ++r)
      if (wct_guided_time_params_ok(r, 650, T) != (r >= 1 && r <= got)) { printf("FAIL params_ok(%d, 650, %d)\n", r, T); return 1; }
  }
  int bad = 0;
  long long pixels = 0, max_a = 0, max_b = 0, max_n = 0, max_s = 0;
  for (int k = 0; k < ncases; ++k) {
    int hd[8];
    if (fread(hd, 4, 8, fp) != 8) return 2;
    const int F = hd[0], H = hd[1], W = hd[2], Hc = hd[3], Wc = hd[4], r = hd[5], eps_q = hd[6], T = hd[7];
    if (F < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > H || Wc > W || !wct_guided_time_params_ok(r, eps_q, T)) return 2;
    const size_t px = (size_t)F * H * W;
    std::vector<uint8_t> s(px * 3), c((size_t)F * Hc * Wc * 3), want(s.size());
    if (fread(s.data(), 1, s.size(), fp) != s.size() || fread(c.data(), 1, c.size(), fp) != c.size() ||
        fread(want.data(), 1, want.size(), fp) != want.size())
      return 2;
    std::vector<int32_t> q[8];                                  // I, I^2, p[3], I p[3]: int32 on purpose, as their sums are below
    for (auto& v : q) v.resize(px);
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = ((size_t)f * H + y) * W + x;
          const uint8_t* p = &c[(((size_t)f * Hc + (y < Hc ? y : Hc - 1)) * Wc + (x < Wc ? x : Wc - 1)) * 3];
          const int g = wct_guided_guide(p[0], p[1], p[2]);
          q[0][i] = g; q[1][i] = g * g;
          for (int ch = 0; ch < 3; ++ch) { q[2 + ch][i] = s[i * 3 + ch]; q[5 + ch][i] = g * s[i * 3 + ch]; }
        }
    std::vector<int32_t> S[8];
    for (int j = 0; j < 8; ++j) S[j] = box3<int32_t>(q[j], F, H, W, r, T);     // the header says each stays below 2^31
    std::vector<int64_t> ab[6];
    for (auto& v : ab) v.resize(px);
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = ((size_t)f * H + y) * W + x;
          const int64_t n = wct_guided_time_n(f, F, T, y, H, x, W, r);
          if (n > max_n) max_n = n;
          for (int j = 0; j < 8; ++j) if (S[j][i] > max_s) max_s = S[j][i];
          for (int ch = 0; ch < 3; ++ch) {
            int32_t a, b;
            wct_guided_ab(n, S[0][i], S[1][i], S[2 + ch][i], S[5 + ch][i], eps_q, &a, &b);
            ab[2 * ch][i] = a; ab[2 * ch + 1][i] = b;
            const long long aa = a < 0 ? -(long long)a : a, bb = b < 0 ? -(long long)b : b;
            if (aa > max_a) max_a = aa;
            if (bb > max_b) max_b = bb;
          }
        }
    std::vector<int64_t> SAB[6];
    for (int j = 0; j < 6; ++j) SAB[j] = box3<int64_t>(ab[j], F, H, W, r, T);
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = ((size_t)f * H + y) * W + x;
          const int64_t n = wct_guided_time_n(f, F, T, y, H, x, W, r);
          for (int ch = 0; ch < 3; ++ch) {
            const uint8_t got = wct_guided_out(n, SAB[2 * ch][i], SAB[2 * ch + 1][i], q[0][i]);
            const uint8_t w = want[i * 3 + ch];
            if (got != w && bad++ < 10)
              printf("FAIL case %d (%dx%dx%d r %d eps_q %d T %d) pixel (%d, %d, %d, %d): %d, expected %d\n", k, F, H, W, r, eps_q, T, f, y,
                     x, ch, got, w);
          }
        }
    pixels += (long long)px;
  }
  fclose(fp);
  if (max_n > WCT_GUIDED_TIME_MAX_WINDOW || max_a >= (1 << 18) || max_b >= 68000000) {
    printf("FAIL bounds: max n %lld, max |a_q| %lld, max |b_q| %lld\n", max_n, max_a, max_b);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld pixels, max n %lld, max sum %lld, max |a_q| %lld, max |b_q| %lld\n", ncases, pixels, max_n,
         max_s, max_a, max_b);
  return 0;
}
