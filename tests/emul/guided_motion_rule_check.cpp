// Host check of wct_tf_amd/csrc/guided_motion_rule.h (the rule the kernels of guided_motion.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_motion_cpu.py and run as a program of its own: the signed-overflow check is
// the proof of the bounds the header states.  A frame's shifted box sum comes from 64-bit prefix sums and is at most
// (2r + 1)^2 * 65025 < 2^31; the sum of those over the frames of the window is formed in int32 on purpose: its terms are
// non-negative, so it overflows exactly when a window sum of pass 1 passes 2^31 - 1.
// usage: guided_motion_rule_check FILE.  FILE: int32 N, then N filter cases: int32 F, H, W, Hc, Wc, r, eps_q, T; F*2 int32
// positions; F*H*W*3 stylized bytes, F*Hc*Wc*3 content bytes, F*H*W*3 expected bytes.  Then int32 M and M estimator cases: int32
// F, Hc, Wc, R; F*Hc*Wc*3 content bytes; F*2 int32 expected positions.  Prints the largest n, pass-1 sum, |a_q| and |b_q| met.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_motion_rule.h"

// sums of a [H][W] over the (2r + 1)^2 box centred at (y + dy, x + dx), cut at the borders: 0 where it lies outside
static std::vector<int64_t> box_shift(const int64_t* a, int H, int W, int r, int dy, int dx) {
  std::vector<int64_t> p((size_t)(H + 1) * (W + 1), 0), o((size_t)H * W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      p[(size_t)(y + 1) * (W + 1) + x + 1] = a[(size_t)y * W + x] + p[(size_t)y * (W + 1) + x + 1] + p[(size_t)(y + 1) * (W + 1) + x] -
                                              p[(size_t)y * (W + 1) + x];
  auto clip = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int y0 = clip(y + dy - r, H), x0 = clip(x + dx - r, W);
      int y1 = clip(y + dy + r + 1, H), x1 = clip(x + dx + r + 1, W);
      if (y1 < y0) y1 = y0;
      if (x1 < x0) x1 = x0;
      o[(size_t)y * W + x] = p[(size_t)y1 * (W + 1) + x1] - p[(size_t)y0 * (W + 1) + x1] - p[(size_t)y1 * (W + 1) + x0] +
                             p[(size_t)y0 * (W + 1) + x0];
    }
  return o;
}

// window sums of a [F][H][W] under the positions: per frame of the window a shifted box, accumulated in V
template <typename V>
static std::vector<V> box3(const std::vector<int64_t>& a, int F, int H, int W, int r, int T, const int32_t* pos) {
  std::vector<V> o(a.size(), 0);
  for (int f = 0; f < F; ++f)
    for (int g = f - T < 0 ? 0 : f - T; g <= (f + T > F - 1 ? F - 1 : f + T); ++g) {
      const std::vector<int64_t> b = box_shift(&a[(size_t)g * H * W], H, W, r, pos[2 * g] - pos[2 * f], pos[2 * g + 1] - pos[2 * f + 1]);
      for (size_t i = 0; i < (size_t)H * W; ++i) o[(size_t)f * H * W + i] += (V)b[i];
    }
  return o;
}

// the comparisons of the estimator at its extreme: a 0 / 255 pair of Hc x Wc (SAD = 255 cnt for every candidate), all candidates
// of the largest range against each other.  Every mean is equal, so (0, 0) must win over all; UBSan watches the products.
static int extreme_pair(int Hc, int Wc, long long* max_product) {
  const int R = WCT_MOTION_MAX_RANGE;
  if (!wct_motion_search_ok(R, Hc, Wc)) return 1;
  for (int dy = -R; dy <= R; ++dy)
    for (int dx = -R; dx <= R; ++dx) {
      const int64_t n = wct_motion_count(dy, dx, Hc, Wc), s = 255 * n;
      if (n < 1) return 1;
      for (int ey = -R; ey <= R; ++ey)
        for (int ex = -R; ex <= R; ++ex) {
          const int64_t m = wct_motion_count(ey, ex, Hc, Wc), u = 255 * m;
          if (s * m > *max_product) *max_product = s * m;
          const bool want = dy * dy + dx * dx != ey * ey + ex * ex ? dy * dy + dx * dx < ey * ey + ex * ex : (dy != ey ? dy < ey : dx < ex);
          if (wct_motion_better(s, n, dy, dx, u, m, ey, ex) != want) return 1;
        }
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, fp) != 1 || ncases < 0) return 2;
  int bad = 0;
  long long pixels = 0, max_a = 0, max_b = 0, max_n = 0, max_s = 0, min_n = 1 << 30;
  for (int k = 0; k < ncases; ++k) {
    int hd[8];
    if (fread(hd, 4, 8, fp) != 8) return 2;
    const int F = hd[0], H = hd[1], W = hd[2], Hc = hd[3], Wc = hd[4], r = hd[5], eps_q = hd[6], T = hd[7];
    if (F < 1 || F > 32 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > H || Wc > W || !wct_guided_time_params_ok(r, eps_q, T)) return 2;
    std::vector<int32_t> pos((size_t)F * 2);
    if (fread(pos.data(), 4, pos.size(), fp) != pos.size() || wct_motion_bad_step(pos.data(), F) >= 0) return 2;
    const size_t px = (size_t)F * H * W;
    std::vector<uint8_t> s(px * 3), c((size_t)F * Hc * Wc * 3), want(s.size());
    if (fread(s.data(), 1, s.size(), fp) != s.size() || fread(c.data(), 1, c.size(), fp) != c.size() ||
        fread(want.data(), 1, want.size(), fp) != want.size())
      return 2;
    std::vector<int64_t> q[8];                                  // I, I^2, p[3], I p[3]
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
    for (int j = 0; j < 8; ++j) S[j] = box3<int32_t>(q[j], F, H, W, r, T, pos.data());    // the header says each stays below 2^31
    std::vector<int64_t> ab[6];
    for (auto& v : ab) v.resize(px);
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = ((size_t)f * H + y) * W + x;
          const int64_t n = wct_guided_motion_n(pos.data(), f, F, T, y, H, x, W, r);
          if (n > max_n) max_n = n;
          if (n < min_n) min_n = n;
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
    for (int j = 0; j < 6; ++j) SAB[j] = box3<int64_t>(ab[j], F, H, W, r, T, pos.data());
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const size_t i = ((size_t)f * H + y) * W + x;
          const int64_t n = wct_guided_motion_n(pos.data(), f, F, T, y, H, x, W, r);
          for (int ch = 0; ch < 3; ++ch) {
            const uint8_t got = wct_guided_out(n, SAB[2 * ch][i], SAB[2 * ch + 1][i], (int)q[0][i]);
            const uint8_t w = want[i * 3 + ch];
            if (got != w && bad++ < 10)
              printf("FAIL case %d (%dx%dx%d r %d eps_q %d T %d) pixel (%d, %d, %d, %d): %d, expected %d\n", k, F, H, W, r, eps_q, T, f, y,
                     x, ch, got, w);
          }
        }
    pixels += (long long)px;
  }
  int nest = 0;
  if (fread(&nest, 4, 1, fp) != 1 || nest < 0) return 2;
  for (int k = 0; k < nest; ++k) {
    int hd[4];
    if (fread(hd, 4, 4, fp) != 4) return 2;
    const int F = hd[0], Hc = hd[1], Wc = hd[2], R = hd[3];
    if (F < 1 || !wct_motion_search_ok(R, Hc, Wc)) return 2;
    const size_t plane = (size_t)Hc * Wc;
    std::vector<uint8_t> c((size_t)F * plane * 3), I((size_t)F * plane);
    std::vector<int32_t> want((size_t)F * 2), pos((size_t)F * 2, 0);
    if (fread(c.data(), 1, c.size(), fp) != c.size() || fread(want.data(), 4, want.size(), fp) != want.size()) return 2;
    for (size_t i = 0; i < I.size(); ++i) I[i] = (uint8_t)wct_guided_guide(c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    for (int f = 0; f + 1 < F; ++f) {
      int32_t d[2];
      wct_motion_pair(&I[f * plane], &I[(f + 1) * plane], Hc, Wc, R, d);
      pos[2 * f + 2] = pos[2 * f] + d[0];
      pos[2 * f + 3] = pos[2 * f + 1] + d[1];
    }
    for (int f = 0; f < F; ++f)
      if ((pos[2 * f] != want[2 * f] || pos[2 * f + 1] != want[2 * f + 1]) && bad++ < 10)
        printf("FAIL estimator case %d (%d frames of %dx%d, R %d) frame %d: (%d, %d), expected (%d, %d)\n", k, F, Hc, Wc, R, f, pos[2 * f],
               pos[2 * f + 1], want[2 * f], want[2 * f + 1]);
  }
  fclose(fp);
  long long max_product = 0;
  // 2^28 pixels as a square, as the longest strip a range of 16 admits, and odd sides (ceil(Hc / 2) ceil(Wc / 2) just above 2^26)
  if (extreme_pair(16384, 16384, &max_product) || extreme_pair(64, 1 << 22, &max_product) || extreme_pair(16383, 16385, &max_product)) {
    printf("FAIL estimator comparisons at the extreme\n");
    return 1;
  }
  if (max_n > WCT_GUIDED_TIME_MAX_WINDOW || min_n < 1 || max_a >= (1 << 18) || max_b >= 68000000) {
    printf("FAIL bounds: n %lld .. %lld, max |a_q| %lld, max |b_q| %lld\n", min_n, max_n, max_a, max_b);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %d estimator cases, %lld pixels, min n %lld, max n %lld, max sum %lld, max |a_q| %lld, max |b_q| %lld, "
         "max product %lld\n", ncases, nest, pixels, min_n, max_n, max_s, max_a, max_b, max_product);
  return 0;
}
