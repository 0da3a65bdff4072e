// Host check of wct_tf_amd/csrc/guided_up_color_rule.h (the rule the kernels of guided_up_color.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_up_color_cpu.py and run as a program of its own: the signed-overflow check is
// the proof of the bounds the header states.  The window sums come from int64 summed-area tables here (the kernels use running
// column sums and row prefixes).  The 32-bit axis taps are compared with the 64-bit ones on every axis met.
// usage: guided_up_color_rule_check FILE.  FILE: int32 N, then N cases: int32 h, w, hc, wc, H, W, r, eps_q; h*w*3 stylized bytes,
// hc*wc*3 small content bytes, H*W*3 full content bytes, H*W*3 expected bytes.  Prints the largest |a_q|, |b_q|, |am|, |bm|, |v| met.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_up_color_rule.h"

static const int KS = WCT_GUIDED_COLOR_SUMS, KC = WCT_GUIDED_COLOR_COEFFS;

static long long absll(long long v) { return v < 0 ? -v : v; }

// the summed-area table of a [h][w] plane, (h + 1) x (w + 1), and a window sum from it
static std::vector<int64_t> sat(const std::vector<int64_t>& a, int h, int w) {
  std::vector<int64_t> t((size_t)(h + 1) * (w + 1), 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      t[(size_t)(y + 1) * (w + 1) + x + 1] = a[(size_t)y * w + x] + t[(size_t)y * (w + 1) + x + 1] + t[(size_t)(y + 1) * (w + 1) + x] -
                                             t[(size_t)y * (w + 1) + x];
  return t;
}
static int64_t win(const std::vector<int64_t>& t, int w, int y0, int y1, int x0, int x1) {
  return t[(size_t)(y1 + 1) * (w + 1) + x1 + 1] - t[(size_t)y0 * (w + 1) + x1 + 1] - t[(size_t)(y1 + 1) * (w + 1) + x0] +
         t[(size_t)y0 * (w + 1) + x0];
}

static int check_axis(int N, int m) {
  if (!wct_guided_up_axis32_ok(N, m)) return 0;
  for (int P = 0; P < N; ++P) {
    int a[3], b[3];
    wct_guided_up_axis(P, N, m, &a[0], &a[1], &a[2]);
    wct_guided_up_axis32(P, N, m, &b[0], &b[1], &b[2]);
    if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2]) { printf("FAIL axis32 N %d m %d P %d\n", N, m, P); return 1; }
    if (a[0] < 0 || a[1] >= m || a[0] > a[1] || a[2] < 0 || a[2] > WCT_GUIDED_UP_ONE) { printf("FAIL axis N %d m %d P %d\n", N, m, P); return 1; }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, f) != 1 || ncases < 0) return 2;
  int bad = 0;
  long long pixels = 0, max_a = 0, max_b = 0, max_am = 0, max_bm = 0, max_v = 0;
  for (int k = 0; k < ncases; ++k) {
    int hd[8];
    if (fread(hd, 4, 8, f) != 8) return 2;
    const int h = hd[0], w = hd[1], hc = hd[2], wc = hd[3], H = hd[4], W = hd[5], r = hd[6], eps_q = hd[7];
    if (hc < 1 || wc < 1 || h < hc || w < wc || H < hc || W < wc || !wct_guided_params_ok(r, eps_q)) return 2;
    std::vector<uint8_t> s((size_t)h * w * 3), c((size_t)hc * wc * 3), C((size_t)H * W * 3), want(C.size());
    if (fread(s.data(), 1, s.size(), f) != s.size() || fread(c.data(), 1, c.size(), f) != c.size() ||
        fread(C.data(), 1, C.size(), f) != C.size() || fread(want.data(), 1, want.size(), f) != want.size())
      return 2;
    // step 1: the 21 planes of wct_guided_color_terms and their tables
    const size_t np = (size_t)h * w;
    std::vector<std::vector<int64_t>> T(KS);
    {
      std::vector<std::vector<int64_t>> pl(KS, std::vector<int64_t>(np));
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          const uint8_t* q = &c[((size_t)(y < hc ? y : hc - 1) * wc + (x < wc ? x : wc - 1)) * 3];
          const uint8_t* p = &s[((size_t)y * w + x) * 3];
          const int I[3] = {q[0], q[1], q[2]}, pp[3] = {p[0], p[1], p[2]};
          unsigned d[WCT_GUIDED_COLOR_SUMS];
          wct_guided_color_terms(I, pp, d);
          for (int j = 0; j < KS; ++j) pl[j][(size_t)y * w + x] = d[j];
        }
      for (int j = 0; j < KS; ++j) T[j] = sat(pl[j], h, w);
    }
    std::vector<std::vector<int64_t>> ab(KC, std::vector<int64_t>(np));
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > h - 1 ? h - 1 : y + r;
        const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > w - 1 ? w - 1 : x + r;
        const int64_t n = (int64_t)wct_guided_extent(y, h, r) * wct_guided_extent(x, w, r);
        int64_t S[WCT_GUIDED_COLOR_SUMS];
        for (int j = 0; j < KS; ++j) S[j] = win(T[j], w, y0, y1, x0, x1);
        int32_t o[WCT_GUIDED_COLOR_COEFFS];
        wct_guided_color_ab(n, S, eps_q, o, nullptr);
        for (int j = 0; j < KC; ++j) {
          ab[j][(size_t)y * w + x] = o[j];
          long long& m = j < 9 ? max_a : max_b;
          if (absll(o[j]) > m) m = absll(o[j]);
        }
      }
    // step 2
    std::vector<int32_t> mean(np * KC);
    {
      std::vector<std::vector<int64_t>> TA(KC);
      for (int j = 0; j < KC; ++j) TA[j] = sat(ab[j], h, w);
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > h - 1 ? h - 1 : y + r;
          const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > w - 1 ? w - 1 : x + r;
          const int64_t n = (int64_t)(y1 - y0 + 1) * (x1 - x0 + 1);
          int64_t S[WCT_GUIDED_COLOR_COEFFS];
          for (int j = 0; j < KC; ++j) S[j] = win(TA[j], w, y0, y1, x0, x1);
          int32_t* m = &mean[((size_t)y * w + x) * KC];
          wct_guided_up_color_mean(n, S, m);
          for (int j = 0; j < KC; ++j) {
            long long& mx = j < 9 ? max_am : max_bm;
            if (absll(m[j]) > mx) mx = absll(m[j]);
          }
        }
    }
    // step 3
    if (check_axis(H, hc) || check_axis(W, wc)) return 1;
    for (int Y = 0; Y < H; ++Y) {
      int y0, y1, fy;
      wct_guided_up_axis(Y, H, hc, &y0, &y1, &fy);
      for (int X = 0; X < W; ++X) {
        int x0, x1, fx;
        wct_guided_up_axis(X, W, wc, &x0, &x1, &fx);
        const uint8_t* q = &C[((size_t)Y * W + X) * 3];
        const int I[3] = {q[0], q[1], q[2]};
        const int32_t* const m4[4] = {&mean[((size_t)y0 * w + x0) * KC], &mean[((size_t)y0 * w + x1) * KC], &mean[((size_t)y1 * w + x0) * KC],
                                      &mean[((size_t)y1 * w + x1) * KC]};
        for (int p = 0; p < 3; ++p) {
          const int64_t v = wct_guided_up_color_sum(m4, p, fy, fx, I);
          if (absll(v) > max_v) max_v = absll(v);
          const uint8_t got = wct_guided_up_out(v), wv = want[((size_t)Y * W + X) * 3 + p];
          if (got != wv && bad++ < 10)
            printf("FAIL case %d (%dx%d -> %dx%d r %d eps_q %d) pixel (%d, %d, %d): %d, expected %d\n", k, hc, wc, H, W, r, eps_q, Y, X, p,
                   got, wv);
        }
      }
    }
    pixels += (long long)H * W;
  }
  fclose(f);
  // the header's bounds: |am| <= WCT_GUIDED_COLOR_MAX_A, |bm| <= WCT_GUIDED_COLOR_MAX_B, |v| < WCT_GUIDED_UP_COLOR_MAX_V
  if (max_a > WCT_GUIDED_COLOR_MAX_A || max_b > WCT_GUIDED_COLOR_MAX_B || max_am > WCT_GUIDED_COLOR_MAX_A ||
      max_bm > WCT_GUIDED_COLOR_MAX_B || max_v >= WCT_GUIDED_UP_COLOR_MAX_V) {
    printf("FAIL bounds: max |a_q| %lld, max |b_q| %lld, max |am| %lld, max |bm| %lld, max |v| %lld\n", max_a, max_b, max_am, max_bm, max_v);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld pixels, max |a_q| %lld, max |b_q| %lld, max |am| %lld, max |bm| %lld, max |v| %lld\n", ncases,
         pixels, max_a, max_b, max_am, max_bm, max_v);
  return 0;
}
