// Host check of wct_tf_amd/csrc/guided_up_time_rule.h (the rule the kernels of guided_up_time.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_up_time_cpu.py and run as a program of its own: the signed-overflow check is
// the proof of the bounds the header states.  The window sums come from int64 summed-area tables per frame here (the kernels use
// running column sums and row prefixes); the window of a pixel is walked frame by frame with wct_guided_up_time_box.
// usage: guided_up_time_rule_check FILE.  FILE: int32 N, then N cases: int32 F, h, w, hc, wc, H, W, r, eps_q, T, has_pos; F*2 int32
// positions when has_pos; F*h*w*3 stylized bytes, F*hc*wc*3 small content bytes, F*H*W*3 full content bytes, F*H*W*3 expected
// bytes.  Prints the largest n, |a_q|, |SA|, |SB|, |am|, |bm|, |v| met.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_up_time_rule.h"

static long long absll(long long v) { return v < 0 ? -v : v; }

// the summed-area table of a [h][w] plane, (h + 1) x (w + 1), and a window sum from it
static std::vector<int64_t> sat(const int64_t* a, int h, int w) {
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

// the sums of K planes (tables T[frame * K + j]) over the window of (f, y, x), and its count
template <int K>
static int64_t window(const std::vector<std::vector<int64_t>>& T, const int32_t* pos, int f, int F, int t, int y, int h, int x, int w,
                      int r, int64_t (&S)[K]) {
  for (int j = 0; j < K; ++j) S[j] = 0;
  int64_t n = 0;
  const int lo = f - t < 0 ? 0 : f - t, hi = f + t > F - 1 ? F - 1 : f + t;
  for (int g = lo; g <= hi; ++g) {
    int ya, yb, xa, xb;
    wct_guided_up_time_box(pos, f, g, y, h, x, w, r, &ya, &yb, &xa, &xb);
    if (ya > yb || xa > xb) continue;
    n += (int64_t)(yb - ya + 1) * (xb - xa + 1);
    for (int j = 0; j < K; ++j) S[j] += win(T[(size_t)g * K + j], w, ya, yb, xa, xb);
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, fp) != 1 || ncases < 0) return 2;
  int bad = 0;
  long long pixels = 0, max_n = 0, max_a = 0, max_sa = 0, max_sb = 0, max_am = 0, max_bm = 0, max_v = 0;
  for (int k = 0; k < ncases; ++k) {
    int hd[11];
    if (fread(hd, 4, 11, fp) != 11) return 2;
    const int F = hd[0], h = hd[1], w = hd[2], hc = hd[3], wc = hd[4], H = hd[5], W = hd[6], r = hd[7], eps_q = hd[8], T = hd[9];
    if (F < 1 || hc < 1 || wc < 1 || h < hc || w < wc || H < hc || W < wc || !wct_guided_up_time_params_ok(r, eps_q, T)) return 2;
    std::vector<int32_t> posv;
    if (hd[10]) {
      posv.resize((size_t)F * 2);
      if (fread(posv.data(), 4, posv.size(), fp) != posv.size() || wct_motion_bad_step(posv.data(), F) >= 0) return 2;
    }
    const int32_t* pos = hd[10] ? posv.data() : nullptr;
    std::vector<uint8_t> s((size_t)F * h * w * 3), c((size_t)F * hc * wc * 3), C((size_t)F * H * W * 3), want(C.size());
    if (fread(s.data(), 1, s.size(), fp) != s.size() || fread(c.data(), 1, c.size(), fp) != c.size() ||
        fread(C.data(), 1, C.size(), fp) != C.size() || fread(want.data(), 1, want.size(), fp) != want.size())
      return 2;
    // step 1: per frame the planes I, I^2, p, I p and their tables
    const size_t np = (size_t)h * w;
    std::vector<std::vector<int64_t>> T8((size_t)F * 8);
    {
      std::vector<int64_t> pl[8];
      for (auto& v : pl) v.resize(np);
      for (int f = 0; f < F; ++f) {
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            const uint8_t* q = &c[(((size_t)f * hc + (y < hc ? y : hc - 1)) * wc + (x < wc ? x : wc - 1)) * 3];
            const int64_t g = wct_guided_guide(q[0], q[1], q[2]);
            const uint8_t* p = &s[(((size_t)f * h + y) * w + x) * 3];
            const size_t i = (size_t)y * w + x;
            pl[0][i] = g; pl[1][i] = g * g;
            for (int ch = 0; ch < 3; ++ch) { pl[2 + ch][i] = p[ch]; pl[5 + ch][i] = g * p[ch]; }
          }
        for (int j = 0; j < 8; ++j) T8[(size_t)f * 8 + j] = sat(pl[j].data(), h, w);
      }
    }
    std::vector<int64_t> ab((size_t)F * np * 6);                  // per frame six planes: a_q, b_q of channel 0, 1, 2
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          int64_t S[8];
          const int64_t n = window<8>(T8, pos, f, F, T, y, h, x, w, r, S);
          if (n != wct_guided_up_time_n(pos, f, F, T, y, h, x, w, r) || n < 1 || n > WCT_GUIDED_TIME_MAX_WINDOW) {
            printf("FAIL case %d: n %lld of (%d, %d, %d)\n", k, (long long)n, f, y, x);
            return 1;
          }
          if (n > max_n) max_n = n;
          for (int ch = 0; ch < 3; ++ch) {
            int32_t a, b;
            wct_guided_ab(n, S[0], S[1], S[2 + ch], S[5 + ch], eps_q, &a, &b);
            ab[((size_t)f * 6 + 2 * ch) * np + (size_t)y * w + x] = a;
            ab[((size_t)f * 6 + 2 * ch + 1) * np + (size_t)y * w + x] = b;
            if (absll(a) > max_a) max_a = absll(a);
          }
        }
    // step 2
    std::vector<std::vector<int64_t>> T6((size_t)F * 6);
    for (size_t j = 0; j < (size_t)F * 6; ++j) T6[j] = sat(&ab[j * np], h, w);
    std::vector<int32_t> am((size_t)F * np * 3), bm(am.size());
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < hc; ++y)                                // (only rows < hc and columns < wc are read afterwards)
        for (int x = 0; x < wc; ++x) {
          int64_t S[6];
          const int64_t n = window<6>(T6, pos, f, F, T, y, h, x, w, r, S);
          for (int ch = 0; ch < 3; ++ch) {
            const size_t i = (((size_t)f * h + y) * w + x) * 3 + ch;
            wct_guided_up_mean(n, S[2 * ch], S[2 * ch + 1], &am[i], &bm[i]);
            if (absll(S[2 * ch]) > max_sa) max_sa = absll(S[2 * ch]);
            if (absll(S[2 * ch + 1]) > max_sb) max_sb = absll(S[2 * ch + 1]);
            if (absll(am[i]) > max_am) max_am = absll(am[i]);
            if (absll(bm[i]) > max_bm) max_bm = absll(bm[i]);
          }
        }
    // step 3: frame f's own means and full content
    for (int f = 0; f < F; ++f)
      for (int Y = 0; Y < H; ++Y) {
        int y0, y1, fy;
        wct_guided_up_axis(Y, H, hc, &y0, &y1, &fy);
        for (int X = 0; X < W; ++X) {
          int x0, x1, fx;
          wct_guided_up_axis(X, W, wc, &x0, &x1, &fx);
          const uint8_t* q = &C[(((size_t)f * H + Y) * W + X) * 3];
          const int I = wct_guided_guide(q[0], q[1], q[2]);
          for (int ch = 0; ch < 3; ++ch) {
            const size_t fb = (size_t)f * h;
            const size_t i[4] = {((fb + y0) * w + x0) * 3 + ch, ((fb + y0) * w + x1) * 3 + ch, ((fb + y1) * w + x0) * 3 + ch,
                                 ((fb + y1) * w + x1) * 3 + ch};
            const int32_t a4[4] = {am[i[0]], am[i[1]], am[i[2]], am[i[3]]}, b4[4] = {bm[i[0]], bm[i[1]], bm[i[2]], bm[i[3]]};
            const int64_t v = wct_guided_up_sum(a4, b4, fy, fx, I);
            if (absll(v) > max_v) max_v = absll(v);
            const uint8_t got = wct_guided_up_out(v), wv = want[(((size_t)f * H + Y) * W + X) * 3 + ch];
            if (got != wv && bad++ < 10)
              printf("FAIL case %d (F %d %dx%d -> %dx%d r %d eps_q %d T %d) frame %d pixel (%d, %d, %d): %d, expected %d\n", k, F, hc, wc, H,
                     W, r, eps_q, T, f, Y, X, ch, got, wv);
          }
        }
      }
    pixels += (long long)F * H * W;
  }
  fclose(fp);
  // the header's bounds: |SA| < 33025 2^18, |SB| < 2.3e12, |am| < 2^18, |bm| < 6.8e7, |v| < 8.9e12
  if (max_sa >= 33025LL * (1 << 18) || max_sb >= 2300000000000LL || max_am >= (1 << 18) || max_bm >= 68000000 ||
      max_v >= 8900000000000LL) {
    printf("FAIL bounds: max |SA| %lld, max |SB| %lld, max |am| %lld, max |bm| %lld, max |v| %lld\n", max_sa, max_sb, max_am, max_bm,
           max_v);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld pixels, max n %lld, max |a_q| %lld, max |SA| %lld, max |SB| %lld, max |am| %lld, max |bm| %lld, "
         "max |v| %lld\n", ncases, pixels, max_n, max_a, max_sa, max_sb, max_am, max_bm, max_v);
  return 0;
}
