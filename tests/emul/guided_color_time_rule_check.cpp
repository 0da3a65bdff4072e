// Host check of wct_tf_amd/csrc/guided_color_time_rule.h (the rule the kernels of guided_color_time.hip share), built with
// -fsanitize=address,undefined by tests/test_guided_color_time_cpu.py and run as a program of its own: the signed-overflow check
// is the proof of the bounds the header restates for n <= 33025.  A frame's shifted box sum comes from 64-bit prefix sums and is at
// most (2r + 1)^2 * 65025 < 2^31; the sum of those over the frames of the window is formed in int32 on purpose: its terms are
// non-negative, so it overflows exactly when a window sum of pass 1 passes 2^31 - 1.
// usage: guided_color_time_rule_check FILE OUT.  FILE: int32 N, then N cases: int32 F, H, W, Hc, Wc, r, eps_q, T; F*2 int32
// positions; F*H*W*3 stylized bytes, F*Hc*Wc*3 content bytes.  OUT receives the F*H*W*3 filtered bytes of every case, in order.
// Then it forms the extremes itself: at (r, T) = (51, 1), (40, 2), (33, 3), clips of 2T + 1 frames of (2r + 2T + 2)^2 that drift by
// (1, -1) per frame (full windows of (2r + 1)^2 (2T + 1) pixels under non-zero shifts) -- all-255, which must come back as 255,
// and a 0 / 255 checkerboard in space that alternates in time, both at eps_q = 1 and 65025.  Prints the largest n, pass-1 sum,
// |a_q|, |b_q| and bitlength(det) met, and holds them against the header's bounds.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../wct_tf_amd/csrc/guided_color_time_rule.h"

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

struct Stats { long long max_a = 0, max_b = 0, max_n = 0, min_n = 1 << 30, max_s = 0, max_bits = 0, pixels = 0; };

static void filter(int F, int H, int W, int Hc, int Wc, int r, int eps_q, int T, const int32_t* pos, const uint8_t* s, const uint8_t* c,
                   uint8_t* out, Stats* st) {
  constexpr int KS = WCT_GUIDED_COLOR_SUMS, KC = WCT_GUIDED_COLOR_COEFFS;
  const size_t px = (size_t)F * H * W;
  std::vector<int64_t> q[KS];
  std::vector<int> guide(px * 3);
  for (auto& v : q) v.resize(px);
  for (int f = 0; f < F; ++f)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = ((size_t)f * H + y) * W + x;
        const uint8_t* cp = &c[(((size_t)f * Hc + (y < Hc ? y : Hc - 1)) * Wc + (x < Wc ? x : Wc - 1)) * 3];
        const int I[3] = {cp[0], cp[1], cp[2]}, p[3] = {s[i * 3], s[i * 3 + 1], s[i * 3 + 2]};
        unsigned d[KS];
        wct_guided_color_terms(I, p, d);
        for (int k = 0; k < KS; ++k) q[k][i] = d[k];
        for (int k = 0; k < 3; ++k) guide[i * 3 + k] = I[k];
      }
  std::vector<int32_t> S[KS];
  for (int k = 0; k < KS; ++k) S[k] = box3<int32_t>(q[k], F, H, W, r, T, pos);      // the header says each stays below 2^31
  std::vector<int64_t> ab[KC];
  for (auto& v : ab) v.resize(px);
  for (int f = 0; f < F; ++f)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = ((size_t)f * H + y) * W + x;
        const int64_t n = wct_guided_motion_n(pos, f, F, T, y, H, x, W, r);
        if (n > st->max_n) st->max_n = n;
        if (n < st->min_n) st->min_n = n;
        int64_t w[KS];
        for (int k = 0; k < KS; ++k) { w[k] = S[k][i]; if (w[k] > st->max_s) st->max_s = w[k]; }
        int32_t o[KC];
        int bits = 0;
        wct_guided_color_ab(n, w, eps_q, o, &bits);
        if (bits > st->max_bits) st->max_bits = bits;
        for (int k = 0; k < KC; ++k) {
          ab[k][i] = o[k];
          const long long v = o[k] < 0 ? -(long long)o[k] : o[k];
          if (k < 9 ? v > st->max_a : v > st->max_b) (k < 9 ? st->max_a : st->max_b) = v;
        }
      }
  std::vector<int64_t> SAB[KC];
  for (int k = 0; k < KC; ++k) SAB[k] = box3<int64_t>(ab[k], F, H, W, r, T, pos);
  for (int f = 0; f < F; ++f)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = ((size_t)f * H + y) * W + x;
        const int64_t n = wct_guided_motion_n(pos, f, F, T, y, H, x, W, r);
        for (int ch = 0; ch < 3; ++ch) {
          const int64_t SA[3] = {SAB[ch][i], SAB[3 + ch][i], SAB[6 + ch][i]};
          out[i * 3 + ch] = wct_guided_color_out(n, SA, SAB[9 + ch][i], &guide[i * 3]);
        }
      }
  st->pixels += (long long)px;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s FILE OUT\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  int ncases = 0;
  if (fread(&ncases, 4, 1, fp) != 1 || ncases < 0) return 2;
  Stats st;
  for (int k = 0; k < ncases; ++k) {
    int hd[8];
    if (fread(hd, 4, 8, fp) != 8) return 2;
    const int F = hd[0], H = hd[1], W = hd[2], Hc = hd[3], Wc = hd[4], r = hd[5], eps_q = hd[6], T = hd[7];
    if (F < 1 || F > 32 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > H || Wc > W || !wct_guided_time_params_ok(r, eps_q, T)) return 2;
    std::vector<int32_t> pos((size_t)F * 2);
    if (fread(pos.data(), 4, pos.size(), fp) != pos.size() || wct_motion_bad_step(pos.data(), F) >= 0) return 2;
    std::vector<uint8_t> s((size_t)F * H * W * 3), c((size_t)F * Hc * Wc * 3), out(s.size());
    if (fread(s.data(), 1, s.size(), fp) != s.size() || fread(c.data(), 1, c.size(), fp) != c.size()) return 2;
    filter(F, H, W, Hc, Wc, r, eps_q, T, pos.data(), s.data(), c.data(), out.data(), &st);
    if (fwrite(out.data(), 1, out.size(), fo) != out.size()) return 2;
  }
  fclose(fp);
  fclose(fo);
  // the extremes
  int bad = 0;
  const int RT[3][2] = {{51, 1}, {40, 2}, {33, 3}}, EPS[2] = {1, WCT_GUIDED_MAX_EPS};
  long long full_n = 0;
  for (auto& rt : RT) {
    const int r = rt[0], T = rt[1], F = 2 * T + 1, side = 2 * r + 2 * T + 2;
    if (wct_guided_time_radius_limit(T) != r) { printf("FAIL radius limit of T = %d is %d\n", T, wct_guided_time_radius_limit(T)); return 1; }
    std::vector<int32_t> pos((size_t)F * 2);
    for (int f = 0; f < F; ++f) { pos[2 * f] = f; pos[2 * f + 1] = -f; }
    const size_t px = (size_t)F * side * side;
    std::vector<uint8_t> white(px * 3, 255), board(px * 3), out(px * 3);
    for (int f = 0; f < F; ++f)
      for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x)
          for (int ch = 0; ch < 3; ++ch) board[((((size_t)f * side + y) * side) + x) * 3 + ch] = (uint8_t)(((f + y + x) & 1) * 255);
    for (int eps_q : EPS) {
      Stats one;
      filter(F, side, side, side, side, r, eps_q, T, pos.data(), white.data(), white.data(), out.data(), &one);
      for (size_t i = 0; i < out.size(); ++i)
        if (out[i] != 255 && bad++ < 10) printf("FAIL all-255 clip r %d T %d eps_q %d byte %zu: %d\n", r, T, eps_q, i, out[i]);
      if (one.max_n != (long long)wct_guided_time_window(r, T) || one.max_s != one.max_n * 65025) {
        printf("FAIL all-255 clip r %d T %d: max n %lld, max sum %lld\n", r, T, one.max_n, one.max_s);
        return 1;
      }
      filter(F, side, side, side, side, r, eps_q, T, pos.data(), board.data(), board.data(), out.data(), &one);
      if (one.max_n > full_n) full_n = one.max_n;
      if (one.max_a > st.max_a) st.max_a = one.max_a;
      if (one.max_b > st.max_b) st.max_b = one.max_b;
      if (one.max_s > st.max_s) st.max_s = one.max_s;
      if (one.max_bits > st.max_bits) st.max_bits = one.max_bits;
      if (one.min_n < st.min_n) st.min_n = one.min_n;
    }
  }
  if (st.max_n > WCT_GUIDED_TIME_MAX_WINDOW || full_n > WCT_GUIDED_TIME_MAX_WINDOW || st.min_n < 1 || st.max_a > WCT_GUIDED_COLOR_MAX_A ||
      st.max_b > WCT_GUIDED_COLOR_MAX_B || st.max_bits > 61) {
    printf("FAIL bounds: n %lld .. %lld (extremes %lld), max |a_q| %lld, max |b_q| %lld, det bits %lld\n", st.min_n, st.max_n, full_n,
           st.max_a, st.max_b, st.max_bits);
    return 1;
  }
  if (bad) { printf("%d mismatches\n", bad); return 1; }
  printf("all checks passed: %d cases, %lld pixels, min n %lld, max n %lld, full n %lld, max sum %lld, max |a_q| %lld, max |b_q| %lld, "
         "det bits %lld\n", ncases, st.pixels, st.min_n, st.max_n, full_n, st.max_s, st.max_a, st.max_b, st.max_bits);
  return 0;
}
