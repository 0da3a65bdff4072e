// Host check of csrc/pool_rule.h, the rule the banded path pools chunk statistics by: a stand-alone program (its own main; build
// it with any host sanitizer), fed by tests/test_banded_cpu.py with chunk statistics and the statistics of the concatenation,
// all in double.  File: int32 cases; per case int32 K, C; int32 n[K]; double means[K][C], covs[K][C][C], mean[C], cov[C][C].
// Passes when every pooled value is within 1e-12 of the largest expected one (mean and covariance each), and K = 1 hands its
// input back exactly.
#include "../../wct_tf_amd/csrc/pool_rule.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

template <typename T>
static bool read(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t cases = 0;
  if (fread(&cases, 4, 1, f) != 1) return 2;
  int bad = 0;
  for (int t = 0; t < cases; ++t) {
    int32_t hdr[2];
    if (fread(hdr, 4, 2, f) != 2) return 2;
    const int K = hdr[0], C = hdr[1];
    const size_t cc = (size_t)C * C;
    std::vector<int32_t> n;
    std::vector<double> means, covs, mean, cov;
    if (!read(f, &n, K) || !read(f, &means, (size_t)K * C) || !read(f, &covs, K * cc) || !read(f, &mean, C) || !read(f, &cov, cc)) return 2;
    std::vector<int> ni(n.begin(), n.end());
    std::vector<double> gm(C), gc(cc);
    wct_pool_all(means.data(), covs.data(), ni.data(), K, C, gm.data(), gc.data());
    double mmax = 0, cmax = 0, merr = 0, cerr = 0;
    for (int c = 0; c < C; ++c) { mmax = std::fmax(mmax, std::fabs(mean[c])); merr = std::fmax(merr, std::fabs(gm[c] - mean[c])); }
    for (size_t e = 0; e < cc; ++e) { cmax = std::fmax(cmax, std::fabs(cov[e])); cerr = std::fmax(cerr, std::fabs(gc[e] - cov[e])); }
    bool ok = merr <= 1e-12 * mmax && cerr <= 1e-12 * cmax;
    if (K == 1) {
      for (int c = 0; c < C; ++c) ok = ok && gm[c] == means[c];
      for (size_t e = 0; e < cc; ++e) ok = ok && gc[e] == covs[e];
    }
    for (int i = 0; i < C; ++i)
      for (int j = 0; j < i; ++j) ok = ok && gc[(size_t)i * C + j] == gc[(size_t)j * C + i] ;   // (given symmetric chunk covariances)
    printf("case %d: K = %d, C = %d: mean err %.3g of %.3g, cov err %.3g of %.3g%s\n", t, K, C, merr, mmax, cerr, cmax, ok ? "" : "  FAILED");
    bad += !ok;
  }
  fclose(f);
  if (bad) { printf("%d of %d cases FAILED\n", bad, (int)cases); return 1; }
  printf("all checks passed: %d cases\n", (int)cases);
  return 0;
}
