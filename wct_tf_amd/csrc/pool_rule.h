// Pooling the statistics of K chunks of rows into the statistics of their concatenation: the rule of the banded stylize path
// (banded.hip), shared by its kernels and by any host program (plain C++: nothing of HIP is needed to include this file).
// Chunks k = 0 .. K - 1 in order, chunk k with n[k] rows, mean m_k [C] and covariance S_k [C][C] normalised by n[k] - 1:
//   N   = sum_k n[k]
//   m   = sum_k n[k] m_k / N
//   Cov = [sum_k (n[k] - 1) S_k + sum_k n[k] (m_k - m)(m_k - m)^T] / (N - 1)
// All arithmetic in double, every sum in chunk order from 0; the caller rounds a result once to the precision it keeps (the
// library: fp32, and wct_tf's diagonal eps is added to the rounded value -- once, after the pooling).  The within-chunk sum
// sum_k (n[k] - 1) S_k is a running sum (wct_pool_within): the library adds a group of chunks at a time and keeps it in a double
// buffer between the groups.  The between-chunk term is n (a b), not (n a) b: Cov[i][j] and Cov[j][i] are the same bits.
// K = 1 has nothing to pool: wct_pool_all hands the chunk's statistics back unchanged (the library never pools one chunk).
#pragma once

#if defined(__HIPCC__)
#define WCT_POOL_HD __host__ __device__
#else
#define WCT_POOL_HD
#endif

// the pooled mean of channel c; means [K][C]
template <typename T>
WCT_POOL_HD inline double wct_pool_mean(const T* means, const int* n, int K, int C, int c) {
  double s = 0.0, N = 0.0;
  for (int k = 0; k < K; ++k) {
    s += (double)n[k] * (double)means[(long long)k * C + c];
    N += (double)n[k];
  }
  return s / N;
}

// the running within-chunk sum of one matrix element after a chunk of n rows whose covariance element is S
template <typename T>
WCT_POOL_HD inline double wct_pool_within(double acc, T S, int n) { return acc + (double)(n - 1) * (double)S; }

// element (i, j) of the pooled covariance: `within` its finished running sum, mi / mj the pooled means of channels i and j
template <typename T>
WCT_POOL_HD inline double wct_pool_cov(double within, const T* means, const int* n, int K, int C, int i, int j, double mi, double mj) {
  double b = 0.0, N = 0.0;
  for (int k = 0; k < K; ++k) {
    const double di = (double)means[(long long)k * C + i] - mi, dj = (double)means[(long long)k * C + j] - mj;
    b += (double)n[k] * (di * dj);
    N += (double)n[k];
  }
  return (within + b) / (N - 1.0);
}

// the whole rule on the host: means [K][C], covs [K][C][C] -> mean [C], cov [C][C]
template <typename T>
inline void wct_pool_all(const T* means, const T* covs, const int* n, int K, int C, double* mean, double* cov) {
  const long long cc = (long long)C * C;
  if (K == 1) {
    for (int c = 0; c < C; ++c) mean[c] = (double)means[c];
    for (long long e = 0; e < cc; ++e) cov[e] = (double)covs[e];
    return;
  }
  for (int c = 0; c < C; ++c) mean[c] = wct_pool_mean(means, n, K, C, c);
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) {
      double within = 0.0;
      for (int k = 0; k < K; ++k) within = wct_pool_within(within, covs[k * cc + (long long)i * C + j], n[k]);
      cov[(long long)i * C + j] = wct_pool_cov(within, means, n, K, C, i, j, mean[i], mean[j]);
    }
}
