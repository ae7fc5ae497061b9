// The arithmetic of the silhouette stage (silhouette.hip, the silhouette consumer of plda.hip's sweep), host and device: the
// distance of a pair score, the order of a cluster sum, the fold of a cluster's mean into a row's a and b, and the finish
// (include/mfa_hip.h "Silhouette").  Plain C++: no HIP type, so the twin (silhouette_host.cpp) builds with a host compiler alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hdbscan_math.hpp"

// The distance of a pair from its score v (hdbscan_math.hpp; larger is nearer), the rules of stats.score_to_distance:
// plda −v (the signed −LLR as it is), euclidean sqrt(max(−v, 0)) (v = −|x_i − x_j|²; a NaN stays one), dot 1 − v.
MFA_ACC_FN double sil_distance(int32_t metric, double v) {
  if (metric == kMetricPlda) return -v;
  if (metric == kMetricEuclidean) {
    const double m = -v;
    return sqrt(m < 0.0 ? 0.0 : m);
  }
  return 1.0 - v;
}

// The order of a cluster sum S(i, c) = Σ d(i, j), j in c, j != i: column j adds to partial (j & 63) >> 4 of four, each from
// +0 over its columns ascending; S = (P0 + P1) + (P2 + P3).  On the device a partial is one lane's running sum (a lane reads
// 16 contiguous columns of every 64-column step) and the two additions are the xor-16 and xor-32 shuffles.
constexpr int kSilPartials = 4;
MFA_ACC_FN int sil_partial(int64_t j) { return (int)((j & 63) >> 4); }
MFA_ACC_FN double sil_combine(double p0, double p1, double p2, double p3) { return (p0 + p1) + (p2 + p3); }

// A row's state over the clusters, taken in ascending order: a from its own cluster (0 for a singleton), b the least mean
// over the others, the first of equal ones (a NaN mean is never taken), bj its cluster (−1: none).
struct SilRow { double a, b; int32_t bj; };
MFA_ACC_FN SilRow sil_row_init() {
  SilRow r;
  r.a = 0.0; r.b = INFINITY; r.bj = -1;
  return r;
}
MFA_ACC_FN void sil_fold(SilRow &r, int32_t own, int32_t c, double S, int64_t n_c) {
  if (c == own) {
    r.a = n_c > 1 ? S / (double)(n_c - 1) : 0.0;
  } else {
    const double m = S / (double)n_c;
    if (m < r.b) { r.b = m; r.bj = c; }
  }
}
// scikit-learn's rules: a singleton scores 0; den = max(a, b), den == 0 scores 0.
MFA_ACC_FN double sil_finish(int64_t n_own, double a, double b) {
  if (n_own == 1) return 0.0;
  const double den = a < b ? b : a;
  if (den == 0.0) return 0.0;
  return (b - a) / den;
}

// Offsets off [C + 1] of the clusters' column ranges: off[0] = 0, off[C] = N, strictly ascending.  One entry's check:
MFA_ACC_FN bool sil_offset_ok(int32_t lo, int32_t hi, int32_t c, int32_t C, int64_t N) {
  return lo >= 0 && lo < hi && (int64_t)hi <= N && (c != 0 || lo == 0) && (c != C - 1 || (int64_t)hi == N);
}
// The cluster of column j under valid offsets: the last c with off[c] <= j (a search that stays inside [0, C − 1] on any input).
MFA_ACC_FN int32_t sil_cluster_of(const int32_t *off, int32_t C, int64_t j) {
  int32_t lo = 0, hi = C - 1;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)off[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// 0 fine, -1 a negative count, -2 D outside [1, 1024], -5 2^31 points or more, -6 C outside [2, N] (N > 0).
MFA_ACC_FN int sil_check_shape(int32_t D, int64_t N, int32_t C) {
  const int rc = hdbscan_check_shape(D, 0, N);
  if (rc) return rc;
  if (N > 0 && (C < 2 || (int64_t)C > N)) return -6;
  return 0;
}
