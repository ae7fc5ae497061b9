// The arithmetic of the HDBSCAN stage (hdbscan.hip, the pair consumers of plda.hip's sweep), host and device: the pair form of
// the three metrics, the one order on edges and the integer keys that carry it through the atomics
// (include/mfa_hip.h "HDBSCAN").  Plain C++: no HIP type, so the twin (hdbscan_host.cpp) builds with a host compiler alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "plda_math.hpp"

// The pair form: every point gets a row y (D doubles) and a scalar q, and the score of the unordered pair {i, j} is
//   v(i, j) = (q_i + q_j) + w · Σ_k y_ik · y_jk     (k ascending; w is 1 or 2, an exact factor)
// Products and q_i + q_j commute and the k order is one, so v(i, j) and v(j, i) are the same bits.  Larger is nearer.
//   dot (2)        y = x,          q = 0,                       w = 1
//   euclidean (1)  y = x,          q = −Σ x² (k ascending),     w = 2     the score is −|x_i − x_j|²
//   plda (0)       y_k = x_k √b_k, q = c/2 − ½ Σ a_k x_k²,      w = 1     the log-likelihood ratio of one example against one:
// at n = 1 plda_column_term gives B = b_k g with b_k = ψ/(2ψ+1) > 0, and the quadratic coefficient of g² in the column constant
// equals A's (a_k = ψ²/((ψ+1)(2ψ+1))); both are taken from plda_column_term at g = 1, and c = ½ Σ log((1+ψ)/v).
MFA_ACC_FN double pair_weight(int32_t metric) { return metric == kMetricEuclidean ? 2.0 : 1.0; }

struct PairTerm { double y, quad, logr; };   // the row's element, its addend to the quadratic sum and to the constant's sum
MFA_ACC_FN PairTerm pair_term(int32_t metric, double x, double psi) {
  PairTerm t;
  t.y = x; t.quad = 0.0; t.logr = 0.0;
  if (metric == kMetricEuclidean) t.quad = x * x;
  else if (metric == kMetricPlda) {
    const PldaTerm p = plda_column_term(1.0, psi, 1.0);
    t.y = x * sqrt(p.B);
    t.quad = p.quad * (x * x);
    t.logr = p.logr;
  }
  return t;
}
MFA_ACC_FN double pair_q(int32_t metric, double sum_quad, double sum_logr) {
  if (metric == kMetricEuclidean) return -sum_quad;
  if (metric == kMetricPlda) return 0.5 * plda_column_const(sum_logr, 0.0) - 0.5 * sum_quad;
  return 0.0;
}
MFA_ACC_FN double pair_score(double qi, double qj, double w, double dot) { return (qi + qj) + w * dot; }

// A point's core score from its list of the k best other points (k = min_samples − 1: scikit-learn counts the point itself):
// the k-th entry, −inf when the list is short; k = 0: +inf.  The mutual-reachability score of a pair:
MFA_ACC_FN double pair_min(double a, double b) { return b < a ? b : a; }
MFA_ACC_FN double mreach_score(double v, double core_i, double core_j) { return pair_min(v, pair_min(core_i, core_j)); }

// The one strict order on edges: the larger score first, then the smaller min(i, j), then the smaller max(i, j).  Mutual
// reachability makes very many equal scores; under a strict total order the minimum spanning tree is unique, and Borůvka's
// choices can close no cycle.
MFA_ACC_FN bool edge_better(double m1, int32_t lo1, int32_t hi1, double m2, int32_t lo2, int32_t hi2) {
  return m1 > m2 || (m1 == m2 && (lo1 < lo2 || (lo1 == lo2 && hi1 < hi2)));
}
// The same for two candidates of one row i (other ends j1, j2 >= 0).
MFA_ACC_FN bool row_edge_better(int32_t i, double m1, int32_t j1, double m2, int32_t j2) {
  return edge_better(m1, i < j1 ? i : j1, i < j1 ? j1 : i, m2, i < j2 ? i : j2, i < j2 ? j2 : i);
}

// Integer keys that preserve the order, for the 64-bit integer atomics: a score that is no NaN as an unsigned key that
// ascends with it (never 0: 0 is "no edge"), and the pair as (lo << 32) | hi, smaller is better.
MFA_ACC_FN uint64_t score_key(double m) {
  union { double d; uint64_t u; } x;
  x.d = m + 0.0;                        // −0 (which no pair score is: its last addend is never −0) would order below +0
  return (x.u >> 63) ? ~x.u : (x.u | ((uint64_t)1 << 63));
}
MFA_ACC_FN double key_score(uint64_t key) {
  union { double d; uint64_t u; } x;
  x.u = (key >> 63) ? (key & ~((uint64_t)1 << 63)) : ~key;
  return x.d;
}
MFA_ACC_FN uint64_t pair_key(int32_t i, int32_t j) {
  return i < j ? ((uint64_t)(uint32_t)i << 32) | (uint32_t)j : ((uint64_t)(uint32_t)j << 32) | (uint32_t)i;
}

constexpr int kHdbscanMaxRounds = 40;   // each round at least halves the components: 31 rounds at 2^31 points; this is the net under it

// 0 fine, -1 a negative count, -2 D outside [1, 1024], -3 k outside [0, 64], -5 2^31 points or more.
MFA_ACC_FN int hdbscan_check_shape(int32_t D, int32_t k, int64_t N) {
  if (k == 0) return plda_check_shape(D, 1, N, N);
  return plda_check_shape(D, k, N, N);
}
