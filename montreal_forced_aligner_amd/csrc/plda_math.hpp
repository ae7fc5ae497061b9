// The arithmetic of the PLDA stage (plda.hip), host and device: the contract of include/mfa_hip.h ("PLDA") where both sides
// run the same operations, and the limits both refuse.  The prepare kernel and its host twin (plda_host.cpp) run exactly
// plda_column_term and plda_column_const's operations, so A and B have the same bits on either side (basic IEEE operations
// only); c may differ in the last places by log1p alone.  The list order plda_better is the one order of every selection.
// Plain C++: no HIP type, so the twins build with a host compiler alone (tests/native/plda_check.cpp).
#pragma once
#include <stdint.h>

#include "gmm_acc_math.hpp"   // MFA_ACC_FN

constexpr int kPldaMaxDim = 1024;
constexpr int kPldaMaxK = 64;          // a row's list is one wavefront register pair: lane j holds the j-th best

// 0 fine, -1 a count that is no count, -2 D outside [1, 1024], -3 k outside [1, 64], -5 2^31 rows or columns or more.
// (-4: a psi entry that is not positive and finite; -6: a train_n below 1; -7: every output NULL — checked by the callers.)
MFA_ACC_FN int plda_check_shape(int32_t D, int32_t k, int64_t n_test, int64_t n_train) {
  if (n_test < 0 || n_train < 0) return -1;
  if (D <= 0 || D > kPldaMaxDim) return -2;
  if (k <= 0 || k > kPldaMaxK) return -3;
  if (n_test >= ((int64_t)1 << 31) || n_train >= ((int64_t)1 << 31)) return -5;
  return 0;
}

MFA_ACC_FN bool plda_psi_ok(double psi) { return psi > 0.0 && psi * 0.0 == 0.0; }   // positive and finite

// Element k of train column j: with a = n psi / (n psi + 1) and v = 1 + psi / (n psi + 1),
//   A = -1/2 (1/v - 1/(1 + psi)) = -1/2 psi a / (v (1 + psi)),  B = (a g) / v,
// and the column constant's two terms log((1 + psi) / v) = log1p(psi a / v) and (a g)^2 / v.  The forms on the right are the
// ones computed: products and quotients of positive numbers, no difference of nearly equal ones, so each carries a relative
// error of a few roundings whatever psi and n are.
struct PldaTerm { double A, B, logr, quad; };
MFA_ACC_FN PldaTerm plda_column_term(double g, double psi, double n) {
  const double npsi = n * psi;
  const double npsi1 = npsi + 1.0;
  const double a = npsi / npsi1;
  const double v = 1.0 + psi / npsi1;
  const double ag = a * g;
  const double pa = psi * a;
  PldaTerm t;
  t.A = -0.5 * (pa / (v * (1.0 + psi)));
  t.B = ag / v;
  t.logr = log1p(pa / v);
  t.quad = ag * ag / v;
  return t;
}
// c = -1/2 (sum log v - sum log(1 + psi) + sum (a g)^2 / v) = 1/2 (sum log((1 + psi) / v) - sum (a g)^2 / v), each sum over k
// ascending: two sums of terms that are not negative, one difference
MFA_ACC_FN double plda_column_const(double sum_logr, double sum_quad) { return 0.5 * (sum_logr - sum_quad); }

// The order of every list: the larger score first, at equal scores the lower index.  Only finite scores are candidates, so
// an empty entry (-inf, -1) is worse than every candidate.
MFA_ACC_FN bool plda_better(double s1, int32_t i1, double s2, int32_t i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }
MFA_ACC_FN bool plda_candidate(double s) { return s - s == 0.0; }   // finite: not NaN, not an infinity

// The neighbour matrix's bit: a plain comparison on the accumulator value, false for a NaN on either side.
MFA_ACC_FN bool plda_neighbor(double s, double threshold) { return s >= threshold; }

// The sweep's metrics: each is a prepare step (A, B, c) for the same arithmetic c_j + sum p^2 A + sum p B.
//   0 plda: plda_column_term / plda_column_const;
//   1 euclidean: A = -1, B = 2 g, c = -sum_k g^2 (k ascending): the score is -|p - g|^2 expanded;
//   2 dot: A = 0, B = g, c = 0: the score is p . g (the cosine of rows made unit length beforehand).
constexpr int kMetricPlda = 0, kMetricEuclidean = 1, kMetricDot = 2;
MFA_ACC_FN bool plda_metric_ok(int32_t metric) { return metric >= kMetricPlda && metric <= kMetricDot; }
MFA_ACC_FN double metric_term_A(int32_t metric) { return metric == kMetricEuclidean ? -1.0 : 0.0; }
MFA_ACC_FN double metric_term_B(int32_t metric, double g) { return metric == kMetricEuclidean ? 2.0 * g : g; }
MFA_ACC_FN double metric_const_add(int32_t metric, double sum, double g) { return metric == kMetricEuclidean ? sum + g * g : sum; }
MFA_ACC_FN double metric_const(int32_t metric, double sum) { return metric == kMetricEuclidean ? -sum : 0.0; }

// A row's length-normalisation factor from its sum: norm 0 none (1), 1 simple: sqrt(D / sum u_k^2), 2 the model's:
// sqrt(D / sum u_k^2 / (psi_k + 1/n)).
MFA_ACC_FN double plda_norm_term(double u, double psi, double inv_n, int norm) {
  return norm == 2 ? u * u / (psi + inv_n) : u * u;
}
