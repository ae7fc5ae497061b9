// Host twins of the PLDA stage (plda.hip): the transform, the prepare step and the sweep with its selections, the contracts
// of include/mfa_hip.h ("PLDA") on host arrays, in plain loops.  No context, no device, no HIP header: this file and
// plda_math.hpp (with the header it includes) are all tests/native/plda_check.cpp needs.  The algorithm is restated from its
// description; Kaldi's source is not among this project's references.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/mfa_hip.h"
#include "plda_math.hpp"

namespace {

struct Outputs {
  double *scores; int32_t *best_idx; double *best_score; int32_t *knn_idx; double *knn_score;
  uint64_t *bits = nullptr; double threshold = 0.0;   // the neighbour words [Nt][ceil(Ns / 64)] and their threshold
};

// 0 go on, 1 nothing to do, negative: the twin's return code
int score_checks(int64_t Nt, int64_t Ns, int D, int k, const void *test, const Outputs &o) {
  const bool knn = o.knn_idx || o.knn_score;
  const int rc = plda_check_shape(D, knn ? k : 1, Nt, Ns);
  if (rc) return rc;
  if (Nt == 0) return 1;
  if (!o.scores && !o.best_idx && !o.best_score && !knn && !o.bits) return -7;
  if (o.bits && o.threshold != o.threshold) return -9;
  if ((o.best_idx != nullptr) != (o.best_score != nullptr) || (o.knn_idx != nullptr) != (o.knn_score != nullptr)) return -1;
  if (!test) return -1;
  return 0;
}

// metrics 1 and 2 (plda_math.hpp)
void prepare_metric(const double *train, int64_t Ns, int D, int32_t metric, double *A, double *B, double *c) {
  for (int64_t j = 0; j < Ns; j++) {
    double sum = 0.0;
    for (int k = 0; k < D; k++) {
      const double g = train[(size_t)j * D + k];
      A[(size_t)j * D + k] = metric_term_A(metric);
      B[(size_t)j * D + k] = metric_term_B(metric, g);
      sum = metric_const_add(metric, sum, g);
    }
    c[j] = metric_const(metric, sum);
  }
}

int prepare(const double *train, int64_t Ns, int D, const int32_t *train_n, const double *psi, double *A, double *B, double *c) {
  for (int k = 0; k < D; k++)
    if (!plda_psi_ok(psi[k])) return -4;
  for (int64_t j = 0; j < Ns; j++)
    if (train_n && train_n[j] < 1) return -6;
  for (int64_t j = 0; j < Ns; j++) {
    const double n = train_n ? (double)train_n[j] : 1.0;
    double s_logr = 0.0, s_quad = 0.0;
    for (int k = 0; k < D; k++) {
      const PldaTerm t = plda_column_term(train[(size_t)j * D + k], psi[k], n);
      A[(size_t)j * D + k] = t.A;
      B[(size_t)j * D + k] = t.B;
      s_logr += t.logr; s_quad += t.quad;
    }
    c[j] = plda_column_const(s_logr, s_quad);
  }
  return 0;
}

void sweep(const double *test, int64_t Nt, int D, const double *A, const double *B, const double *c, int64_t Ns, int exclude_diag, int k,
           const Outputs &o) {
  const int keff = o.knn_idx ? k : (o.best_idx ? 1 : 0);
  const double ninf = -std::numeric_limits<double>::infinity();
  std::vector<double> ls((size_t)(keff > 0 ? keff : 1));
  std::vector<int32_t> li((size_t)(keff > 0 ? keff : 1));
  const size_t W = (size_t)((Ns + 63) / 64);
  for (int64_t i = 0; i < Nt; i++) {
    const double *p = test + (size_t)i * D;
    for (int e = 0; e < keff; e++) { ls[e] = ninf; li[e] = -1; }
    if (o.bits)
      for (size_t w = 0; w < W; w++) o.bits[(size_t)i * W + w] = 0;
    for (int64_t j = 0; j < Ns; j++) {
      const double *Aj = A + (size_t)j * D, *Bj = B + (size_t)j * D;
      double s = c[j];
      for (int k0 = 0; k0 < D; k0 += 4) {              // the device's step: four (p p) A, then four p B
        const int k1 = k0 + 4 < D ? k0 + 4 : D;
        for (int kk = k0; kk < k1; kk++) s += (p[kk] * p[kk]) * Aj[kk];
        for (int kk = k0; kk < k1; kk++) s += p[kk] * Bj[kk];
      }
      if (o.scores) o.scores[(size_t)i * Ns + j] = s;
      if (o.bits && plda_neighbor(s, o.threshold)) o.bits[(size_t)i * W + (size_t)(j >> 6)] |= (uint64_t)1 << (j & 63);
      if (keff == 0 || !plda_candidate(s) || (exclude_diag && j == i)) continue;
      if (!plda_better(s, (int32_t)j, ls[keff - 1], li[keff - 1])) continue;
      int pos = keff - 1;
      while (pos > 0 && plda_better(s, (int32_t)j, ls[pos - 1], li[pos - 1])) { ls[pos] = ls[pos - 1]; li[pos] = li[pos - 1]; pos--; }
      ls[pos] = s; li[pos] = (int32_t)j;
    }
    if (o.best_idx) { o.best_idx[i] = li[0]; o.best_score[i] = ls[0]; }
    if (o.knn_idx)
      for (int e = 0; e < k; e++) { o.knn_idx[(size_t)i * k + e] = li[e]; o.knn_score[(size_t)i * k + e] = ls[e]; }
  }
}

}  // namespace

extern "C" MFA_API int mfa_debug_plda_transform_host(const double *h_x, int64_t n, int32_t D, const double *h_transform,
                                                     const double *h_offset, const double *h_psi, const int32_t *h_num_examples,
                                                     int32_t norm, double *h_out) {
  const int rc = plda_check_shape(D, 1, n, 0);
  if (rc) return rc;
  if (norm < 0 || norm > 2) return -1;
  if (n == 0) return 0;
  if (!h_x || !h_transform || !h_offset || !h_out || (norm == 2 && !h_psi) || h_x == h_out) return -1;
  for (int64_t r = 0; r < n; r++) {
    const double *x = h_x + (size_t)r * D;
    double *u = h_out + (size_t)r * D;
    for (int j = 0; j < D; j++) {
      double s = h_offset[j];
      for (int k = 0; k < D; k++) s += x[k] * h_transform[(size_t)j * D + k];
      u[j] = s;
    }
    if (norm == 0) continue;
    const double inv_n = 1.0 / (double)(h_num_examples ? h_num_examples[r] : 1);
    double sum = 0.0;
    for (int k = 0; k < D; k++) sum += plda_norm_term(u[k], norm == 2 ? h_psi[k] : 0.0, inv_n, norm);
    const double f = std::sqrt((double)D / sum);
    for (int k = 0; k < D; k++) u[k] *= f;
  }
  return 0;
}

extern "C" MFA_API int mfa_debug_plda_prepare_host(const double *h_train, int64_t n_train, int32_t D, const int32_t *h_train_n,
                                                   const double *h_psi, double *h_A, double *h_B, double *h_c) {
  const int rc = plda_check_shape(D, 1, 0, n_train);
  if (rc) return rc;
  if (!h_psi) return -1;
  if (n_train > 0 && (!h_train || !h_A || !h_B || !h_c)) return -1;
  return prepare(h_train, n_train, D, h_train_n, h_psi, h_A, h_B, h_c);
}

extern "C" MFA_API int mfa_debug_plda_sweep_host(const double *h_test, int64_t n_test, int32_t D, const double *h_A, const double *h_B,
                                                 const double *h_c, int64_t n_train, int32_t exclude_diagonal, int32_t k,
                                                 double *h_scores, int32_t *h_best_idx, double *h_best_score, int32_t *h_knn_idx,
                                                 double *h_knn_score) {
  const Outputs o{h_scores, h_best_idx, h_best_score, h_knn_idx, h_knn_score};
  const int st = score_checks(n_test, n_train, D, k, h_test, o);
  if (st) return st < 0 ? st : 0;
  if (n_train > 0 && (!h_A || !h_B || !h_c)) return -1;
  sweep(h_test, n_test, D, h_A, h_B, h_c, n_train, exclude_diagonal, k, o);
  return 0;
}

extern "C" MFA_API int mfa_debug_plda_score_host(const double *h_test, int64_t n_test, const double *h_train, int64_t n_train, int32_t D,
                                                 const int32_t *h_train_n, const double *h_psi, int32_t exclude_diagonal, int32_t k,
                                                 double *h_scores, int32_t *h_best_idx, double *h_best_score, int32_t *h_knn_idx,
                                                 double *h_knn_score) {
  const Outputs o{h_scores, h_best_idx, h_best_score, h_knn_idx, h_knn_score};
  const int st = score_checks(n_test, n_train, D, k, h_test, o);
  if (st) return st < 0 ? st : 0;
  if (!h_psi || (n_train > 0 && !h_train)) return -1;
  std::vector<double> A((size_t)n_train * D), B((size_t)n_train * D), c((size_t)n_train);
  const int rc = prepare(h_train, n_train, D, h_train_n, h_psi, A.data(), B.data(), c.data());
  if (rc) return rc;
  sweep(h_test, n_test, D, A.data(), B.data(), c.data(), n_train, exclude_diagonal, k, o);
  return 0;
}

// The neighbour entries' twins: mfa_neighbor_bits_batch and mfa_debug_neighbor_sweep_batch in plain loops.  Return codes as the
// scoring twin's, and -8 an unknown metric, -9 a threshold that is not a number.
extern "C" MFA_API int mfa_debug_neighbor_bits_host(const double *h_test, int64_t n_test, const double *h_train, int64_t n_train, int32_t D,
                                                    int32_t metric, const int32_t *h_train_n, const double *h_psi, int32_t exclude_diagonal,
                                                    int32_t k, double threshold, double *h_scores, int32_t *h_best_idx, double *h_best_score,
                                                    int32_t *h_knn_idx, double *h_knn_score, uint64_t *h_bits) {
  const Outputs o{h_scores, h_best_idx, h_best_score, h_knn_idx, h_knn_score, h_bits, threshold};
  if (!plda_metric_ok(metric)) return -8;
  const int st = score_checks(n_test, n_train, D, k, h_test, o);
  if (st) return st < 0 ? st : 0;
  if ((metric == kMetricPlda && !h_psi) || (n_train > 0 && !h_train)) return -1;
  std::vector<double> A((size_t)n_train * D), B((size_t)n_train * D), c((size_t)n_train);
  if (metric == kMetricPlda) {
    const int rc = prepare(h_train, n_train, D, h_train_n, h_psi, A.data(), B.data(), c.data());
    if (rc) return rc;
  } else {
    prepare_metric(h_train, n_train, D, metric, A.data(), B.data(), c.data());
  }
  sweep(h_test, n_test, D, A.data(), B.data(), c.data(), n_train, exclude_diagonal, k, o);
  return 0;
}

extern "C" MFA_API int mfa_debug_neighbor_sweep_host(const double *h_test, int64_t n_test, int32_t D, const double *h_A, const double *h_B,
                                                     const double *h_c, int64_t n_train, int32_t exclude_diagonal, int32_t k,
                                                     double threshold, double *h_scores, int32_t *h_best_idx, double *h_best_score,
                                                     int32_t *h_knn_idx, double *h_knn_score, uint64_t *h_bits) {
  const Outputs o{h_scores, h_best_idx, h_best_score, h_knn_idx, h_knn_score, h_bits, threshold};
  const int st = score_checks(n_test, n_train, D, k, h_test, o);
  if (st) return st < 0 ? st : 0;
  if (n_train > 0 && (!h_A || !h_B || !h_c)) return -1;
  sweep(h_test, n_test, D, h_A, h_B, h_c, n_train, exclude_diagonal, k, o);
  return 0;
}
