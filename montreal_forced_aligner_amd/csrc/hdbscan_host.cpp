// Host twins of the HDBSCAN stage (hdbscan.hip): the pair form's prepare step, the scores v, the core scores and the spanning
// tree, the contracts of include/mfa_hip.h ("HDBSCAN") on host arrays, in plain loops.  No context, no device, no HIP header:
// this file and hdbscan_math.hpp (with the headers it includes) are all tests/native/hdbscan_check.cpp needs.  The tree twin is
// Kruskal under edge_better: under a strict total order every correct algorithm returns the same edges.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/mfa_hip.h"
#include "hdbscan_math.hpp"

namespace {

// The sweep's sum for the pair form: the accumulator starts from c = 0, k ascending (the A operand is 0: its products add +0).
double pair_dot(const double *yi, const double *yj, int D) {
  double s = 0.0;
  for (int k = 0; k < D; k++) s += yi[k] * yj[k];
  return s;
}

struct Edge { double m; int32_t lo, hi; };

int32_t find(std::vector<int32_t> &parent, int32_t x) {
  while (parent[(size_t)x] != x) {
    parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    x = parent[(size_t)x];
  }
  return x;
}

}  // namespace

extern "C" MFA_API int mfa_debug_hdbscan_core_host(const double *h_x, int64_t N, int32_t D, int32_t metric, const double *h_psi, int32_t k,
                                                   double *h_y, double *h_q, double *h_core, double *h_v, const double *h_v_in) {
  if (!plda_metric_ok(metric)) return -8;
  const int rc = hdbscan_check_shape(D, k, N);
  if (rc) return rc;
  if (N == 0) return 0;
  if (!h_x || !h_y || !h_q || !h_core || (metric == kMetricPlda && !h_psi)) return -1;
  if (metric == kMetricPlda)
    for (int d = 0; d < D; d++)
      if (!plda_psi_ok(h_psi[d])) return -4;
  for (int64_t i = 0; i < N; i++) {
    double s_quad = 0.0, s_logr = 0.0;
    for (int d = 0; d < D; d++) {
      const PairTerm t = pair_term(metric, h_x[(size_t)i * D + d], metric == kMetricPlda ? h_psi[d] : 1.0);
      h_y[(size_t)i * D + d] = t.y;
      s_quad += t.quad;
      s_logr += t.logr;
    }
    h_q[i] = pair_q(metric, s_quad, s_logr);
  }
  const double w = pair_weight(metric), ninf = -std::numeric_limits<double>::infinity();
  std::vector<double> ls((size_t)(k > 0 ? k : 1));
  std::vector<int32_t> li((size_t)(k > 0 ? k : 1));
  for (int64_t i = 0; i < N; i++) {
    for (int e = 0; e < k; e++) { ls[(size_t)e] = ninf; li[(size_t)e] = -1; }
    if (k > 0 || h_v)
      for (int64_t j = 0; j < N; j++) {
        const double s = h_v_in ? h_v_in[(size_t)i * N + j]
                                : pair_score(h_q[i], h_q[j], w, pair_dot(h_y + (size_t)i * D, h_y + (size_t)j * D, D));
        if (h_v) h_v[(size_t)i * N + j] = s;
        if (k == 0 || !plda_candidate(s) || j == i) continue;
        if (!plda_better(s, (int32_t)j, ls[(size_t)k - 1], li[(size_t)k - 1])) continue;
        int pos = k - 1;
        while (pos > 0 && plda_better(s, (int32_t)j, ls[(size_t)pos - 1], li[(size_t)pos - 1])) {
          ls[(size_t)pos] = ls[(size_t)pos - 1]; li[(size_t)pos] = li[(size_t)pos - 1]; pos--;
        }
        ls[(size_t)pos] = s; li[(size_t)pos] = (int32_t)j;
      }
    h_core[i] = k > 0 ? ls[(size_t)k - 1] : std::numeric_limits<double>::infinity();
  }
  return 0;
}

extern "C" MFA_API int mfa_debug_hdbscan_mst_host(const double *h_y, const double *h_q, const double *h_core, const double *h_v, int64_t N,
                                                  int32_t D, int32_t metric, int32_t *h_edge_lo, int32_t *h_edge_hi, double *h_edge_score,
                                                  int32_t *h_n_edges) {
  if (!plda_metric_ok(metric)) return -8;
  const int rc = hdbscan_check_shape(D, 0, N);
  if (rc) return rc;
  if (!h_n_edges) return -1;
  *h_n_edges = 0;
  if (N <= 1) return 0;
  if ((!h_v && (!h_y || !h_q)) || !h_core || !h_edge_lo || !h_edge_hi || !h_edge_score) return -1;
  const double w = pair_weight(metric);
  std::vector<Edge> edges;
  for (int64_t i = 0; i < N; i++)
    for (int64_t j = i + 1; j < N; j++) {
      const double s = h_v ? h_v[(size_t)i * N + j] : pair_score(h_q[i], h_q[j], w, pair_dot(h_y + (size_t)i * D, h_y + (size_t)j * D, D));
      if (!plda_candidate(s)) continue;
      edges.push_back(Edge{mreach_score(s, h_core[i], h_core[j]), (int32_t)i, (int32_t)j});
    }
  std::sort(edges.begin(), edges.end(), [](const Edge &a, const Edge &b) { return edge_better(a.m, a.lo, a.hi, b.m, b.lo, b.hi); });
  std::vector<int32_t> parent((size_t)N);
  std::iota(parent.begin(), parent.end(), 0);
  int32_t n = 0;
  for (const Edge &e : edges) {
    const int32_t a = find(parent, e.lo), b = find(parent, e.hi);
    if (a == b) continue;
    parent[(size_t)(a < b ? b : a)] = a < b ? a : b;
    h_edge_lo[n] = e.lo; h_edge_hi[n] = e.hi; h_edge_score[n] = e.m;
    n++;
    if (n == N - 1) break;
  }
  *h_n_edges = n;
  return 0;
}
