// Host twin of the silhouette stage (silhouette.hip): the contract of include/mfa_hip.h ("Silhouette") on host arrays, in plain
// loops and in the documented order of every sum.  No context, no device, no HIP header: this file and silhouette_math.hpp (with
// the headers it includes) are all tests/native/silhouette_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "silhouette_math.hpp"

namespace {

// The sweep's sum for the pair form: the accumulator starts from c = 0, k ascending.
double pair_dot(const double *yi, const double *yj, int D) {
  double s = 0.0;
  for (int k = 0; k < D; k++) s += yi[k] * yj[k];
  return s;
}

}  // namespace

extern "C" MFA_API int mfa_debug_silhouette_host(const double *h_x, int64_t N, int32_t D, int32_t metric, const double *h_psi,
                                                 const int32_t *h_off, int32_t C, double *h_sil, double *h_a, double *h_b, int32_t *h_bj,
                                                 double *h_v, const double *h_v_in) {
  if (!plda_metric_ok(metric)) return -8;
  const int rc = sil_check_shape(D, N, C);
  if (rc) return rc;
  if (N == 0) return 0;
  if (!h_x || !h_off || !h_sil || (metric == kMetricPlda && !h_psi)) return -1;
  if (metric == kMetricPlda)
    for (int d = 0; d < D; d++)
      if (!plda_psi_ok(h_psi[d])) return -4;
  for (int32_t c = 0; c < C; c++)
    if (!sil_offset_ok(h_off[c], h_off[c + 1], c, C, N)) return -7;
  std::vector<double> y((size_t)N * D), q((size_t)N);
  for (int64_t i = 0; i < N; i++) {
    double s_quad = 0.0, s_logr = 0.0;
    for (int d = 0; d < D; d++) {
      const PairTerm t = pair_term(metric, h_x[(size_t)i * D + d], metric == kMetricPlda ? h_psi[d] : 1.0);
      y[(size_t)i * D + d] = t.y;
      s_quad += t.quad;
      s_logr += t.logr;
    }
    q[(size_t)i] = pair_q(metric, s_quad, s_logr);
  }
  const double w = pair_weight(metric);
  for (int64_t i = 0; i < N; i++) {
    const int32_t own = sil_cluster_of(h_off, C, i);
    SilRow r = sil_row_init();
    for (int32_t c = 0; c < C; c++) {
      double P[kSilPartials] = {0.0, 0.0, 0.0, 0.0};
      for (int64_t j = h_off[c]; j < h_off[c + 1]; j++) {
        const double s = h_v_in ? h_v_in[(size_t)i * N + j]
                                : pair_score(q[(size_t)i], q[(size_t)j], w, pair_dot(&y[(size_t)i * D], &y[(size_t)j * D], D));
        if (h_v) h_v[(size_t)i * N + j] = s;
        if (j != i) P[sil_partial(j)] += sil_distance(metric, s);
      }
      sil_fold(r, own, c, sil_combine(P[0], P[1], P[2], P[3]), (int64_t)h_off[c + 1] - h_off[c]);
    }
    h_sil[i] = sil_finish((int64_t)h_off[own + 1] - h_off[own], r.a, r.b);
    if (h_a) h_a[i] = r.a;
    if (h_b) h_b[i] = r.b;
    if (h_bj) h_bj[i] = r.bj;
  }
  return 0;
}
