// Host twins of the i-vector extractor stage (ivector.hip): posterior pruning, the utterance statistics and the E-step, the
// contracts of include/mfa_hip.h ("I-vector extractor") on host arrays, in plain loops, utterances ascending.  No context, no
// device, no HIP header: this file and ivector_math.hpp (with the headers it includes) are all tests/native/ivector_check.cpp
// needs.  The algorithm is restated from its description; Kaldi's source is not among this project's references.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "ivector_math.hpp"

extern "C" MFA_API int mfa_debug_ivector_prune_post_host(const float *h_post, int64_t total_frames, int32_t n, float min_post,
                                                         float scale, float *h_out) {
  const int rc = ivector_check_shape(1, 1, n, 1, total_frames, 0);
  if (rc) return rc;
  if (total_frames == 0) return 0;
  if (!h_post || !h_out) return -1;
  for (int64_t t = 0; t < total_frames; t++) ivector_prune_frame(h_post + t * n, h_out + t * n, n, min_post, scale);
  return 0;
}

extern "C" MFA_API int mfa_debug_ivector_utt_stats_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                                        int32_t G, int32_t n, const int32_t *h_gselect, const float *h_post,
                                                        double max_count, double *h_gamma, double *h_X, double *h_S) {
  if (n_utt < 0) return -1;
  if (n_utt > 0 && !h_frame_off) return -1;
  const int64_t total = n_utt > 0 ? h_frame_off[n_utt] : 0;
  const int rc = ivector_check_shape(dim, G, n, 1, total, n_utt);
  if (rc) return rc;
  if (n_utt == 0) return 0;
  if (!h_gamma || !h_X) return -1;
  if (total > 0 && (!h_feats || !h_gselect || !h_post)) return -1;
  if (h_frame_off[0] != 0) return -1;
  for (int u = 0; u < n_utt; u++)
    if (h_frame_off[u + 1] < h_frame_off[u]) return -1;
  std::vector<double> x((size_t)dim);
  for (int u = 0; u < n_utt; u++) {
    double *gamma = h_gamma + (size_t)u * G, *X = h_X + (size_t)u * G * dim;
    for (int g = 0; g < G; g++) gamma[g] = 0.0;
    for (size_t i = 0; i < (size_t)G * dim; i++) X[i] = 0.0;
    for (int64_t t = h_frame_off[u]; t < h_frame_off[u + 1]; t++) {
      for (int k = 0; k < dim; k++) {
        const float v = h_feats[t * dim + k];
        x[k] = std::isfinite(v) ? (double)v : 0.0;
      }
      for (int j = 0; j < n; j++) {
        const int g = h_gselect[t * n + j];
        if (g < 0 || g >= G) continue;
        const double p = (double)h_post[t * n + j];
        if (p == 0.0) continue;
        gamma[g] += p;
        for (int k = 0; k < dim; k++) X[(size_t)g * dim + k] += p * x[k];
        if (h_S) {
          double *S = h_S + (size_t)g * (dim * (dim + 1) / 2);
          for (int a = 0; a < dim; a++)
            for (int b = 0; b <= a; b++) S[ivector_packed(a, b)] += p * (x[a] * x[b]);
        }
      }
    }
    if (max_count > 0.0) {
      double tot = 0.0;
      for (int g = 0; g < G; g++) tot += gamma[g];
      if (tot > max_count) {
        const double s = max_count / tot;
        for (int g = 0; g < G; g++) gamma[g] *= s;
        for (size_t i = 0; i < (size_t)G * dim; i++) X[i] *= s;
      }
    }
  }
  return 0;
}

extern "C" MFA_API int mfa_debug_ivector_estep_host(const double *h_gamma, const double *h_X, int32_t n_utt, int32_t dim, int32_t G,
                                                    int32_t R, const double *h_W, const double *h_U, double prior_offset,
                                                    double *h_ivec_mean, double *h_ivec_var, double *h_aux, double *h_Gamma,
                                                    double *h_Y, double *h_Rq, double *h_isum, double *h_iscat, double *h_n) {
  const int rc = ivector_check_shape(dim, G, 1, R, 0, n_utt);
  if (rc) return rc;
  const int acc = (h_Gamma != nullptr) + (h_Y != nullptr) + (h_Rq != nullptr) + (h_isum != nullptr) + (h_iscat != nullptr) + (h_n != nullptr);
  if (acc != 0 && acc != 6) return -1;
  if (n_utt == 0) return 0;
  if (!h_gamma || !h_X || !h_W || !h_U || !h_ivec_mean) return -1;
  const int P = R * (R + 1) / 2;
  const size_t GD = (size_t)G * dim;
  std::vector<double> L((size_t)P), var((size_t)P), lin((size_t)R), y((size_t)R), mu((size_t)R), col((size_t)R);
  for (int u = 0; u < n_utt; u++) {
    const double *gamma = h_gamma + (size_t)u * G, *X = h_X + (size_t)u * GD;
    bool any = false;
    for (int g = 0; g < G; g++) any = any || gamma[g] != 0.0;
    // Q = I + sum_g gamma_g U_g, lin = prior_offset e0 + sum_(g,d) X_gd W_gd: the prior term first, then g ascending
    for (int r = 0; r < R; r++)
      for (int c = 0; c <= r; c++) L[ivector_packed(r, c)] = r == c ? 1.0 : 0.0;
    for (int g = 0; g < G; g++)
      for (int e = 0; e < P; e++) L[e] += gamma[g] * h_U[(size_t)g * P + e];
    for (int r = 0; r < R; r++) lin[r] = r == 0 ? prior_offset : 0.0;
    for (size_t k = 0; k < GD; k++)
      for (int r = 0; r < R; r++) lin[r] += X[k] * h_W[k * R + r];
    // Cholesky Q = L L^T, left-looking, k ascending
    for (int j = 0; j < R; j++) {
      for (int i = j; i < R; i++) {
        double s = L[ivector_packed(i, j)];
        for (int k = 0; k < j; k++) s -= L[ivector_packed(i, k)] * L[ivector_packed(j, k)];
        col[i] = s;
      }
      const double d = std::sqrt(col[j]);
      L[ivector_packed(j, j)] = d;
      for (int i = j + 1; i < R; i++) L[ivector_packed(i, j)] = col[i] / d;
    }
    double logdet = 0.0;
    for (int j = 0; j < R; j++) logdet += std::log(L[ivector_packed(j, j)]);
    logdet *= 2.0;
    // L^-1 in place, columns from the last: Linv[i][j] = -(sum_(k = j+1..i) Linv[i][k] L[k][j]) / L[j][j]
    for (int j = R - 1; j >= 0; j--) {
      const double d = L[ivector_packed(j, j)];
      for (int i = j + 1; i < R; i++) col[i] = L[ivector_packed(i, j)];
      for (int i = j + 1; i < R; i++) {
        double s = 0.0;
        for (int k = j + 1; k <= i; k++) s += L[ivector_packed(i, k)] * col[k];
        L[ivector_packed(i, j)] = -(s / d);
      }
      L[ivector_packed(j, j)] = 1.0 / d;
    }
    // mu = Linv^T (Linv lin), Var = Linv^T Linv
    for (int i = 0; i < R; i++) {
      double s = 0.0;
      for (int k = 0; k <= i; k++) s += L[ivector_packed(i, k)] * lin[k];
      y[i] = s;
    }
    bool finite = true;
    double quad = 0.0;
    for (int r = 0; r < R; r++) {
      double s = 0.0;
      for (int k = r; k < R; k++) s += L[ivector_packed(k, r)] * y[k];
      mu[r] = s;
      finite = finite && std::isfinite(s);
      h_ivec_mean[(size_t)u * R + r] = s;
    }
    for (int r = 0; r < R; r++) quad += lin[r] * mu[r];
    if (h_aux) { h_aux[2 * (size_t)u] = quad; h_aux[2 * (size_t)u + 1] = logdet; }
    if (!h_ivec_var && !acc) continue;
    for (int r = 0; r < R; r++)
      for (int c = 0; c <= r; c++) {
        double s = 0.0;
        for (int k = r; k < R; k++) s += L[ivector_packed(k, r)] * L[ivector_packed(k, c)];
        var[ivector_packed(r, c)] = s;
      }
    if (h_ivec_var)
      for (int e = 0; e < P; e++) h_ivec_var[(size_t)u * P + e] = var[e];
    if (!acc || !any || !finite) continue;
    for (int r = 0; r < R; r++)
      for (int c = 0; c <= r; c++) var[ivector_packed(r, c)] += mu[r] * mu[c];   // Sc
    for (int g = 0; g < G; g++) {
      h_Gamma[g] += gamma[g];
      if (gamma[g] != 0.0)
        for (int e = 0; e < P; e++) h_Rq[(size_t)g * P + e] += gamma[g] * var[e];
    }
    for (size_t k = 0; k < GD; k++)
      if (X[k] != 0.0)
        for (int r = 0; r < R; r++) h_Y[k * R + r] += X[k] * mu[r];
    for (int r = 0; r < R; r++) h_isum[r] += mu[r];
    for (int e = 0; e < P; e++) h_iscat[e] += var[e];
    h_n[0] += 1.0;
  }
  return 0;
}
