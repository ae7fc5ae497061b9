// Host twins of the diagonal-UBM stage (ubm.hip): Gaussian selection and the global statistics over the selected Gaussians,
// the contract of include/mfa_hip.h ("Diagonal UBM") on host arrays, frames in ascending index, expf / logf from libm.  No
// context, no device, no HIP header: this file, ubm_math.hpp and gmm_acc_math.hpp are all tests/native/ubm_check.cpp needs.
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/mfa_hip.h"
#include "ubm_math.hpp"

namespace {

// −½·inv_vars of every Gaussian: the second row of the log-likelihood chain
std::vector<float> half_inv_vars(int32_t dim, int32_t G, const float *h_inv_vars) {
  std::vector<float> half((size_t)G * dim);
  for (size_t i = 0; i < half.size(); i++) half[i] = ubm_half_inv_var(h_inv_vars[i]);
  return half;
}

}  // namespace

extern "C" MFA_API int mfa_debug_ubm_gselect_host(const float *h_feats, int64_t total_frames, int32_t dim, int32_t G,
                                                  const float *h_gconsts, const float *h_means_invvars, const float *h_inv_vars,
                                                  int32_t num_gselect, int32_t *h_gselect, float *h_loglike) {
  const int rc = ubm_check_shape(dim, G, total_frames);
  if (rc) return rc;
  if (num_gselect <= 0 || std::min(num_gselect, G) > kUbmMaxSelect) return -4;
  if (total_frames == 0) return 0;
  if (!h_feats || !h_gconsts || !h_means_invvars || !h_inv_vars || !h_gselect) return -1;
  const int n = std::min(num_gselect, G);
  const std::vector<float> half = half_inv_vars(dim, G, h_inv_vars);
  std::vector<uint64_t> key((size_t)G);
  for (int64_t t = 0; t < total_frames; t++) {
    const float *x = h_feats + t * dim;
    for (int g = 0; g < G; g++)
      key[g] = ubm_key(gmm_acc_loglike(h_gconsts[g], dim, h_means_invvars + (size_t)g * dim, 1, half.data() + (size_t)g * dim, 1, x), g);
    std::partial_sort(key.begin(), key.begin() + n, key.end(), std::greater<uint64_t>());
    for (int j = 0; j < n; j++) h_gselect[t * n + j] = ubm_key_index(key[j]);
    if (h_loglike) {
      const float mx = ubm_key_loglike(key[0]);
      float sum = 0.0f;
      for (int j = 0; j < n; j++) sum += expf(ubm_key_loglike(key[j]) - mx);
      h_loglike[t] = gmm_acc_frame_loglike(mx, sum);
    }
  }
  return 0;
}

extern "C" MFA_API int mfa_debug_ubm_acc_host(const float *h_feats, int64_t total_frames, int32_t dim, int32_t G,
                                              const float *h_gconsts, const float *h_means_invvars, const float *h_inv_vars,
                                              int32_t n, const int32_t *h_gselect, const float *h_frame_weight, double *h_occ,
                                              double *h_mean, double *h_var, double *h_tot, float *h_post) {
  const int rc = ubm_check_shape(dim, G, total_frames);
  if (rc) return rc;
  if (h_gselect && (n <= 0 || n > kUbmMaxSelect)) return -4;
  if (h_post && !h_gselect) return -1;
  if (total_frames == 0) return 0;
  if (!h_feats || !h_gconsts || !h_means_invvars || !h_inv_vars || !h_occ || !h_mean || !h_var || !h_tot) return -1;
  const int len = h_gselect ? n : G;
  const std::vector<float> half = half_inv_vars(dim, G, h_inv_vars);
  std::vector<float> ll((size_t)len), e((size_t)len);
  std::vector<int> idx((size_t)len);
  for (int64_t t = 0; t < total_frames; t++) {
    const float *x = h_feats + t * dim;
    const float w = h_frame_weight ? h_frame_weight[t] : 1.0f;
    if (h_post)
      for (int j = 0; j < n; j++) h_post[t * n + j] = 0.0f;
    bool any = false;
    float mx = -INFINITY;
    for (int j = 0; j < len; j++) {
      const int g = h_gselect ? h_gselect[t * n + j] : j;
      idx[j] = g >= 0 && g < G ? g : -1;
      if (idx[j] < 0) continue;
      any = true;
      ll[j] = gmm_acc_loglike(h_gconsts[g], dim, h_means_invvars + (size_t)g * dim, 1, half.data() + (size_t)g * dim, 1, x);
      mx = fmaxf(mx, ll[j]);
    }
    if (!any || w == 0.0f) continue;
    float sum = 0.0f;
    for (int j = 0; j < len; j++)
      if (idx[j] >= 0) { e[j] = expf(ll[j] - mx); sum += e[j]; }
    const float inv = 1.0f / sum;
    for (int j = 0; j < len; j++) {
      if (idx[j] < 0) continue;
      const int g = idx[j];
      const float post = gmm_acc_posterior(e[j], inv, w);
      if (h_post) h_post[t * n + j] = post;
      const double gamma = (double)post;
      h_occ[g] += gamma;
      double *mean = h_mean + (size_t)g * dim, *var = h_var + (size_t)g * dim;
      for (int k = 0; k < dim; k++) gmm_acc_add(gamma, x[k], mean[k], var[k]);
    }
    gmm_acc_total(w, gmm_acc_frame_loglike(mx, sum), h_tot[0], h_tot[1]);
  }
  return 0;
}
