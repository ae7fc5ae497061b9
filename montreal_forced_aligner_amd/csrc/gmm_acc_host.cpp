// Host twin of the GMM statistics (gmm_acc.hip): the whole arithmetic contract of include/mfa_hip.h on host arrays, frames
// in ascending index, expf / logf from libm.  No context, no device, no HIP header: this file and gmm_acc_math.hpp are all
// tests/native/gmm_acc_check.cpp and gmm_acc2_check.cpp need.  One loop serves both forms: the one-feature twin passes its
// matrix twice.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "gmm_acc_math.hpp"

// h_feats: the rows of the log-likelihood chain and the softmax; h_feats_sum: the rows the sums are formed from (the same
// pointer in the one-feature form).
static int gmm_acc_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                        const float *h_means_invvars, const float *h_inv_vars, const float *h_feats, const float *h_feats_sum,
                        int64_t total_frames, const int32_t *h_pdf, const float *h_weight, const int32_t *h_tid, int32_t n_tids,
                        double *h_occ, double *h_mean, double *h_var, double *h_tot, int64_t *h_tid_count, float *h_post,
                        int32_t post_stride) {
  if (dim <= 0 || num_pdfs <= 0 || total_frames < 0 || !h_pdf_offsets || !h_gconsts || !h_means_invvars || !h_inv_vars) return -1;
  if (total_frames > 0 && (!h_feats || !h_feats_sum || !h_pdf || !h_weight)) return -1;
  if (!h_occ || !h_mean || !h_var || !h_tot) return -1;
  int max_gauss = 0;
  for (int p = 0; p < num_pdfs; p++) {
    const int n = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
    if (n <= 0) return -1;
    if (n > 128) return -2;
    if (n > max_gauss) max_gauss = n;
  }
  if (h_post && post_stride < max_gauss) return -1;
  std::vector<float> half((size_t)dim), ll((size_t)max_gauss), e((size_t)max_gauss);
  for (int64_t t = 0; t < total_frames; t++) {
    if (h_post)
      for (int g = 0; g < post_stride; g++) h_post[t * post_stride + g] = 0.0f;
    const int p = h_pdf[t];
    const float w = h_weight[t];
    if (p < 0 || p >= num_pdfs || w == 0.0f) continue;
    const int g0 = h_pdf_offsets[p], n = h_pdf_offsets[p + 1] - g0;
    const float *x = h_feats + t * dim, *xs = h_feats_sum + t * dim;
    float mx = -INFINITY;
    for (int g = 0; g < n; g++) {
      const float *iv = h_inv_vars + (size_t)(g0 + g) * dim;
      for (int k = 0; k < dim; k++) half[k] = -0.5f * iv[k];          // the packed model's second row (gmm_pack_rows)
      ll[g] = gmm_acc_loglike(h_gconsts[g0 + g], dim, h_means_invvars + (size_t)(g0 + g) * dim, 1, half.data(), 1, x);
      mx = fmaxf(mx, ll[g]);
    }
    float sum = 0.0f;
    for (int g = 0; g < n; g++) { e[g] = expf(ll[g] - mx); sum += e[g]; }
    const float inv = 1.0f / sum;
    for (int g = 0; g < n; g++) {
      const float post = gmm_acc_posterior(e[g], inv, w);
      if (h_post) h_post[t * post_stride + g] = post;
      const double gamma = (double)post;
      h_occ[g0 + g] += gamma;
      double *mean = h_mean + (size_t)(g0 + g) * dim, *var = h_var + (size_t)(g0 + g) * dim;
      for (int k = 0; k < dim; k++) gmm_acc_add(gamma, xs[k], mean[k], var[k]);
    }
    gmm_acc_total(w, gmm_acc_frame_loglike(mx, sum), h_tot[0], h_tot[1]);
    if (h_tid && h_tid_count && h_tid[t] > 0 && h_tid[t] < n_tids) h_tid_count[h_tid[t]] += 1;
  }
  return 0;
}

extern "C" MFA_API int mfa_debug_gmm_acc_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                                              const float *h_means_invvars, const float *h_inv_vars, const float *h_feats,
                                              int64_t total_frames, const int32_t *h_pdf, const float *h_weight,
                                              const int32_t *h_tid, int32_t n_tids, double *h_occ, double *h_mean, double *h_var,
                                              double *h_tot, int64_t *h_tid_count, float *h_post, int32_t post_stride) {
  return gmm_acc_host(dim, num_pdfs, h_pdf_offsets, h_gconsts, h_means_invvars, h_inv_vars, h_feats, h_feats, total_frames, h_pdf,
                      h_weight, h_tid, n_tids, h_occ, h_mean, h_var, h_tot, h_tid_count, h_post, post_stride);
}

extern "C" MFA_API int mfa_debug_gmm_acc_twofeats_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets,
                                                       const float *h_gconsts, const float *h_means_invvars, const float *h_inv_vars,
                                                       const float *h_feats, const float *h_feats_sum, int64_t total_frames,
                                                       const int32_t *h_pdf, const float *h_weight, const int32_t *h_tid,
                                                       int32_t n_tids, double *h_occ, double *h_mean, double *h_var, double *h_tot,
                                                       int64_t *h_tid_count, float *h_post, int32_t post_stride) {
  return gmm_acc_host(dim, num_pdfs, h_pdf_offsets, h_gconsts, h_means_invvars, h_inv_vars, h_feats, h_feats_sum, total_frames,
                      h_pdf, h_weight, h_tid, n_tids, h_occ, h_mean, h_var, h_tot, h_tid_count, h_post, post_stride);
}
