// Host twin of the GMM statistics (gmm_acc.hip): the whole arithmetic contract of include/mfa_hip.h on host arrays, frames
// in ascending index, expf / logf from libm.  No context, no device, no HIP header: this file, gmm_acc_twin.hpp (a frame's
// exponentials, shared with mllt_acc_host.cpp) and gmm_acc_math.hpp are all tests/native/gmm_acc_check.cpp and
// gmm_acc2_check.cpp need.  One loop serves both forms: the one-feature twin passes its
// matrix twice.
#include <cstdint>

#include "../../include/mfa_hip.h"
#include "gmm_acc_twin.hpp"

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
  const int max_gauss = gmm_acc_twin_max_gauss(num_pdfs, h_pdf_offsets);
  if (max_gauss < 0) return max_gauss;
  if (h_post && post_stride < max_gauss) return -1;
  GmmAccTwinFrame f(dim, max_gauss);
  for (int64_t t = 0; t < total_frames; t++) {
    if (h_post)
      for (int g = 0; g < post_stride; g++) h_post[t * post_stride + g] = 0.0f;
    const int p = h_pdf[t];
    const float w = h_weight[t];
    if (p < 0 || p >= num_pdfs || w == 0.0f) continue;
    const int g0 = h_pdf_offsets[p], n = h_pdf_offsets[p + 1] - g0;
    const float *x = h_feats + t * dim, *xs = h_feats_sum + t * dim;
    f.fill(dim, n, h_gconsts + g0, h_means_invvars + (size_t)g0 * dim, h_inv_vars + (size_t)g0 * dim, x);
    const float inv = 1.0f / f.sum;
    for (int g = 0; g < n; g++) {
      const float post = gmm_acc_posterior(f.e[g], inv, w);
      if (h_post) h_post[t * post_stride + g] = post;
      const double gamma = (double)post;
      h_occ[g0 + g] += gamma;
      double *mean = h_mean + (size_t)(g0 + g) * dim, *var = h_var + (size_t)(g0 + g) * dim;
      for (int k = 0; k < dim; k++) gmm_acc_add(gamma, xs[k], mean[k], var[k]);
    }
    gmm_acc_total(w, gmm_acc_frame_loglike(f.mx, f.sum), h_tot[0], h_tot[1]);
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
