// Host twin of the MLLT statistics (mllt_acc.hip): the whole arithmetic contract of include/mfa_hip.h on host arrays, frames
// in ascending index, expf / logf from libm, plain loops.  No context, no device, no HIP header: this file, mllt_acc_math.hpp,
// gmm_acc_twin.hpp (a frame's exponentials, shared with gmm_acc_host.cpp) and gmm_acc_math.hpp are all
// tests/native/mllt_acc_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "gmm_acc_twin.hpp"
#include "mllt_acc_math.hpp"

extern "C" MFA_API int mfa_debug_mllt_acc_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                                               const float *h_means_invvars, const float *h_inv_vars, const float *h_means,
                                               const float *h_feats, int64_t total_frames, const int32_t *h_pdf,
                                               const float *h_weight, double *h_occ, double *h_full, double *h_tot, float *h_post,
                                               int32_t post_stride) {
  if (dim <= 0 || num_pdfs <= 0 || total_frames < 0 || !h_pdf_offsets || !h_gconsts || !h_means_invvars || !h_inv_vars || !h_means)
    return -1;
  if (total_frames > 0 && (!h_feats || !h_pdf || !h_weight)) return -1;
  if (!h_occ || !h_full || !h_tot) return -1;
  if (dim > 48) return -3;
  const int max_gauss = gmm_acc_twin_max_gauss(num_pdfs, h_pdf_offsets);
  if (max_gauss < 0) return max_gauss;
  if (h_post && post_stride < max_gauss) return -1;
  const size_t DD = (size_t)dim * dim;
  GmmAccTwinFrame f(dim, max_gauss);
  std::vector<float> d((size_t)dim);
  std::vector<char> touched((size_t)num_pdfs, 0);
  for (int64_t t = 0; t < total_frames; t++) {
    if (h_post)
      for (int g = 0; g < post_stride; g++) h_post[t * post_stride + g] = 0.0f;
    const int p = h_pdf[t];
    const float w = h_weight[t];
    if (p < 0 || p >= num_pdfs || w == 0.0f) continue;
    touched[p] = 1;
    const int g0 = h_pdf_offsets[p], n = h_pdf_offsets[p + 1] - g0;
    const float *x = h_feats + t * dim;
    f.fill(dim, n, h_gconsts + g0, h_means_invvars + (size_t)g0 * dim, h_inv_vars + (size_t)g0 * dim, x);
    const float inv = 1.0f / f.sum;
    for (int g = 0; g < n; g++) {
      const float post = gmm_acc_posterior(f.e[g], inv, w);
      if (h_post) h_post[t * post_stride + g] = post;
      const double gamma = (double)post;
      h_occ[g0 + g] += gamma;
      const float *mu = h_means + (size_t)(g0 + g) * dim;
      for (int k = 0; k < dim; k++) d[k] = mllt_acc_diff(x[k], mu[k]);
      double *full = h_full + (size_t)(g0 + g) * DD;
      for (int i = 0; i < dim; i++) {
        const double gdi = mllt_acc_left(gamma, d[i]);
        for (int j = 0; j <= i; j++) mllt_acc_add(gdi, d[j], full[(size_t)i * dim + j]);
      }
    }
    gmm_acc_total(w, gmm_acc_frame_loglike(f.mx, f.sum), h_tot[0], h_tot[1]);
  }
  // the upper triangle is a copy of the lower, for the Gaussians of every pdf a frame was added to
  for (int p = 0; p < num_pdfs; p++) {
    if (!touched[p]) continue;
    for (int g = h_pdf_offsets[p]; g < h_pdf_offsets[p + 1]; g++) {
      double *full = h_full + (size_t)g * DD;
      for (int i = 0; i < dim; i++)
        for (int j = 0; j < i; j++) full[(size_t)j * dim + i] = full[(size_t)i * dim + j];
    }
  }
  return 0;
}
