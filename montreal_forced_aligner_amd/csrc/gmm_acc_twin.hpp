// What the host twins of the posterior-weighted statistics (gmm_acc_host.cpp, mllt_acc_host.cpp) share: the check of the
// model's mixture sizes and a frame's log-likelihoods, maximum and shifted exponentials, by gmm_acc_math.hpp's operations in
// ascending Gaussian order, expf from libm.  Plain C++: no HIP type, so the twins build with a host compiler alone.
#pragma once
#include <cstdint>
#include <vector>

#include "gmm_acc_math.hpp"

// The largest mixture of the model; -1 if a pdf has no Gaussian, -2 if one has more than 128 (the twins' return codes).
inline int gmm_acc_twin_max_gauss(int32_t num_pdfs, const int32_t *h_pdf_offsets) {
  int max_gauss = 0;
  for (int p = 0; p < num_pdfs; p++) {
    const int n = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
    if (n <= 0) return -1;
    if (n > 128) return -2;
    if (n > max_gauss) max_gauss = n;
  }
  return max_gauss;
}

struct GmmAccTwinFrame {
  std::vector<float> half, ll, e;     // scratch: −½·inv_vars of a Gaussian, the log-likelihoods; e[g] = expf(ll[g] − mx)
  float mx = 0.0f, sum = 0.0f;        // the largest log-likelihood; Σ e[g], added in ascending g
  GmmAccTwinFrame(int dim, int max_gauss) : half((size_t)dim), ll((size_t)max_gauss), e((size_t)max_gauss) {}

  // One frame x against a pdf's n Gaussians, whose rows of the three model arrays start at the pointers given.
  void fill(int dim, int n, const float *gconsts, const float *means_invvars, const float *inv_vars, const float *x) {
    mx = -INFINITY;
    for (int g = 0; g < n; g++) {
      const float *iv = inv_vars + (size_t)g * dim;
      for (int k = 0; k < dim; k++) half[k] = -0.5f * iv[k];          // the packed model's second row (gmm_pack_rows)
      ll[g] = gmm_acc_loglike(gconsts[g], dim, means_invvars + (size_t)g * dim, 1, half.data(), 1, x);
      mx = fmaxf(mx, ll[g]);
    }
    sum = 0.0f;
    for (int g = 0; g < n; g++) { e[g] = expf(ll[g] - mx); sum += e[g]; }
  }
};
