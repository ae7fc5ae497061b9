// The arithmetic of the GMM statistics (gmm_acc.hip), host and device: the contract of include/mfa_hip.h ("GMM
// statistics") operation for operation.  The kernel and the host twin behind mfa_debug_gmm_acc_host (gmm_acc_host.cpp) both
// run exactly these functions, so a Gaussian's log-likelihood has the same bits on either side; what may differ is expf /
// logf themselves, the order in which a frame's exponentials are added, and the order of the double sums.
// Compiled with -ffp-contract=off: every fused operation below is written as one.  Plain C++: no HIP type, so the twin's
// translation unit also builds with a host compiler alone (tests/native/gmm_acc_check.cpp).
#pragma once
#include <math.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_ACC_FN __host__ __device__ inline
#else
#define MFA_ACC_FN inline
#endif

// One Gaussian on one frame: the float32 fmaf chain of fmllr_frame_kernel — from gconst, means_invvars·x over ascending k,
// then (−½·inv_vars)·(x·x) over ascending k.  lin / quad: the Gaussian's two weight rows, element k at [k·stride] (the
// kernel reads them from a [k][Gaussian] LDS tile, the twin from the model's rows).
MFA_ACC_FN float gmm_acc_loglike(float gconst, int dim, const float *lin, int lin_stride, const float *quad, int quad_stride,
                                 const float *x) {
  float acc = gconst;
  for (int k = 0; k < dim; k++) acc = fmaf(lin[k * lin_stride], x[k], acc);
  for (int k = 0; k < dim; k++) {
    const float xv = x[k];
    acc = fmaf(quad[k * quad_stride], xv * xv, acc);
  }
  return acc;
}

// The same chain for F frames at once (x: F rows, x_stride apart): every weight is read once for the F frames.  Each
// frame's chain is the one above, operation for operation — the same bits.
template <int F>
MFA_ACC_FN void gmm_acc_loglike_block(float gconst, int dim, const float *lin, int lin_stride, const float *quad, int quad_stride,
                                      const float *x, int x_stride, float (&out)[F]) {
  for (int f = 0; f < F; f++) out[f] = gconst;
  for (int k = 0; k < dim; k++) {
    const float w = lin[k * lin_stride];
    for (int f = 0; f < F; f++) out[f] = fmaf(w, x[f * x_stride + k], out[f]);
  }
  for (int k = 0; k < dim; k++) {
    const float w = quad[k * quad_stride];
    for (int f = 0; f < F; f++) {
      const float xv = x[f * x_stride + k];
      out[f] = fmaf(w, xv * xv, out[f]);
    }
  }
}

// γ_g = e_g · (1/s) · w, left to right in float32
MFA_ACC_FN float gmm_acc_posterior(float e, float inv_sum, float weight) { return e * inv_sum * weight; }

// the frame's log-likelihood from the maximum and the sum of the shifted exponentials
MFA_ACC_FN float gmm_acc_frame_loglike(float mx, float sum) { return mx + logf(sum); }

// mean += γ·x, var += γ·(x·x): double, the square formed in double (exact: 48 bits), one fma each
MFA_ACC_FN void gmm_acc_add(double gamma, float x, double &mean, double &var) {
  const double xd = (double)x;
  mean = fma(gamma, xd, mean);
  var = fma(gamma, xd * xd, var);
}

// tot[0] += w·loglike (fma), tot[1] += w
MFA_ACC_FN void gmm_acc_total(float weight, float loglike, double &tot_like, double &tot_count) {
  tot_like = fma((double)weight, (double)loglike, tot_like);
  tot_count += (double)weight;
}
