// The arithmetic of the diagonal-UBM stage (ubm.hip), host and device: the contract of include/mfa_hip.h ("Diagonal UBM")
// beyond what gmm_acc_math.hpp already fixes.  The kernels and the host twins (ubm_host.cpp) run exactly these functions and
// gmm_acc_math.hpp's, so a Gaussian's log-likelihood, its selection key and therefore the selected indices and their order
// have the same bits on either side.  Plain C++: no HIP type, so the twins build with a host compiler alone
// (tests/native/ubm_check.cpp).
#pragma once
#include <stdint.h>

#include "gmm_acc_math.hpp"

constexpr int kUbmMaxDim = 48;       // columns of a staged row (the GMM statistics' limit)
constexpr int kUbmMaxGauss = 2048;   // 32 rounds of lane = Gaussian
constexpr int kUbmMaxSelect = 64;    // a frame's best list is one wavefront register: lane j holds the j-th best

// The limits both sides refuse, in the order of the twins' return codes: 0 fine, -1 a count that is no count, -2 dim > 48,
// -3 G outside [1, 2048], -5 2^31 frames or more.  (-4 is the list length: it differs between the two calls.)
MFA_ACC_FN int ubm_check_shape(int32_t dim, int32_t G, int64_t total_frames) {
  if (dim <= 0 || total_frames < 0) return -1;
  if (dim > kUbmMaxDim) return -2;
  if (G <= 0 || G > kUbmMaxGauss) return -3;
  if (total_frames >= ((int64_t)1 << 31)) return -5;
  return 0;
}

// The selection key of Gaussian g with log-likelihood ll: the order-preserving uint32 image of the float's bits in the high
// word, g + 1 in the low word.  Keys compare as (log-likelihood, index) pairs: at equal log-likelihood the larger index is
// the larger key.  Every bit pattern has a key, a NaN's included (above +inf with the sign bit clear, below -inf with it
// set), and keys of different g differ: whatever the features are, a frame's best keys name distinct Gaussians.  0 is no
// key: an empty list entry.
MFA_ACC_FN uint64_t ubm_key(float ll, int g) {
  uint32_t b;
  __builtin_memcpy(&b, &ll, 4);
  const uint32_t u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)u << 32) | (uint32_t)(g + 1);
}

MFA_ACC_FN int ubm_key_index(uint64_t key) { return (int)(uint32_t)key - 1; }

MFA_ACC_FN float ubm_key_loglike(uint64_t key) {
  const uint32_t u = (uint32_t)(key >> 32);
  const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
  float ll;
  __builtin_memcpy(&ll, &b, 4);
  return ll;
}

// the packed model's second weight row of a Gaussian (gmm_pack_rows): exact, a scaling by a power of two
MFA_ACC_FN float ubm_half_inv_var(float inv_var) { return -0.5f * inv_var; }
