// The arithmetic of the i-vector extractor stage (ivector.hip), host and device: the contract of include/mfa_hip.h ("I-vector
// extractor") where both sides must agree to the bit, and the limits both refuse.  The pruning kernel and its host twin
// (ivector_host.cpp) run exactly ivector_prune_frame, so a pruned posterior has the same float32 bits on either side.  Plain
// C++: no HIP type, so the twins build with a host compiler alone (tests/native/ivector_check.cpp).
#pragma once
#include <stdint.h>

#include "ubm_math.hpp"

constexpr int kIvecMaxDim = kUbmMaxDim;       // 48: columns of a staged feature row
constexpr int kIvecMaxGauss = kUbmMaxGauss;   // 2048
constexpr int kIvecMaxSelect = kUbmMaxSelect; // 64 entries of a frame's list
constexpr int kIvecMaxR = 192;                // the packed triangle of Q in one workgroup's LDS: 148 224 B of 160 KiB

// 0 fine, -1 a count that is no count, -2 dim outside [1, 48], -3 G outside [1, 2048], -4 n outside [1, 64], -5 2^31 frames
// or more, -6 R outside [1, 192].  A check that does not apply is passed a value inside its range.
MFA_ACC_FN int ivector_check_shape(int32_t dim, int32_t G, int32_t n, int32_t R, int64_t total_frames, int64_t n_utt) {
  if (total_frames < 0 || n_utt < 0) return -1;
  if (dim <= 0 || dim > kIvecMaxDim) return -2;
  if (G <= 0 || G > kIvecMaxGauss) return -3;
  if (n <= 0 || n > kIvecMaxSelect) return -4;
  if (total_frames >= ((int64_t)1 << 31) || n_utt >= ((int64_t)1 << 31)) return -5;
  if (R <= 0 || R > kIvecMaxR) return -6;
  return 0;
}

// element (r, c), c <= r, of a symmetric matrix stored as its packed lower triangle, row-major
MFA_ACC_FN int ivector_packed(int r, int c) { return r * (r + 1) / 2 + c; }

// One frame of gauss-to-post's pruning, float32, entries in list order.  An entry survives when it is >= min_post (a NaN
// never is).  When none survives, the first of the largest entries does, if it is positive.  The survivors are summed in
// list order, each is divided by the sum and then multiplied by scale; every other entry becomes 0.  A frame whose
// survivors do not sum to a positive number (all zeros: a frame that took no part) becomes all zeros.  in == out is fine:
// the sum is complete before the first store.
MFA_ACC_FN void ivector_prune_frame(const float *in, float *out, int n, float min_post, float scale) {
  int kept = 0, best = 0;
  float sum = 0.0f;
  for (int j = 0; j < n; j++) {
    const float p = in[j];
    if (p >= min_post) { sum += p; kept++; }
    if (p > in[best] || !(in[best] == in[best])) best = j;   // first of the largest; steps off a leading NaN
  }
  if (kept == 0 && in[best] > 0.0f) sum = in[best];
  const bool alive = sum > 0.0f;
  const float lone = in[best];
  for (int j = 0; j < n; j++) {
    const float p = in[j];
    const bool keep = alive && (kept > 0 ? p >= min_post : (j == best && lone > 0.0f));
    out[j] = keep ? p / sum * scale : 0.0f;
  }
}
