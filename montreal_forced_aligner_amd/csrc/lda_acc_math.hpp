// The arithmetic of the LDA statistics (lda_acc.hip), host and device: the contract of include/mfa_hip.h ("LDA
// statistics") operation for operation.  The kernel and the host twin behind mfa_debug_lda_acc_host (lda_acc_host.cpp) both
// run exactly these functions, so a spliced vector, a frame's weight and the prune decision have the same bits on either
// side; what may differ is the order of the double sums and whether a second-moment term is rounded once (an fma on the
// f64 matrix pipe) or twice.  Compiled with -ffp-contract=off: every fused operation below is written as one.  Plain C++: no
// HIP type, so the twin's translation unit also builds with a host compiler alone (tests/native/lda_acc_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "align_equal_math.hpp"   // mfa_ae_random: the counter-based stream of the prune draws

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_LDA_FN __host__ __device__ inline
#else
#define MFA_LDA_FN inline
#endif

constexpr int kLdaMaxSpliced = 128;   // S = (2·ctx + 1)·dim at most (mfa_lda_acc_max_dim)

// What ApplyCmvn subtracts from column d of a speaker's rows: (float)(sum / count) of its statistics [2][dim + 1].
MFA_LDA_FN float lda_cmvn_offset(const double *spk_stats, int dim, int d) { return (float)(spk_stats[d] / spk_stats[dim]); }

// One CMVN-applied value: float32, the bits of feats.hip (v + (float)(-mean) = v - (float)mean).
MFA_LDA_FN float lda_cmvn_apply(float v, float offset) { return v - offset; }

// Row of the batch that element i of the spliced vector of frame t (of the utterance [f0, f1)) reads, and its column:
// offsets ascend from -ctx, columns within an offset; frames outside the utterance are its first / last.
MFA_LDA_FN int64_t lda_splice_row(int64_t t, int i, int dim, int ctx, int64_t f0, int64_t f1, int *col) {
  const int o = i / dim;
  *col = i - o * dim;
  int64_t r = t + o - ctx;
  return r < f0 ? f0 : (r >= f1 ? f1 - 1 : r);
}

// A frame's weight after the random prune (Kaldi RandPrune on a counter-based generator): |w| >= theta or theta <= 0
// leaves it; otherwise it becomes copysign(theta, w) with probability |w| / theta and 0 (the frame takes no part) else.
// draw: the frame's index inside its utterance.
MFA_LDA_FN float lda_prune_weight(float w, float theta, uint32_t seed, uint32_t key, uint32_t draw) {
  if (!(theta > 0.0f) || w == 0.0f || !(fabsf(w) < theta)) return w;
  const float r = fabsf(w) / theta;
  const uint32_t u = mfa_ae_random(seed, key, draw);
  return (float)(u >> 8) * 5.9604644775390625e-08f < r ? copysignf(theta, w) : 0.0f;     // 2^-24
}

// The frame's class and weight from its transition-id: returns false when the frame takes no part (before the prune).
MFA_LDA_FN bool lda_frame_class(int32_t tid, const int32_t *tid2class, const float *tid_weight, int32_t n_tids, int32_t n_classes,
                                int32_t *cls, float *w) {
  if (tid <= 0 || tid >= n_tids) return false;
  const int32_t c = tid2class[tid];
  const float wt = tid_weight[tid];
  if (wt == 0.0f || c < 0 || c >= n_classes) return false;
  *cls = c; *w = wt;
  return true;
}

// zero += w; first_i = fma(w, x_i, first_i): double
MFA_LDA_FN void lda_first_add(double w, float x, double &first) { first = fma(w, (double)x, first); }

// second_ij += (w·x_i)·x_j: the first product is exact in double (24 + 24 bits); multiply, then add
MFA_LDA_FN void lda_second_add(double wxi, float xj, double &second) { second += wxi * (double)xj; }
