// The arithmetic of the clustering stage (cluster.hip), host and device: the layout of the neighbour bit matrix, the limits
// both sides refuse and the integer rules of DBSCAN on it (include/mfa_hip.h "Clustering").  Plain C++: no HIP type, so the
// twin builds with a host compiler alone (tests/native/cluster_check.cpp).
#pragma once
#include <stdint.h>

#include "gmm_acc_math.hpp"   // MFA_ACC_FN

// Row i of the matrix is W = cluster_words(N) words; bit j & 63 of word j >> 6 is the edge (i, j).
MFA_ACC_FN int64_t cluster_words(int64_t N) { return (N + 63) >> 6; }

// The bits of word w that are columns below N: all of them but in the last word of a row.
MFA_ACC_FN uint64_t cluster_pad_mask(int64_t N, int64_t w) {
  const int64_t left = N - (w << 6);
  return left >= 64 ? ~(uint64_t)0 : (left <= 0 ? (uint64_t)0 : (((uint64_t)1 << left) - 1));
}

// 0 fine, -1 a NULL array (the callers), -2 N outside [0, 2^31), -3 min_samples below 1.
MFA_ACC_FN int cluster_check(int64_t N, int32_t min_samples) {
  if (N < 0 || N >= ((int64_t)1 << 31)) return -2;
  if (min_samples < 1) return -3;
  return 0;
}

// A point is a core point when its row, the point itself included, holds min_samples bits.
MFA_ACC_FN bool cluster_is_core(int32_t count, int32_t min_samples) { return count >= min_samples; }

constexpr int32_t kClusterNoRoot = 0x7fffffff;   // the root of a point that is no core point / has no core neighbour
constexpr int32_t kClusterNoise = -1;            // its label
