// Host twin of the clustering stage (cluster.hip): DBSCAN on a neighbour bit matrix, the contract of include/mfa_hip.h
// ("Clustering") on host arrays.  The answer is unique, so the twin is free in its method: it symmetrises bit by bit, walks
// the core points' components depth first from the lowest unvisited core index, and numbers them in that order.  No context,
// no device, no HIP header: this file and cluster_math.hpp (with the header it includes) are all
// tests/native/cluster_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "cluster_math.hpp"

extern "C" MFA_API int mfa_debug_dbscan_from_bits_host(uint64_t *h_bits, int64_t N, int32_t min_samples, int32_t *h_labels, int32_t *h_core,
                                                       int32_t *h_count, int32_t *h_n_clusters) {
  const int rc = cluster_check(N, min_samples);
  if (rc) return rc;
  if (!h_n_clusters) return -1;
  *h_n_clusters = 0;
  if (N == 0) return 0;
  if (!h_bits || !h_labels || !h_core || !h_count) return -1;
  const int64_t W = cluster_words(N);
  auto get = [&](int64_t i, int64_t j) { return (h_bits[(size_t)i * W + (j >> 6)] >> (j & 63)) & 1; };
  auto set = [&](int64_t i, int64_t j) { h_bits[(size_t)i * W + (j >> 6)] |= (uint64_t)1 << (j & 63); };
  for (int64_t i = 0; i < N; i++) {                  // padding off, the diagonal on, an edge in either direction an edge
    h_bits[(size_t)i * W + (W - 1)] &= cluster_pad_mask(N, W - 1);
    set(i, i);
  }
  for (int64_t i = 0; i < N; i++)
    for (int64_t j = i + 1; j < N; j++)
      if (get(i, j) | get(j, i)) { set(i, j); set(j, i); }
  for (int64_t i = 0; i < N; i++) {
    int32_t n = 0;
    for (int64_t w = 0; w < W; w++) n += __builtin_popcountll(h_bits[(size_t)i * W + w]);
    h_count[i] = n;
    h_core[i] = cluster_is_core(n, min_samples) ? 1 : 0;
    h_labels[i] = kClusterNoise;
  }
  int32_t next = 0;
  std::vector<int64_t> stack;
  for (int64_t s = 0; s < N; s++) {                  // a cluster starts at the lowest core index not yet in one
    if (!h_core[s] || h_labels[s] != kClusterNoise) continue;
    h_labels[s] = next;
    stack.push_back(s);
    while (!stack.empty()) {
      const int64_t i = stack.back();
      stack.pop_back();
      for (int64_t j = 0; j < N; j++)
        if (h_core[j] && h_labels[j] == kClusterNoise && get(i, j)) { h_labels[j] = next; stack.push_back(j); }
    }
    next++;
  }
  for (int64_t i = 0; i < N; i++) {                  // a border point: the smallest number among its core neighbours
    if (h_core[i]) continue;
    int32_t best = kClusterNoRoot;
    for (int64_t j = 0; j < N; j++)
      if (h_core[j] && get(i, j) && h_labels[j] < best) best = h_labels[j];
    h_labels[i] = best == kClusterNoRoot ? kClusterNoise : best;
  }
  *h_n_clusters = next;
  return 0;
}
