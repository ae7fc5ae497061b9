// The host twins of the neighbour sweep (csrc/plda_host.cpp) and of DBSCAN on its bit matrix (csrc/cluster_host.cpp) as a
// stand-alone program for the host sanitizers: tests/test_cluster_cpu.py builds it with -fsanitize=address,undefined and runs it
// once.  Every array is sized exactly, so an index past an end is a report.  Inputs: point counts around the word size (1, 63,
// 64, 65, 129), rectangular shapes, the three metrics, NaN vectors, thresholds at the infinities, random words with stray
// padding bits, no points, the refusals.  What the results must satisfy is checked from the definitions.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/mfa_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double small_int(uint32_t &s) { return (double)((int)(lcg(s) >> 28) - 8); }   // -8 .. 7

static bool bit(const std::vector<uint64_t> &b, size_t W, size_t i, size_t j) { return (b[i * W + (j >> 6)] >> (j & 63)) & 1; }

static void neighbour_bits(int nt, int ns, int D, int metric, double thr, bool poison) {
  uint32_t s = 5u + (uint32_t)nt * 31u + (uint32_t)ns * 7u + (uint32_t)metric;
  std::vector<double> test((size_t)nt * D), train((size_t)ns * D), psi((size_t)D), scores((size_t)nt * ns);
  for (auto &v : test) v = small_int(s);
  for (auto &v : train) v = small_int(s);
  for (auto &v : psi) v = 0.5 + (double)(lcg(s) >> 30);
  if (poison && nt > 1 && ns > 1) {
    test[(size_t)D] = std::numeric_limits<double>::quiet_NaN();       // row 1
    train[(size_t)D] = std::numeric_limits<double>::quiet_NaN();      // column 1
  }
  const size_t W = (size_t)(ns + 63) / 64;
  std::vector<uint64_t> bits((size_t)nt * W, ~(uint64_t)0);
  const int rc = mfa_debug_neighbor_bits_host(test.data(), nt, train.empty() ? nullptr : train.data(), ns, D, metric, nullptr, psi.data(), 0, 1,
                                              thr, scores.empty() ? nullptr : scores.data(), nullptr, nullptr, nullptr, nullptr,
                                              bits.empty() ? nullptr : bits.data());
  CHECK(rc == 0);
  for (int i = 0; i < nt; i++) {
    for (size_t j = 0; j < W * 64; j++) {
      const bool want = j < (size_t)ns && scores[(size_t)i * ns + j] >= thr;
      CHECK(bit(bits, W, (size_t)i, j) == want);
    }
    if (poison && nt > 1 && ns > 1 && i == 1)
      for (size_t w = 0; w < W; w++) CHECK(bits[(size_t)i * W + w] == 0);
    if (poison && nt > 1 && ns > 1) CHECK(!bit(bits, W, (size_t)i, 1));
  }
  if (metric == 1)                                   // exact on these integers: -|p - g|^2
    for (int i = 0; i < nt && !poison; i++)
      for (int j = 0; j < ns; j++) {
        double d = 0.0;
        for (int k = 0; k < D; k++) d += (test[(size_t)i * D + k] - train[(size_t)j * D + k]) * (test[(size_t)i * D + k] - train[(size_t)j * D + k]);
        CHECK(scores[(size_t)i * ns + j] == -d);
      }
}

static void dbscan(int N, int min_samples, uint32_t seed, int density_shift) {
  const size_t W = (size_t)(N + 63) / 64;
  std::vector<uint64_t> bits((size_t)N * W), in;
  uint32_t s = seed;
  for (auto &w : bits) {                             // sparse random words, padding bits among them
    uint64_t v = ~(uint64_t)0;
    for (int r = 0; r < density_shift; r++) v &= ((uint64_t)lcg(s) << 32) | lcg(s);
    w = v;
  }
  in = bits;
  std::vector<int32_t> labels((size_t)N), core((size_t)N), count((size_t)N);
  int32_t n_clusters = -5;
  const int rc = mfa_debug_dbscan_from_bits_host(bits.data(), N, min_samples, labels.data(), core.data(), count.data(), &n_clusters);
  CHECK(rc == 0);
  int32_t seen = -1;
  for (int i = 0; i < N; i++) {
    int32_t n = 0;
    for (size_t j = 0; j < W * 64; j++) {
      const bool want = j < (size_t)N && ((size_t)i == j || bit(in, W, (size_t)i, j) || bit(in, W, j, (size_t)i));
      CHECK(bit(bits, W, (size_t)i, j) == want);
      n += want;
    }
    CHECK(count[i] == n && core[i] == (n >= min_samples));
    CHECK(labels[i] >= -1 && labels[i] < n_clusters);
    if (core[i]) {
      CHECK(labels[i] >= 0 && labels[i] <= seen + 1);    // numbered in the order of the first core index
      if (labels[i] > seen) seen = labels[i];
      for (int j = 0; j < N; j++)
        if (core[j] && bit(bits, W, (size_t)i, (size_t)j)) CHECK(labels[j] == labels[i]);
    } else {
      int32_t best = -1;
      for (int j = 0; j < N; j++)
        if (core[j] && bit(bits, W, (size_t)i, (size_t)j) && (best < 0 || labels[j] < best)) best = labels[j];
      CHECK(labels[i] == best);
    }
  }
  CHECK(seen + 1 == n_clusters);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  for (int metric = 0; metric < 3; metric++) {
    for (int n : {1, 63, 64, 65, 129}) neighbour_bits(n, n, 3, metric, -20.0, false);
    neighbour_bits(5, 130, 5, metric, -30.0, true);
    neighbour_bits(70, 3, 1, metric, 0.0, true);
    neighbour_bits(4, 66, 4, metric, -inf, true);
    neighbour_bits(4, 66, 4, metric, inf, false);
  }
  {                                                  // the refusals
    double x[4] = {1, 2, 3, 4}, psi[2] = {1, 1};
    uint64_t b[2];
    CHECK(mfa_debug_neighbor_bits_host(x, 2, x, 2, 2, 3, nullptr, psi, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == -8);
    CHECK(mfa_debug_neighbor_bits_host(x, 2, x, 2, 2, 1, nullptr, psi, 0, 1, std::nan(""), nullptr, nullptr, nullptr, nullptr, nullptr, b) == -9);
    CHECK(mfa_debug_neighbor_bits_host(x, 2, x, 2, 0, 1, nullptr, psi, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == -2);
    CHECK(mfa_debug_neighbor_bits_host(x, 2, x, 2, 2, 1, nullptr, psi, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -7);
    CHECK(mfa_debug_neighbor_bits_host(x, 2, nullptr, 2, 2, 1, nullptr, psi, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == -1);
    CHECK(mfa_debug_neighbor_bits_host(x, 2, x, 2, 2, 0, nullptr, nullptr, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == -1);
    CHECK(mfa_debug_neighbor_bits_host(nullptr, 0, x, 2, 2, 1, nullptr, psi, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == 0);
    CHECK(mfa_debug_neighbor_sweep_host(x, 2, 2, x, x, psi, 2, 0, 1, std::nan(""), nullptr, nullptr, nullptr, nullptr, nullptr, b) == -9);
    CHECK(mfa_debug_neighbor_sweep_host(x, 2, 2, x, x, psi, 2, 0, 1, 0.0, nullptr, nullptr, nullptr, nullptr, nullptr, b) == 0);
  }
  uint32_t seed = 77u;
  for (int n : {1, 2, 63, 64, 65, 129})
    for (int ms : {1, 3, 6})
      for (int shift : {3, 5}) dbscan(n, ms, seed += 13u, shift);
  {
    int32_t nc = 9, l[1], co[1], cn[1];
    uint64_t b[1] = {0};
    CHECK(mfa_debug_dbscan_from_bits_host(nullptr, 0, 1, nullptr, nullptr, nullptr, &nc) == 0 && nc == 0);
    CHECK(mfa_debug_dbscan_from_bits_host(b, -1, 1, l, co, cn, &nc) == -2);
    CHECK(mfa_debug_dbscan_from_bits_host(b, (int64_t)1 << 31, 1, l, co, cn, &nc) == -2);
    CHECK(mfa_debug_dbscan_from_bits_host(b, 1, 0, l, co, cn, &nc) == -3);
    CHECK(mfa_debug_dbscan_from_bits_host(nullptr, 1, 1, l, co, cn, &nc) == -1);
    CHECK(mfa_debug_dbscan_from_bits_host(b, 1, 1, l, co, cn, nullptr) == -1);
    CHECK(mfa_debug_dbscan_from_bits_host(b, 1, 1, l, co, cn, &nc) == 0 && nc == 1 && l[0] == 0 && co[0] == 1 && cn[0] == 1 && b[0] == 1);
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("cluster twins ok\n");
  return 0;
}
