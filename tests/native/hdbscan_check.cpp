// The host twins of the HDBSCAN stage (csrc/hdbscan_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_hdbscan_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: point counts around the word size (1, 2, 3, 63, 64, 65, 130), the three metrics, k
// from 0 to 64, a NaN vector, equal points, the refusals.  What the results must satisfy is checked from the definitions: the
// scores are symmetric, a core score is the k-th best of its row, the edges are a forest in the edge order with the weights of
// the definition, and the tree from the stored matrix is the same tree.
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

static bool better(double m1, int lo1, int hi1, double m2, int lo2, int hi2) {
  return m1 > m2 || (m1 == m2 && (lo1 < lo2 || (lo1 == lo2 && hi1 < hi2)));
}

static int find(std::vector<int> &p, int x) {
  while (p[(size_t)x] != x) x = p[(size_t)x] = p[(size_t)p[(size_t)x]];
  return x;
}

static void run(int N, int D, int metric, int k, bool poison, bool equal) {
  uint32_t s = 9u + (uint32_t)N * 131u + (uint32_t)D * 17u + (uint32_t)metric * 5u + (uint32_t)k;
  std::vector<double> x((size_t)N * D), psi((size_t)D), y((size_t)N * D), q((size_t)N), core((size_t)N), v((size_t)N * N);
  for (auto &e : x) e = equal ? 2.0 : small_int(s);
  for (auto &e : psi) e = 0.5 + (double)(lcg(s) >> 30);
  if (poison && N > 1) x[(size_t)D] = std::numeric_limits<double>::quiet_NaN();      // point 1
  CHECK(mfa_debug_hdbscan_core_host(x.data(), N, D, metric, psi.data(), k, y.data(), q.data(), core.data(), v.data(), nullptr) == 0);
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < N; i++) {
    int above = 0, at = 0, finite = 0;
    for (int j = 0; j < N; j++) {
      const double a = v[(size_t)i * N + j], b = v[(size_t)j * N + i];
      CHECK((a != a && b != b) || a == b);
      if (j == i || !(a - a == 0.0)) continue;
      finite++;
      above += a > core[(size_t)i];
      at += a == core[(size_t)i];
    }
    if (k == 0) CHECK(core[(size_t)i] == inf);
    else if (finite < k) CHECK(core[(size_t)i] == -inf);
    else CHECK(above < k && above + at >= k);
    if (poison && N > 1 && i == 1) CHECK(finite == 0);
  }
  std::vector<double> core2((size_t)N);                                                // the same cores from the matrix handed back
  std::vector<double> y2((size_t)N * D), q2((size_t)N);
  CHECK(mfa_debug_hdbscan_core_host(x.data(), N, D, metric, psi.data(), k, y2.data(), q2.data(), core2.data(), nullptr, v.data()) == 0);
  for (int i = 0; i < N; i++) CHECK(core2[(size_t)i] == core[(size_t)i]);
  const size_t M = (size_t)(N > 1 ? N - 1 : 1);
  std::vector<int32_t> lo(M), hi(M);
  std::vector<double> m(M);
  int32_t n_edges = -3;
  CHECK(mfa_debug_hdbscan_mst_host(y.data(), q.data(), core.data(), nullptr, N, D, metric, lo.data(), hi.data(), m.data(), &n_edges) == 0);
  CHECK(n_edges >= 0 && n_edges <= N - 1 + (N == 0));
  const int want = poison && N > 1 ? N - 2 : N - 1;
  CHECK(n_edges == (N > 0 ? want : 0));
  std::vector<int> parent((size_t)N);
  for (int i = 0; i < N; i++) parent[(size_t)i] = i;
  for (int e = 0; e < n_edges; e++) {
    CHECK(lo[(size_t)e] >= 0 && lo[(size_t)e] < hi[(size_t)e] && hi[(size_t)e] < N);
    if (e > 0) CHECK(better(m[(size_t)e - 1], lo[(size_t)e - 1], hi[(size_t)e - 1], m[(size_t)e], lo[(size_t)e], hi[(size_t)e]));
    const int a = find(parent, lo[(size_t)e]), b = find(parent, hi[(size_t)e]);
    CHECK(a != b);
    parent[(size_t)a] = b;
    const double vij = v[(size_t)lo[(size_t)e] * N + hi[(size_t)e]];
    const double cm = core[(size_t)lo[(size_t)e]] < core[(size_t)hi[(size_t)e]] ? core[(size_t)lo[(size_t)e]] : core[(size_t)hi[(size_t)e]];
    CHECK(m[(size_t)e] == (vij < cm ? vij : cm));
  }
  std::vector<int32_t> lo2(M), hi2(M);                                                 // and from the matrix
  std::vector<double> m2(M);
  int32_t n2 = -3;
  CHECK(mfa_debug_hdbscan_mst_host(nullptr, nullptr, core.data(), v.data(), N, D, metric, lo2.data(), hi2.data(), m2.data(), &n2) == 0);
  CHECK(n2 == n_edges);
  for (int e = 0; e < n_edges && e < n2; e++) CHECK(lo2[(size_t)e] == lo[(size_t)e] && hi2[(size_t)e] == hi[(size_t)e] && m2[(size_t)e] == m[(size_t)e]);
}

int main() {
  for (int metric = 0; metric < 3; metric++) {
    for (int n : {1, 2, 3, 63, 64, 65, 130})
      for (int k : {0, 1, 4, 64}) run(n, 3, metric, k, false, false);
    run(70, 5, metric, 3, true, false);
    run(20, 1, metric, 2, false, true);
    run(66, 50, metric, 5, false, false);
  }
  {                                                  // the refusals
    double x[4] = {1, 2, 3, 4}, psi[2] = {1, 1}, bad[2] = {1, -1}, y[4], q[2], core[2], m[1];
    int32_t lo[1], hi[1], n = 7;
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 3, psi, 1, y, q, core, nullptr, nullptr) == -8);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 0, 1, psi, 1, y, q, core, nullptr, nullptr) == -2);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 1025, 1, psi, 1, y, q, core, nullptr, nullptr) == -2);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 1, psi, 65, y, q, core, nullptr, nullptr) == -3);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 1, psi, -1, y, q, core, nullptr, nullptr) == -3);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 0, bad, 1, y, q, core, nullptr, nullptr) == -4);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 0, nullptr, 1, y, q, core, nullptr, nullptr) == -1);
    CHECK(mfa_debug_hdbscan_core_host(x, (int64_t)1 << 31, 2, 1, psi, 1, y, q, core, nullptr, nullptr) == -5);
    CHECK(mfa_debug_hdbscan_core_host(x, -1, 2, 1, psi, 1, y, q, core, nullptr, nullptr) == -1);
    CHECK(mfa_debug_hdbscan_core_host(nullptr, 2, 2, 1, psi, 1, y, q, core, nullptr, nullptr) == -1);
    CHECK(mfa_debug_hdbscan_core_host(nullptr, 0, 2, 1, psi, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_hdbscan_core_host(x, 2, 2, 1, nullptr, 1, y, q, core, nullptr, nullptr) == 0);
    CHECK(mfa_debug_hdbscan_mst_host(y, q, core, nullptr, 2, 2, 4, lo, hi, m, &n) == -8);
    CHECK(mfa_debug_hdbscan_mst_host(y, q, core, nullptr, 2, 2, 1, lo, hi, m, nullptr) == -1);
    CHECK(mfa_debug_hdbscan_mst_host(y, q, nullptr, nullptr, 2, 2, 1, lo, hi, m, &n) == -1);
    CHECK(mfa_debug_hdbscan_mst_host(nullptr, q, core, nullptr, 2, 2, 1, lo, hi, m, &n) == -1);
    CHECK(mfa_debug_hdbscan_mst_host(y, q, core, nullptr, 2, 2, 1, lo, hi, m, &n) == 0 && n == 1 && lo[0] == 0 && hi[0] == 1);
    CHECK(mfa_debug_hdbscan_mst_host(nullptr, nullptr, nullptr, nullptr, 1, 2, 1, nullptr, nullptr, nullptr, &n) == 0 && n == 0);
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("hdbscan twins ok\n");
  return 0;
}
