// The host twin of the silhouette stage (csrc/silhouette_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_silhouette_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: point counts around the step size (2, 3, 63, 64, 65, 130, 300), the three metrics,
// cluster layouts with boundaries at and around column 64, singletons, many clusters in one step, equal points, the refusals.
// What the results must satisfy is checked from the definitions on the twin's own score matrix: a and b are the means the
// definition names (small integers: every sum is exact for the dot metric, so equality is asked there), bj is the lowest cluster
// with the least mean, a singleton scores 0, and the twin on the matrix handed back returns the same bits.
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

static bool close(double a, double b) { return a == b || std::fabs(a - b) <= 1e-9 * (1.0 + std::fabs(a) + std::fabs(b)); }

static void run(int N, int D, int metric, const std::vector<int32_t> &off, bool equal) {
  const int C = (int)off.size() - 1;
  uint32_t s = 11u + (uint32_t)N * 131u + (uint32_t)D * 17u + (uint32_t)metric * 5u + (uint32_t)C;
  std::vector<double> x((size_t)N * D), psi((size_t)D), sil((size_t)N), a((size_t)N), b((size_t)N), v((size_t)N * N);
  std::vector<int32_t> bj((size_t)N);
  for (auto &e : x) e = equal ? 2.0 : small_int(s);
  for (auto &e : psi) e = 0.5 + (double)(lcg(s) >> 30);
  CHECK(mfa_debug_silhouette_host(x.data(), N, D, metric, psi.data(), off.data(), C, sil.data(), a.data(), b.data(), bj.data(), v.data(),
                                  nullptr) == 0);
  const double inf = std::numeric_limits<double>::infinity();
  for (int i = 0; i < N; i++) {
    int own = 0;
    while (off[(size_t)own + 1] <= i) own++;
    double best = inf;
    int best_c = -1;
    for (int c = 0; c < C; c++) {
      double S = 0.0;
      for (int j = off[(size_t)c]; j < off[(size_t)c + 1]; j++) {
        if (j == i) continue;
        const double vij = v[(size_t)i * N + j];
        S += metric == 0 ? -vij : (metric == 1 ? std::sqrt(vij < 0.0 ? -vij : 0.0) : 1.0 - vij);
      }
      const int n_c = off[(size_t)c + 1] - off[(size_t)c];
      if (c == own) {
        const double want = n_c > 1 ? S / (n_c - 1) : 0.0;
        CHECK(metric == 2 ? a[(size_t)i] == want : close(a[(size_t)i], want));
      } else if (S / n_c < best) {
        best = S / n_c;
        best_c = c;
      }
    }
    CHECK(metric == 2 ? b[(size_t)i] == best : close(b[(size_t)i], best));
    if (metric == 2) CHECK(bj[(size_t)i] == best_c);
    CHECK(bj[(size_t)i] >= 0 && bj[(size_t)i] < C && bj[(size_t)i] != own);
    const int n_own = off[(size_t)own + 1] - off[(size_t)own];
    const double den = a[(size_t)i] < b[(size_t)i] ? b[(size_t)i] : a[(size_t)i];
    if (n_own == 1 || den == 0.0) CHECK(sil[(size_t)i] == 0.0);
    else CHECK(sil[(size_t)i] == (b[(size_t)i] - a[(size_t)i]) / den);
    if (metric == 1) CHECK(sil[(size_t)i] >= -1.0 && sil[(size_t)i] <= 1.0);   // a distance that is never negative
  }
  std::vector<double> sil2((size_t)N);                                                 // the same from the matrix handed back, no parts
  CHECK(mfa_debug_silhouette_host(x.data(), N, D, metric, psi.data(), off.data(), C, sil2.data(), nullptr, nullptr, nullptr, nullptr,
                                  v.data()) == 0);
  for (int i = 0; i < N; i++) CHECK(sil2[(size_t)i] == sil[(size_t)i]);
}

static std::vector<int32_t> singletons_but_a_pair(int n) {
  std::vector<int32_t> off = {0, 2};
  for (int j = 3; j <= n; j++) off.push_back(j);
  return off;
}

int main() {
  for (int metric = 0; metric < 3; metric++) {
    for (int n : {2, 3, 63, 64, 65, 130, 300}) {
      run(n, 3, metric, {0, n / 2, n}, false);
      if (n >= 3) run(n, 3, metric, singletons_but_a_pair(n), false);
      if (n >= 66) run(n, 5, metric, {0, 64, n}, false);
      if (n >= 66) run(n, 4, metric, {0, 63, 64, 65, n}, false);
      if (n >= 200) run(n, 1, metric, {0, 20, 190, n}, false);
      if (n >= 40) {
        std::vector<int32_t> off;
        for (int j = 0; j < 36; j += 2) off.push_back(j);
        off.push_back(n);
        run(n, 3, metric, off, false);
      }
    }
    run(20, 2, metric, {0, 7, 20}, true);
    run(66, 50, metric, {0, 30, 31, 66}, false);
  }
  {                                                  // the refusals
    double x[6] = {1, 2, 3, 4, 5, 6}, psi[2] = {1, 1}, bad[2] = {1, -1}, sil[3];
    int32_t off[3] = {0, 1, 3}, off1[2] = {0, 3}, empty[3] = {0, 0, 3}, late[3] = {1, 2, 3}, shrt[3] = {0, 1, 2}, back[4] = {0, 2, 1, 3};
    int32_t each[4] = {0, 1, 2, 3};
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 3, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -8);
    CHECK(mfa_debug_silhouette_host(x, 3, 0, 1, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -2);
    CHECK(mfa_debug_silhouette_host(x, 3, 1025, 1, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -2);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 0, bad, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -4);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 0, nullptr, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(mfa_debug_silhouette_host(x, (int64_t)1 << 31, 2, 1, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(mfa_debug_silhouette_host(x, -1, 2, 1, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, off1, 1, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -6);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, off, 4, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -6);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, empty, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -7);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, late, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -7);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, shrt, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -7);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, back, 3, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -7);
    CHECK(mfa_debug_silhouette_host(nullptr, 3, 2, 1, psi, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, nullptr, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, psi, off, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1);
    CHECK(mfa_debug_silhouette_host(nullptr, 0, 2, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, nullptr, off, 2, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_silhouette_host(x, 3, 2, 1, nullptr, each, 3, sil, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 && sil[0] == 0.0 &&
          sil[1] == 0.0 && sil[2] == 0.0);
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("silhouette twin ok\n");
  return 0;
}
