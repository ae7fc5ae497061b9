// The host twins of the PLDA stage (csrc/plda_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_plda_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: the limits (D = 1 and 1024, k = 1 and 64, more entries asked for than columns),
// dimensions that are no multiple of the step's 4, every combination of outputs, the diagonal excluded, NaN and infinite
// vectors, no train vectors, no test vectors, the transform with each normalisation, the refusals.
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
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0; }

struct Out {
  std::vector<double> scores, best_score, knn_score;
  std::vector<int32_t> best_idx, knn_idx;
};

// which: bit 0 the matrix, bit 1 the best column, bit 2 the k nearest
static Out score(int nt, int ns, int D, int k, int which, bool exclude, bool poison, int *rc) {
  uint32_t s = 11u + (uint32_t)D * 131u + (uint32_t)ns;
  std::vector<double> test((size_t)nt * D), train((size_t)ns * D), psi((size_t)D);
  std::vector<int32_t> n((size_t)ns);
  for (auto &v : test) v = 4.0 * unit(s) - 2.0;
  for (auto &v : train) v = 4.0 * unit(s) - 2.0;
  for (auto &v : psi) v = 0.05 + 4.0 * unit(s);
  for (size_t j = 0; j < n.size(); j++) n[j] = j % 4 == 3 ? 1000 : (int32_t)(1 + j % 3);
  if (poison && nt > 1 && ns > 1) {
    test[(size_t)D] = std::numeric_limits<double>::quiet_NaN();                // row 1
    train[(size_t)D * 1 + (D - 1)] = std::numeric_limits<double>::infinity();    // column 1
    test[0] = 1e200;                                                            // row 0: p·p overflows
  }
  Out o;
  if (which & 1) o.scores.resize((size_t)nt * ns);
  if (which & 2) { o.best_idx.resize((size_t)nt); o.best_score.resize((size_t)nt); }
  if (which & 4) { o.knn_idx.resize((size_t)nt * (k > 0 ? k : 1)); o.knn_score.resize((size_t)nt * (k > 0 ? k : 1)); }
  *rc = mfa_debug_plda_score_host(test.empty() ? nullptr : test.data(), nt, train.empty() ? nullptr : train.data(), ns, D,
                                  n.empty() ? nullptr : n.data(), psi.data(), exclude ? 1 : 0, k, which & 1 ? o.scores.data() : nullptr,
                                  which & 2 ? o.best_idx.data() : nullptr, which & 2 ? o.best_score.data() : nullptr,
                                  which & 4 ? o.knn_idx.data() : nullptr, which & 4 ? o.knn_score.data() : nullptr);
  return o;
}

static void check_lists(const Out &o, int nt, int ns, int k, bool exclude) {
  const int cand = ns - (exclude ? 1 : 0);
  for (int i = 0; i < nt; i++) {
    for (int e = 0; e < k; e++) {
      const int32_t idx = o.knn_idx[(size_t)i * k + e];
      const double sc = o.knn_score[(size_t)i * k + e];
      CHECK(idx >= -1 && idx < ns);
      if (idx < 0) CHECK(std::isinf(sc) && sc < 0);
      else {
        CHECK(std::isfinite(sc));
        CHECK(!(exclude && idx == i));
        if (!o.scores.empty()) CHECK(o.scores[(size_t)i * ns + idx] == sc);
      }
      if (e > 0 && idx >= 0) {
        const double prev = o.knn_score[(size_t)i * k + e - 1];
        CHECK(prev > sc || (prev == sc && o.knn_idx[(size_t)i * k + e - 1] < idx));
      }
      if (e >= cand) CHECK(idx == -1);
    }
    if (!o.best_idx.empty()) CHECK(o.best_idx[i] == o.knn_idx[(size_t)i * k] && (o.best_idx[i] < 0 || o.best_score[i] == o.knn_score[(size_t)i * k]));
  }
}

int main() {
  int rc = 0;
  const int dims[] = {1, 3, 4, 5, 17, 1024};
  for (int D : dims) {
    const int nt = D == 1024 ? 3 : 19, ns = D == 1024 ? 5 : 37;
    for (int k : {1, 5, 64}) {
      for (int excl = 0; excl < 2; excl++) {
        Out o = score(nt, ns, D, k, 7, excl != 0, false, &rc);
        CHECK(rc == 0);
        check_lists(o, nt, ns, k, excl != 0);
      }
    }
    for (int which = 1; which < 8; which++) {
      score(nt, ns, D, 3, which, false, false, &rc);
      CHECK(rc == 0);
    }
  }
  {                                                    // poisoned vectors stay where they are, and are never selected
    Out clean = score(9, 11, 5, 4, 7, false, false, &rc);
    Out o = score(9, 11, 5, 4, 7, false, true, &rc);
    CHECK(rc == 0);
    check_lists(o, 9, 11, 4, false);
    for (int i = 0; i < 9; i++)
      for (int j = 0; j < 11; j++) {
        const double v = o.scores[(size_t)i * 11 + j];
        if (i <= 1 || j == 1) CHECK(!std::isfinite(v));
        else CHECK(v == clean.scores[(size_t)i * 11 + j]);
      }
    CHECK(o.best_idx[0] == -1 && o.best_idx[1] == -1);
    for (int i = 2; i < 9; i++)
      for (int e = 0; e < 4; e++) CHECK(o.knn_idx[(size_t)i * 4 + e] != 1);
  }
  {                                                    // nothing to score
    Out o = score(4, 0, 3, 2, 6, false, false, &rc);
    CHECK(rc == 0);
    for (int i = 0; i < 4; i++) CHECK(o.best_idx[i] == -1 && o.knn_idx[2 * i] == -1 && o.knn_idx[2 * i + 1] == -1);
    score(0, 5, 3, 2, 7, false, false, &rc);
    CHECK(rc == 0);
    score(1, 1, 3, 1, 6, true, false, &rc);            // the only column is the diagonal
    CHECK(rc == 0);
  }
  {                                                    // the refusals
    score(2, 3, 0, 1, 2, false, false, &rc);  CHECK(rc == -2);
    score(2, 3, 4, 0, 4, false, false, &rc);  CHECK(rc == -3);
    score(2, 3, 4, 65, 4, false, false, &rc); CHECK(rc == -3);
    score(2, 3, 4, 1, 0, false, false, &rc);  CHECK(rc == -7);
    std::vector<double> v(8, 1.0), bad(4, 1.0), sc(2);
    std::vector<int32_t> idx(2), n(2, 1);
    CHECK(mfa_debug_plda_score_host(v.data(), 2, v.data(), 2, 4, n.data(), bad.data(), 0, 1, nullptr, idx.data(), nullptr, nullptr, nullptr) == -1);
    bad[3] = 0.0;
    CHECK(mfa_debug_plda_score_host(v.data(), 2, v.data(), 2, 4, n.data(), bad.data(), 0, 1, nullptr, idx.data(), sc.data(), nullptr, nullptr) == -4);
    bad[3] = std::numeric_limits<double>::quiet_NaN();
    CHECK(mfa_debug_plda_score_host(v.data(), 2, v.data(), 2, 4, n.data(), bad.data(), 0, 1, nullptr, idx.data(), sc.data(), nullptr, nullptr) == -4);
    bad[3] = 1.0; n[1] = 0;
    CHECK(mfa_debug_plda_score_host(v.data(), 2, v.data(), 2, 4, n.data(), bad.data(), 0, 1, nullptr, idx.data(), sc.data(), nullptr, nullptr) == -6);
    CHECK(mfa_debug_plda_score_host(v.data(), (int64_t)1 << 31, v.data(), 2, 4, nullptr, bad.data(), 0, 1, nullptr, idx.data(), sc.data(), nullptr, nullptr) == -5);
    CHECK(mfa_debug_plda_score_host(v.data(), -1, v.data(), 2, 4, nullptr, bad.data(), 0, 1, nullptr, idx.data(), sc.data(), nullptr, nullptr) == -1);
  }
  for (int D : {1, 5, 64, 65, 1024}) {                 // the transform
    const int N = D == 1024 ? 2 : 7;
    uint32_t s = 5u + (uint32_t)D;
    std::vector<double> x((size_t)N * D), T((size_t)D * D), off((size_t)D), psi((size_t)D), out((size_t)N * D);
    std::vector<int32_t> n((size_t)N);
    for (auto &v : x) v = 2.0 * unit(s) - 1.0;
    for (auto &v : T) v = 2.0 * unit(s) - 1.0;
    for (auto &v : off) v = unit(s);
    for (auto &v : psi) v = 0.1 + unit(s);
    for (int r = 0; r < N; r++) n[r] = 1 + r % 9;
    for (int norm = 0; norm < 3; norm++) {
      CHECK(mfa_debug_plda_transform_host(x.data(), N, D, T.data(), off.data(), norm == 2 ? psi.data() : nullptr, norm == 2 ? n.data() : nullptr,
                                          norm, out.data()) == 0);
      if (norm == 1)
        for (int r = 0; r < N; r++) {
          double q = 0.0;
          for (int k = 0; k < D; k++) q += out[(size_t)r * D + k] * out[(size_t)r * D + k];
          CHECK(std::fabs(q - D) <= 1e-9 * D);
        }
    }
    CHECK(mfa_debug_plda_transform_host(x.data(), N, D, T.data(), off.data(), nullptr, nullptr, 2, out.data()) == -1);
    CHECK(mfa_debug_plda_transform_host(x.data(), N, D, T.data(), off.data(), nullptr, nullptr, 1, x.data()) == -1);
    CHECK(mfa_debug_plda_transform_host(x.data(), 0, D, T.data(), off.data(), nullptr, nullptr, 1, nullptr) == 0);
  }
  {                                                    // the prepare and sweep entries on their own
    const int ns = 6, nt = 3, D = 5;
    uint32_t s = 3u;
    std::vector<double> train((size_t)ns * D), psi((size_t)D), A((size_t)ns * D), B((size_t)ns * D), c((size_t)ns), test((size_t)nt * D);
    for (auto &v : train) v = unit(s);
    for (auto &v : test) v = unit(s);
    for (auto &v : psi) v = 0.2 + unit(s);
    CHECK(mfa_debug_plda_prepare_host(train.data(), ns, D, nullptr, psi.data(), A.data(), B.data(), c.data()) == 0);
    for (double a : A) CHECK(a < 0.0);
    std::vector<double> sc((size_t)nt * ns), sc2((size_t)nt * ns);
    CHECK(mfa_debug_plda_sweep_host(test.data(), nt, D, A.data(), B.data(), c.data(), ns, 0, 1, sc.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_plda_score_host(test.data(), nt, train.data(), ns, D, nullptr, psi.data(), 0, 1, sc2.data(), nullptr, nullptr, nullptr, nullptr) == 0);
    for (size_t e = 0; e < sc.size(); e++) CHECK(sc[e] == sc2[e]);
    CHECK(mfa_debug_plda_prepare_host(train.data(), 0, D, nullptr, psi.data(), nullptr, nullptr, nullptr) == 0);
  }
  if (failures == 0) printf("plda_check: all passed\n");
  return failures == 0 ? 0 : 1;
}
