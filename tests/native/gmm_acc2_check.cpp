// The two-feature host twin of the GMM statistics (mfa_debug_gmm_acc_twofeats_host, csrc/gmm_acc_host.cpp) as a stand-alone
// program for the host sanitizers: tests/test_gmm_acc_twofeats_cpu.py builds it with -fsanitize=address,undefined and runs it
// once.  Every array is sized exactly, so an index past an end of either matrix is a report.  Inputs: 128 Gaussians at dim 48
// with ids outside the model, equal matrices against the one-feature twin, an empty call, a frame whose sums are known
// exactly, the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mfa_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

struct Model {
  int dim;
  std::vector<int32_t> off;
  std::vector<float> gc, mi, iv;
};

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static Model make_model(int dim, const std::vector<int> &sizes, uint32_t seed) {
  Model m;
  m.dim = dim;
  m.off.push_back(0);
  for (int n : sizes) m.off.push_back(m.off.back() + n);
  const int G = m.off.back();
  m.gc.resize(G); m.mi.resize((size_t)G * dim); m.iv.resize((size_t)G * dim);
  for (int g = 0; g < G; g++) {
    m.gc[g] = -10.0f - unit(seed);
    for (int k = 0; k < dim; k++) {
      const float var = 0.5f + unit(seed), mean = 4.0f * unit(seed) - 2.0f;
      m.iv[(size_t)g * dim + k] = 1.0f / var;
      m.mi[(size_t)g * dim + k] = mean / var;
    }
  }
  return m;
}

struct Acc {
  std::vector<double> occ, mean, var, tot;
  std::vector<int64_t> cnt;
  Acc(int G, int dim, int n_tids) : occ(G, 0.0), mean((size_t)G * dim, 0.0), var((size_t)G * dim, 0.0), tot(2, 0.0), cnt(n_tids, 0) {}
};

static const float *ptr(const std::vector<float> &v) { return v.empty() ? nullptr : v.data(); }

static int run2(const Model &m, const std::vector<float> &x, const std::vector<float> &y, const std::vector<int32_t> &pdf,
                const std::vector<float> &w, const std::vector<int32_t> *tid, int n_tids, Acc &a, std::vector<float> *post, int stride) {
  return mfa_debug_gmm_acc_twofeats_host(m.dim, (int32_t)m.off.size() - 1, m.off.data(), m.gc.data(), m.mi.data(), m.iv.data(), ptr(x),
                                         ptr(y), (int64_t)pdf.size(), pdf.empty() ? nullptr : pdf.data(), ptr(w),
                                         tid ? tid->data() : nullptr, n_tids, a.occ.data(), a.mean.data(), a.var.data(), a.tot.data(),
                                         tid ? a.cnt.data() : nullptr, post ? post->data() : nullptr, stride);
}

static int run1(const Model &m, const std::vector<float> &x, const std::vector<int32_t> &pdf, const std::vector<float> &w,
                const std::vector<int32_t> *tid, int n_tids, Acc &a, std::vector<float> *post, int stride) {
  return mfa_debug_gmm_acc_host(m.dim, (int32_t)m.off.size() - 1, m.off.data(), m.gc.data(), m.mi.data(), m.iv.data(), ptr(x),
                                (int64_t)pdf.size(), pdf.empty() ? nullptr : pdf.data(), ptr(w), tid ? tid->data() : nullptr, n_tids,
                                a.occ.data(), a.mean.data(), a.var.data(), a.tot.data(), tid ? a.cnt.data() : nullptr,
                                post ? post->data() : nullptr, stride);
}

int main() {
  uint32_t seed = 4321u;
  {  // dim 48, pdfs of 1, 128 and 3 Gaussians; ids outside the model; weight 0; two different matrices
    const Model m = make_model(48, {1, 128, 3}, 7u);
    const int T = 300, n_tids = 7;
    std::vector<float> x((size_t)T * 48), y((size_t)T * 48), w(T);
    std::vector<int32_t> pdf(T), tid(T);
    for (auto &v : x) v = 6.0f * unit(seed) - 3.0f;
    for (auto &v : y) v = 6.0f * unit(seed) - 3.0f;
    for (int t = 0; t < T; t++) {
      const int r = (int)(lcg(seed) >> 16) % 8;
      pdf[t] = r < 3 ? 0 : r < 6 ? 1 : r == 6 ? -1 : 3 + (int)(lcg(seed) >> 28);
      w[t] = (lcg(seed) >> 20) % 5 == 0 ? 0.0f : 0.25f + unit(seed);
      tid[t] = (int)(lcg(seed) >> 16) % 12 - 2;
    }
    Acc a(132, 48, n_tids), one(132, 48, n_tids), same(132, 48, n_tids);
    std::vector<float> post((size_t)T * 128, -1.0f), post1((size_t)T * 128, -1.0f);
    CHECK(run2(m, x, y, pdf, w, &tid, n_tids, a, &post, 128) == 0);
    CHECK(run1(m, x, pdf, w, &tid, n_tids, one, &post1, 128) == 0);
    // posteriors, occupancies, totals and counts follow x alone; the sums follow y
    CHECK(post == post1 && a.occ == one.occ && a.tot == one.tot && a.cnt == one.cnt);
    CHECK(a.mean != one.mean && a.var != one.var);
    // the pdf of one Gaussian: gamma = w exactly, so its sums are those of y's rows, formed the same way
    double mean0 = 0.0, var0 = 0.0;
    for (int t = 0; t < T; t++)
      if (pdf[t] == 0 && w[t] != 0.0f) {
        const double v = (double)y[(size_t)t * 48 + 47];
        mean0 = std::fma((double)w[t], v, mean0);
        var0 = std::fma((double)w[t], v * v, var0);
      }
    CHECK(a.mean[47] == mean0 && a.var[47] == var0);
    // equal matrices, and the same array twice: the one-feature twin's bits
    const std::vector<float> copy = x;
    CHECK(run2(m, x, copy, pdf, w, &tid, n_tids, same, nullptr, 0) == 0);
    CHECK(same.occ == one.occ && same.mean == one.mean && same.var == one.var && same.tot == one.tot && same.cnt == one.cnt);
    Acc twice(132, 48, n_tids);
    CHECK(run2(m, x, x, pdf, w, nullptr, 0, twice, nullptr, 0) == 0);
    CHECK(twice.mean == one.mean && twice.var == one.var);
    // a stride below the largest pdf is refused before anything is written
    std::vector<float> small((size_t)T * 127);
    Acc c(132, 48, n_tids);
    CHECK(run2(m, x, y, pdf, w, nullptr, 0, c, &small, 127) == -1);
    CHECK(c.tot[1] == 0.0);
    // no sum matrix with frames
    CHECK(run2(m, x, {}, pdf, w, nullptr, 0, c, nullptr, 0) == -1);
    CHECK(c.tot[1] == 0.0);
  }
  {  // empty input: nothing is read, nothing is written
    const Model m = make_model(13, {2, 5}, 9u);
    Acc a(7, 13, 4);
    a.occ[3] = 1.5; a.tot[0] = -2.0;
    CHECK(run2(m, {}, {}, {}, {}, nullptr, 0, a, nullptr, 0) == 0);
    CHECK(a.occ[3] == 1.5 && a.tot[0] == -2.0 && a.tot[1] == 0.0);
  }
  {  // one frame, one Gaussian: γ = w exactly, sums are the second matrix's row
    const Model m = make_model(3, {1}, 11u);
    Acc a(1, 3, 2);
    const std::vector<float> x = {9.0f, 9.0f, 9.0f}, y = {1.5f, -2.0f, 0.25f}, w = {0.5f};
    const std::vector<int32_t> pdf = {0}, tid = {1};
    CHECK(run2(m, x, y, pdf, w, &tid, 2, a, nullptr, 0) == 0);
    CHECK(a.occ[0] == 0.5 && a.mean[0] == 0.75 && a.mean[1] == -1.0 && a.var[1] == 2.0 && a.var[2] == 0.03125 && a.cnt[1] == 1);
  }
  {  // refusals
    const Model big = make_model(4, {129}, 3u);
    Acc a(129, 4, 1);
    CHECK(run2(big, {0, 0, 0, 0}, {0, 0, 0, 0}, {0}, {1.0f}, nullptr, 0, a, nullptr, 0) == -2);
    Model empty = make_model(4, {2, 2}, 3u);
    empty.off[1] = 0;   // pdf 0 without Gaussians
    Acc b(4, 4, 1);
    CHECK(run2(empty, {0, 0, 0, 0}, {0, 0, 0, 0}, {0}, {1.0f}, nullptr, 0, b, nullptr, 0) == -1);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
