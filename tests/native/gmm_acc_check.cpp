// The host twin of the GMM statistics (csrc/gmm_acc_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_gmm_acc_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so
// an index past an end is a report.  Inputs: an empty call, a pdf nobody visits, ids outside the model, 128 Gaussians, dim 48,
// posteriors asked for and not, the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static int run(const Model &m, const std::vector<float> &x, const std::vector<int32_t> &pdf, const std::vector<float> &w,
               const std::vector<int32_t> *tid, int n_tids, Acc &a, std::vector<float> *post, int stride) {
  return mfa_debug_gmm_acc_host(m.dim, (int32_t)m.off.size() - 1, m.off.data(), m.gc.data(), m.mi.data(), m.iv.data(),
                                x.empty() ? nullptr : x.data(), (int64_t)pdf.size(), pdf.empty() ? nullptr : pdf.data(),
                                w.empty() ? nullptr : w.data(), tid ? tid->data() : nullptr, n_tids, a.occ.data(), a.mean.data(),
                                a.var.data(), a.tot.data(), tid ? a.cnt.data() : nullptr, post ? post->data() : nullptr, stride);
}

int main() {
  uint32_t seed = 12345u;
  {  // dim 48, pdfs of 1, 128 and 3 Gaussians; the last pdf is visited by nobody; ids outside the model; weight 0
    const Model m = make_model(48, {1, 128, 3}, 7u);
    const int T = 300, n_tids = 7;
    std::vector<float> x((size_t)T * 48), w(T);
    std::vector<int32_t> pdf(T), tid(T);
    for (auto &v : x) v = 6.0f * unit(seed) - 3.0f;
    for (int t = 0; t < T; t++) {
      const int r = (int)(lcg(seed) >> 16) % 8;
      pdf[t] = r < 3 ? 0 : r < 6 ? 1 : r == 6 ? -1 : 3 + (int)(lcg(seed) >> 28);     // 3 and up: not a pdf of the model
      w[t] = (lcg(seed) >> 20) % 5 == 0 ? 0.0f : 0.25f + unit(seed);
      tid[t] = (int)(lcg(seed) >> 16) % 12 - 2;                                       // −2 … 9: some outside [1, n_tids)
    }
    Acc a(132, 48, n_tids);
    std::vector<float> post((size_t)T * 128, -1.0f);
    CHECK(run(m, x, pdf, w, &tid, n_tids, a, &post, 128) == 0);
    double wsum = 0.0, occ = 0.0;
    int64_t counted = 0, expect = 0;
    for (int t = 0; t < T; t++) {
      const bool takes = pdf[t] >= 0 && pdf[t] < 3 && w[t] != 0.0f;
      if (takes) wsum += (double)w[t];
      if (takes && tid[t] > 0 && tid[t] < n_tids) expect++;
      float s = 0.0f;
      for (int g = 0; g < 128; g++) { CHECK(post[(size_t)t * 128 + g] >= 0.0f); s += post[(size_t)t * 128 + g]; }
      CHECK(takes ? std::fabs(s - w[t]) <= 1e-4f * w[t] : s == 0.0f);
    }
    for (int g = 0; g < 132; g++) occ += a.occ[g];
    for (int64_t c : a.cnt) counted += c;
    CHECK(a.tot[1] == wsum);
    CHECK(std::fabs(occ - wsum) <= 1e-4 * wsum);
    CHECK(counted == expect);
    for (int g = 129; g < 132; g++) {   // the pdf nobody visits
      CHECK(a.occ[g] == 0.0);
      for (int k = 0; k < 48; k++) CHECK(a.mean[(size_t)g * 48 + k] == 0.0 && a.var[(size_t)g * 48 + k] == 0.0);
    }
    CHECK(std::isfinite(a.tot[0]));
    // the same without posteriors and without counts: the same sums
    Acc b(132, 48, n_tids);
    CHECK(run(m, x, pdf, w, nullptr, 0, b, nullptr, 0) == 0);
    CHECK(a.occ == b.occ && a.mean == b.mean && a.var == b.var && a.tot == b.tot);
    // a stride below the largest pdf is refused before anything is written
    std::vector<float> small((size_t)T * 127);
    Acc c(132, 48, n_tids);
    CHECK(run(m, x, pdf, w, nullptr, 0, c, &small, 127) == -1);
    CHECK(c.tot[1] == 0.0);
  }
  {  // empty input: nothing is read, nothing is written
    const Model m = make_model(13, {2, 5}, 9u);
    Acc a(7, 13, 4);
    a.occ[3] = 1.5; a.tot[0] = -2.0;
    CHECK(run(m, {}, {}, {}, nullptr, 0, a, nullptr, 0) == 0);
    CHECK(a.occ[3] == 1.5 && a.tot[0] == -2.0 && a.tot[1] == 0.0);
  }
  {  // one frame, one Gaussian: γ = w exactly, sums are the frame's
    const Model m = make_model(3, {1}, 11u);
    Acc a(1, 3, 2);
    const std::vector<float> x = {1.5f, -2.0f, 0.25f}, w = {0.5f};
    const std::vector<int32_t> pdf = {0}, tid = {1};
    CHECK(run(m, x, pdf, w, &tid, 2, a, nullptr, 0) == 0);
    CHECK(a.occ[0] == 0.5 && a.mean[0] == 0.75 && a.mean[1] == -1.0 && a.var[1] == 2.0 && a.var[2] == 0.03125 && a.cnt[1] == 1);
  }
  {  // refusals
    const Model big = make_model(4, {129}, 3u);
    Acc a(129, 4, 1);
    CHECK(run(big, {0, 0, 0, 0}, {0}, {1.0f}, nullptr, 0, a, nullptr, 0) == -2);
    Model empty = make_model(4, {2, 2}, 3u);
    empty.off[1] = 0;   // pdf 0 without Gaussians
    Acc b(4, 4, 1);
    CHECK(run(empty, {0, 0, 0, 0}, {0}, {1.0f}, nullptr, 0, b, nullptr, 0) == -1);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
