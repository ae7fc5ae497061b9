// The host twin of the MLLT statistics (csrc/mllt_acc_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_mllt_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: dim 48 with pdfs of 1, 128 and 3 Gaussians (one visited by nobody), ids outside the
// model, weight 0, posteriors asked for and not, an empty call, one frame by hand, the refusals.
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
  std::vector<float> gc, mi, iv, mu;
};

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static Model make_model(int dim, const std::vector<int> &sizes, uint32_t seed) {
  Model m;
  m.dim = dim;
  m.off.push_back(0);
  for (int n : sizes) m.off.push_back(m.off.back() + n);
  const int G = m.off.back();
  m.gc.resize(G); m.mi.resize((size_t)G * dim); m.iv.resize((size_t)G * dim); m.mu.resize((size_t)G * dim);
  for (int g = 0; g < G; g++) {
    m.gc[g] = -10.0f - unit(seed);
    for (int k = 0; k < dim; k++) {
      const float var = 0.5f + unit(seed), mean = 4.0f * unit(seed) - 2.0f;
      m.iv[(size_t)g * dim + k] = 1.0f / var;
      m.mi[(size_t)g * dim + k] = mean / var;
      m.mu[(size_t)g * dim + k] = m.mi[(size_t)g * dim + k] / m.iv[(size_t)g * dim + k];
    }
  }
  return m;
}

struct Acc {
  std::vector<double> occ, full, tot;
  Acc(int G, int dim) : occ(G, 0.0), full((size_t)G * dim * dim, 0.0), tot(2, 0.0) {}
};

static int run(const Model &m, const std::vector<float> &x, const std::vector<int32_t> &pdf, const std::vector<float> &w, Acc &a,
               std::vector<float> *post, int stride) {
  return mfa_debug_mllt_acc_host(m.dim, (int32_t)m.off.size() - 1, m.off.data(), m.gc.data(), m.mi.data(), m.iv.data(),
                                 m.mu.data(), x.empty() ? nullptr : x.data(), (int64_t)pdf.size(),
                                 pdf.empty() ? nullptr : pdf.data(), w.empty() ? nullptr : w.data(), a.occ.data(), a.full.data(),
                                 a.tot.data(), post ? post->data() : nullptr, stride);
}

int main() {
  uint32_t seed = 12345u;
  {  // dim 48, pdfs of 1, 128 and 3 Gaussians; the last pdf is visited by nobody; ids outside the model; weight 0
    const int D = 48;
    const Model m = make_model(D, {1, 128, 3}, 7u);
    const int T = 120;
    std::vector<float> x((size_t)T * D), w(T);
    std::vector<int32_t> pdf(T);
    for (auto &v : x) v = 6.0f * unit(seed) - 3.0f;
    for (int t = 0; t < T; t++) {
      const int r = (int)(lcg(seed) >> 16) % 8;
      pdf[t] = r < 3 ? 0 : r < 6 ? 1 : r == 6 ? -1 : 3 + (int)(lcg(seed) >> 28);     // 3 and up: not a pdf of the model
      w[t] = (lcg(seed) >> 20) % 5 == 0 ? 0.0f : 0.25f + unit(seed);
    }
    Acc a(132, D);
    std::vector<float> post((size_t)T * 128, -1.0f);
    CHECK(run(m, x, pdf, w, a, &post, 128) == 0);
    double wsum = 0.0, occ = 0.0;
    for (int t = 0; t < T; t++)
      if (pdf[t] >= 0 && pdf[t] < 3 && w[t] != 0.0f) wsum += (double)w[t];
    for (int g = 0; g < 132; g++) occ += a.occ[g];
    CHECK(a.tot[1] == wsum);
    CHECK(std::fabs(occ - wsum) <= 1e-4 * wsum);
    CHECK(std::isfinite(a.tot[0]));
    for (int g = 0; g < 129; g++)        // symmetric, the diagonal not negative, the trace positive where frames arrived
      for (int i = 0; i < D; i++) {
        CHECK(a.full[((size_t)g * D + i) * D + i] >= 0.0);
        for (int j = 0; j < i; j++) CHECK(a.full[((size_t)g * D + i) * D + j] == a.full[((size_t)g * D + j) * D + i]);
      }
    CHECK(a.full[0] > 0.0);
    for (size_t e = (size_t)129 * D * D; e < a.full.size(); e++) CHECK(a.full[e] == 0.0);     // the pdf nobody visits
    for (int g = 129; g < 132; g++) CHECK(a.occ[g] == 0.0);
    // the same without posteriors: the same sums
    Acc b(132, D);
    CHECK(run(m, x, pdf, w, b, nullptr, 0) == 0);
    CHECK(a.occ == b.occ && a.full == b.full && a.tot == b.tot);
    // a stride below the largest pdf is refused before anything is written
    std::vector<float> small((size_t)T * 127);
    Acc c(132, D);
    CHECK(run(m, x, pdf, w, c, &small, 127) == -1);
    CHECK(c.tot[1] == 0.0);
  }
  {  // empty input: nothing is read, nothing is written
    const Model m = make_model(13, {2, 5}, 9u);
    Acc a(7, 13);
    a.occ[3] = 1.5; a.tot[0] = -2.0; a.full[5] = 4.0;
    CHECK(run(m, {}, {}, {}, a, nullptr, 0) == 0);
    CHECK(a.occ[3] == 1.5 && a.tot[0] == -2.0 && a.tot[1] == 0.0 && a.full[5] == 4.0 && a.full[0] == 0.0);
  }
  {  // one frame, one Gaussian: γ = w exactly, d by hand
    Model m = make_model(3, {1}, 11u);
    for (int k = 0; k < 3; k++) { m.iv[k] = 1.0f; m.mi[k] = (float)k; m.mu[k] = (float)k; }
    Acc a(1, 3);
    a.full[1] = 100.0;                   // an upper-triangle value of the caller's is not read: the lower triangle is the value
    const std::vector<float> x = {1.5f, -2.0f, 2.25f}, w = {0.5f};
    const std::vector<int32_t> pdf = {0};
    CHECK(run(m, x, pdf, w, a, nullptr, 0) == 0);
    // d = (1.5, -3, 0.25)
    CHECK(a.occ[0] == 0.5 && a.full[0] == 1.125 && a.full[3] == -2.25 && a.full[1] == -2.25 && a.full[4] == 4.5);
    CHECK(a.full[6] == 0.1875 && a.full[2] == 0.1875 && a.full[7] == -0.375 && a.full[5] == -0.375 && a.full[8] == 0.03125);
  }
  {  // refusals
    const Model big = make_model(4, {129}, 3u);
    Acc a(129, 4);
    CHECK(run(big, {0, 0, 0, 0}, {0}, {1.0f}, a, nullptr, 0) == -2);
    Model empty = make_model(4, {2, 2}, 3u);
    empty.off[1] = 0;   // pdf 0 without Gaussians
    Acc b(4, 4);
    CHECK(run(empty, {0, 0, 0, 0}, {0}, {1.0f}, b, nullptr, 0) == -1);
    const Model wide = make_model(49, {1}, 3u);
    Acc c(1, 49);
    CHECK(run(wide, std::vector<float>(49, 0.0f), {0}, {1.0f}, c, nullptr, 0) == -3);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
