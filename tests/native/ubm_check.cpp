// The host twins of the diagonal-UBM stage (csrc/ubm_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_ubm_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: dim 48 with 2048 Gaussians and lists of 64, a list longer than the model, NaN and
// infinite rows, indices outside the model, weight 0, the dense path, empty calls, the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <set>
#include <vector>

#include "../../include/mfa_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

struct Model {
  int dim, G;
  std::vector<float> gc, mi, iv;
};

static Model make_model(int dim, int G, uint32_t seed) {
  Model m{dim, G, std::vector<float>(G), std::vector<float>((size_t)G * dim), std::vector<float>((size_t)G * dim)};
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

static int select(const Model &m, const std::vector<float> &x, int n, std::vector<int32_t> &gs, std::vector<float> *ll) {
  const int64_t T = (int64_t)(x.size() / m.dim);
  return mfa_debug_ubm_gselect_host(x.empty() ? nullptr : x.data(), T, m.dim, m.G, m.gc.data(), m.mi.data(), m.iv.data(), n,
                                    gs.empty() ? nullptr : gs.data(), ll ? ll->data() : nullptr);
}

struct Acc {
  std::vector<double> occ, mean, var, tot;
  Acc(int G, int dim) : occ(G, 0.0), mean((size_t)G * dim, 0.0), var((size_t)G * dim, 0.0), tot(2, 0.0) {}
};

static int acc(const Model &m, const std::vector<float> &x, int n, const std::vector<int32_t> *gs, const std::vector<float> *w, Acc &a,
               std::vector<float> *post) {
  const int64_t T = (int64_t)(x.size() / m.dim);
  return mfa_debug_ubm_acc_host(x.empty() ? nullptr : x.data(), T, m.dim, m.G, m.gc.data(), m.mi.data(), m.iv.data(), n,
                                gs ? gs->data() : nullptr, w ? w->data() : nullptr, a.occ.data(), a.mean.data(), a.var.data(),
                                a.tot.data(), post ? post->data() : nullptr);
}

int main() {
  uint32_t seed = 4242u;
  {  // the largest shapes: dim 48, 2048 Gaussians, lists of 64; a NaN row and an infinite row
    const Model m = make_model(48, 2048, 5u);
    const int T = 40, n = 64;
    std::vector<float> x((size_t)T * 48), ll(T);
    for (auto &v : x) v = 6.0f * unit(seed) - 3.0f;
    for (int k = 0; k < 48; k++) x[(size_t)3 * 48 + k] = std::numeric_limits<float>::quiet_NaN();
    x[(size_t)7 * 48 + 5] = std::numeric_limits<float>::infinity();
    std::vector<int32_t> gs((size_t)T * n, -9);
    CHECK(select(m, x, n, gs, &ll) == 0);
    for (int t = 0; t < T; t++) {
      std::set<int32_t> seen;
      for (int j = 0; j < n; j++) { const int32_t g = gs[(size_t)t * n + j]; CHECK(g >= 0 && g < 2048); seen.insert(g); }
      CHECK((int)seen.size() == n);
      if (t != 3 && t != 7) CHECK(std::isfinite(ll[t]));
    }
    // statistics over the selection, some entries outside the model, some frames of weight 0
    std::vector<float> w(T, 1.0f), post((size_t)T * n, -1.0f);
    for (int t = 0; t < T; t += 5) w[t] = 0.0f;
    w[1] = 0.5f;
    for (int t = 0; t < T; t++) gs[(size_t)t * n + (t % n)] = t % 2 ? -1 : 2048;
    for (int j = 0; j < n; j++) gs[(size_t)9 * n + j] = 5000 + j;              // frame 9: no valid entry at all
    Acc a(2048, 48);
    std::vector<float> fin;
    std::vector<int32_t> gfin;
    std::vector<float> wfin;
    for (int t = 0; t < T; t++)
      if (t != 3 && t != 7) {
        fin.insert(fin.end(), x.begin() + (size_t)t * 48, x.begin() + (size_t)(t + 1) * 48);
        gfin.insert(gfin.end(), gs.begin() + (size_t)t * n, gs.begin() + (size_t)(t + 1) * n);
        wfin.push_back(w[t]);
      }
    post.resize(wfin.size() * n);
    CHECK(acc(m, fin, n, &gfin, &wfin, a, &post) == 0);
    double wsum = 0.0, occ = 0.0;
    for (size_t t = 0; t < wfin.size(); t++) {
      bool any = false;
      float s = 0.0f;
      for (int j = 0; j < n; j++) {
        const int32_t g = gfin[t * n + j];
        any = any || (g >= 0 && g < 2048);
        CHECK(post[t * n + j] >= 0.0f);
        if (g < 0 || g >= 2048) CHECK(post[t * n + j] == 0.0f);
        s += post[t * n + j];
      }
      const bool takes = any && wfin[t] != 0.0f;
      if (takes) wsum += (double)wfin[t];
      CHECK(takes ? std::fabs(s - wfin[t]) <= 1e-4f * wfin[t] : s == 0.0f);
    }
    for (double v : a.occ) occ += v;
    CHECK(a.tot[1] == wsum);
    CHECK(std::fabs(occ - wsum) <= 1e-4 * wsum);
    CHECK(std::isfinite(a.tot[0]));
    // the same without posteriors: the same sums
    Acc b(2048, 48);
    CHECK(acc(m, fin, n, &gfin, &wfin, b, nullptr) == 0);
    CHECK(a.occ == b.occ && a.mean == b.mean && a.var == b.var && a.tot == b.tot);
  }
  {  // a list longer than the model returns every Gaussian, sorted; the dense path over the same frames
    const Model m = make_model(13, 5, 8u);
    const int T = 9;
    std::vector<float> x((size_t)T * 13), ll(T);
    for (auto &v : x) v = 4.0f * unit(seed) - 2.0f;
    std::vector<int32_t> gs((size_t)T * 5);
    CHECK(select(m, x, 64 + 30, gs, &ll) == 0);
    for (int t = 0; t < T; t++) {
      std::set<int32_t> seen(gs.begin() + t * 5, gs.begin() + (t + 1) * 5);
      CHECK(seen.size() == 5 && *seen.begin() == 0 && *seen.rbegin() == 4);
    }
    Acc a(5, 13), b(5, 13);
    CHECK(acc(m, x, 5, &gs, nullptr, a, nullptr) == 0);
    CHECK(acc(m, x, 0, nullptr, nullptr, b, nullptr) == 0);
    CHECK(a.tot[1] == (double)T && b.tot[1] == (double)T);
    CHECK(std::fabs(a.tot[0] - b.tot[0]) <= 1e-4 * std::fabs(b.tot[0]));     // the same softmax in another order
  }
  {  // one frame, one Gaussian: γ = w exactly, the sums are the frame's
    const Model m = make_model(3, 1, 11u);
    Acc a(1, 3);
    const std::vector<float> x = {1.5f, -2.0f, 0.25f}, w = {0.5f};
    const std::vector<int32_t> gs = {0};
    CHECK(acc(m, x, 1, &gs, &w, a, nullptr) == 0);
    CHECK(a.occ[0] == 0.5 && a.mean[0] == 0.75 && a.mean[1] == -1.0 && a.var[1] == 2.0 && a.var[2] == 0.03125 && a.tot[1] == 0.5);
  }
  {  // empty input: nothing is read, nothing is written
    const Model m = make_model(13, 7, 9u);
    Acc a(7, 13);
    a.occ[3] = 1.5; a.tot[0] = -2.0;
    std::vector<int32_t> none;
    CHECK(acc(m, {}, 4, &none, nullptr, a, nullptr) == 0);
    CHECK(acc(m, {}, 0, nullptr, nullptr, a, nullptr) == 0);
    CHECK(a.occ[3] == 1.5 && a.tot[0] == -2.0 && a.tot[1] == 0.0);
    CHECK(select(m, {}, 4, none, nullptr) == 0);
  }
  {  // refusals: nothing is touched
    const Model m = make_model(4, 70, 3u);
    const std::vector<float> x(4, 0.0f);
    std::vector<int32_t> gs(70);
    std::vector<float> post(70);
    Acc a(70, 4);
    CHECK(select(m, x, 0, gs, nullptr) == -4);
    CHECK(select(m, x, 65, gs, nullptr) == -4);
    CHECK(acc(m, x, 65, &gs, nullptr, a, nullptr) == -4);
    CHECK(acc(m, x, 0, &gs, nullptr, a, nullptr) == -4);
    CHECK(acc(m, x, 4, nullptr, nullptr, a, &post) == -1);
    CHECK(mfa_debug_ubm_gselect_host(x.data(), 0, 49, 70, m.gc.data(), m.mi.data(), m.iv.data(), 4, gs.data(), nullptr) == -2);
    CHECK(mfa_debug_ubm_gselect_host(x.data(), 0, 4, 2049, m.gc.data(), m.mi.data(), m.iv.data(), 4, gs.data(), nullptr) == -3);
    CHECK(mfa_debug_ubm_gselect_host(x.data(), 0, 4, 0, m.gc.data(), m.mi.data(), m.iv.data(), 4, gs.data(), nullptr) == -3);
    CHECK(mfa_debug_ubm_gselect_host(x.data(), (int64_t)1 << 31, 4, 70, m.gc.data(), m.mi.data(), m.iv.data(), 4, gs.data(), nullptr) == -5);
    CHECK(mfa_debug_ubm_gselect_host(x.data(), 1, 4, 70, m.gc.data(), m.mi.data(), m.iv.data(), 4, nullptr, nullptr) == -1);
    CHECK(mfa_debug_ubm_acc_host(x.data(), 1, 4, 70, m.gc.data(), m.mi.data(), m.iv.data(), 4, gs.data(), nullptr, nullptr, a.mean.data(),
                                 a.var.data(), a.tot.data(), nullptr) == -1);
    CHECK(a.tot[1] == 0.0);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
