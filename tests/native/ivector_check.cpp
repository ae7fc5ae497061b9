// The host twins of the i-vector extractor stage (csrc/ivector_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_ivector_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: the limits (dim 48, lists of 64, R = 192 once), empty utterances, indices outside
// the model, NaN features and posteriors, pruning in place, max_count, extraction and accumulation, empty calls, the refusals.
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
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

struct Stats {
  std::vector<double> gamma, X, S;
};

// U utterances of the given lengths, lists of n entries (every tenth outside the model), G Gaussians
static Stats utt_stats(int dim, int G, int n, const std::vector<int64_t> &off, bool with_S, double max_count, bool poison, int *rc) {
  const int U = (int)off.size() - 1;
  const int64_t T = off.back();
  uint32_t s = 7u + (uint32_t)dim * 131u + (uint32_t)G;
  std::vector<float> x((size_t)T * dim), post((size_t)T * n);
  std::vector<int32_t> gs((size_t)T * n);
  for (auto &v : x) v = 4.0f * unit(s) - 2.0f;
  for (size_t i = 0; i < gs.size(); i++) {
    gs[i] = i % 10 == 9 ? G + (int32_t)(i % 3) - 1 + (i % 2 ? 1 : -G - 1) : (int32_t)(lcg(s) % (uint32_t)G);
    post[i] = unit(s);
  }
  if (poison && T > 2) {
    x[dim] = std::numeric_limits<float>::quiet_NaN();
    x[2 * dim] = std::numeric_limits<float>::infinity();
    post[1] = std::numeric_limits<float>::quiet_NaN();
  }
  Stats st{std::vector<double>((size_t)U * G), std::vector<double>((size_t)U * G * dim),
           std::vector<double>(with_S ? (size_t)G * dim * (dim + 1) / 2 : 0, 0.0)};
  *rc = mfa_debug_ivector_utt_stats_host(x.empty() ? nullptr : x.data(), off.data(), U, dim, G, n, gs.empty() ? nullptr : gs.data(),
                                         post.empty() ? nullptr : post.data(), max_count, st.gamma.data(), st.X.data(),
                                         with_S ? st.S.data() : nullptr);
  return st;
}

static void estep(int dim, int G, int R, const Stats &st, int U, bool acc, bool want_var) {
  const int P = R * (R + 1) / 2;
  uint32_t s = 99u + (uint32_t)R;
  // a valid model: M random, SigmaInv = I, so W = M and U_g = M^T M
  std::vector<double> W((size_t)G * dim * R), Um((size_t)G * P, 0.0);
  for (auto &v : W) v = (double)unit(s) - 0.5;
  for (int g = 0; g < G; g++)
    for (int r = 0; r < R; r++)
      for (int c = 0; c <= r; c++) {
        double a = 0.0;
        for (int k = 0; k < dim; k++) a += W[((size_t)g * dim + k) * R + r] * W[((size_t)g * dim + k) * R + c];
        Um[(size_t)g * P + r * (r + 1) / 2 + c] = a;
      }
  std::vector<double> mean((size_t)U * R), var(want_var ? (size_t)U * P : 0), aux((size_t)U * 2);
  std::vector<double> Gam(G, 0.0), Y((size_t)G * dim * R, 0.0), Rq((size_t)G * P, 0.0), isum(R, 0.0), iscat(P, 0.0), n(1, 0.0);
  const int rc = mfa_debug_ivector_estep_host(st.gamma.data(), st.X.data(), U, dim, G, R, W.data(), Um.data(), 10.0, mean.data(),
                                              want_var ? var.data() : nullptr, aux.data(), acc ? Gam.data() : nullptr,
                                              acc ? Y.data() : nullptr, acc ? Rq.data() : nullptr, acc ? isum.data() : nullptr,
                                              acc ? iscat.data() : nullptr, acc ? n.data() : nullptr);
  CHECK(rc == 0);
  if (acc) CHECK(n[0] >= 0.0 && n[0] <= (double)U);
}

int main() {
  int rc = 0;
  // pruning: out of place, in place, the hand cases
  {
    std::vector<float> p = {0.01f, 0.02f, 0.005f, 0.5f, 0.5f, 0.0f, 0.025f, 0.9f, 0.075f, 0.0f, 0.0f, 0.0f};
    std::vector<float> out(p.size());
    CHECK(mfa_debug_ivector_prune_post_host(p.data(), 4, 3, 0.025f, 1.0f, out.data()) == 0);
    CHECK(out[0] == 0.0f && out[1] == 1.0f && out[2] == 0.0f);
    CHECK(out[3] == 0.5f && out[4] == 0.5f && out[5] == 0.0f);
    CHECK(out[6] > 0.0f && out[9] == 0.0f && out[10] == 0.0f && out[11] == 0.0f);
    std::vector<float> in_place = p;
    CHECK(mfa_debug_ivector_prune_post_host(in_place.data(), 4, 3, 0.025f, 1.0f, in_place.data()) == 0);
    CHECK(in_place == out);
    std::vector<float> wide(64 * 5);
    uint32_t s = 3;
    for (auto &v : wide) v = unit(s) / 32.0f;
    wide[70] = std::numeric_limits<float>::quiet_NaN();
    CHECK(mfa_debug_ivector_prune_post_host(wide.data(), 5, 64, 0.025f, 5.0f, wide.data()) == 0);
    CHECK(mfa_debug_ivector_prune_post_host(nullptr, 0, 3, 0.025f, 1.0f, nullptr) == 0);
    CHECK(mfa_debug_ivector_prune_post_host(p.data(), 4, 0, 0.025f, 1.0f, out.data()) == -4);
    CHECK(mfa_debug_ivector_prune_post_host(p.data(), 4, 65, 0.025f, 1.0f, out.data()) == -4);
    CHECK(mfa_debug_ivector_prune_post_host(p.data(), 4, 3, 0.025f, 1.0f, nullptr) == -1);
    CHECK(mfa_debug_ivector_prune_post_host(p.data(), (int64_t)1 << 31, 3, 0.025f, 1.0f, out.data()) == -5);
  }
  // statistics and E-step at the limits and at odd shapes
  const std::vector<int64_t> off = {0, 0, 1, 64, 128, 193, 193, 393};
  const int U = (int)off.size() - 1;
  {
    Stats st = utt_stats(48, 70, 64, off, true, 0.0, true, &rc);
    CHECK(rc == 0);
    for (int g = 0; g < 70; g++) CHECK(st.gamma[g] == 0.0);                 // the empty utterance
    estep(48, 70, 5, st, U, true, true);
    estep(48, 70, 17, st, U, false, false);
  }
  {
    Stats st = utt_stats(3, 4, 2, off, true, 10.0, false, &rc);
    CHECK(rc == 0);
    for (int u = 0; u < U; u++) {
      double tot = 0.0;
      for (int g = 0; g < 4; g++) tot += st.gamma[(size_t)u * 4 + g];
      CHECK(tot <= 10.0 * (1.0 + 1e-12));
    }
    estep(3, 4, 192, st, 3, true, true);
    estep(3, 4, 1, st, U, true, true);
  }
  {
    Stats st = utt_stats(13, 2048, 1, off, false, 0.0, false, &rc);
    CHECK(rc == 0);
  }
  // empty calls and refusals
  {
    const std::vector<int64_t> none = {0};
    double d[8] = {0};
    float f[8] = {0};
    int32_t g[8] = {0};
    const int64_t one[2] = {0, 1}, bad[2] = {1, 2}, back[3] = {0, 2, 1};
    CHECK(mfa_debug_ivector_utt_stats_host(nullptr, none.data(), 0, 3, 4, 2, nullptr, nullptr, 0.0, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 0, 4, 2, g, f, 0.0, d, d, nullptr) == -2);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 49, 4, 2, g, f, 0.0, d, d, nullptr) == -2);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 1, 0, 2, g, f, 0.0, d, d, nullptr) == -3);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 1, 2049, 2, g, f, 0.0, d, d, nullptr) == -3);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 1, 4, 0, g, f, 0.0, d, d, nullptr) == -4);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 1, 4, 65, g, f, 0.0, d, d, nullptr) == -4);
    CHECK(mfa_debug_ivector_utt_stats_host(f, one, 1, 1, 4, 2, g, f, 0.0, nullptr, d, nullptr) == -1);
    CHECK(mfa_debug_ivector_utt_stats_host(nullptr, one, 1, 1, 4, 2, g, f, 0.0, d, d, nullptr) == -1);
    CHECK(mfa_debug_ivector_utt_stats_host(f, bad, 1, 1, 4, 2, g, f, 0.0, d, d, nullptr) == -1);
    CHECK(mfa_debug_ivector_utt_stats_host(f, back, 2, 1, 4, 2, g, f, 0.0, d, d, nullptr) == -1);
    CHECK(mfa_debug_ivector_estep_host(nullptr, nullptr, 0, 3, 4, 2, nullptr, nullptr, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_ivector_estep_host(d, d, 1, 1, 1, 0, d, d, 1.0, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == -6);
    CHECK(mfa_debug_ivector_estep_host(d, d, 1, 1, 1, 193, d, d, 1.0, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == -6);
    CHECK(mfa_debug_ivector_estep_host(d, d, 1, 1, 1, 1, d, d, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == -1);
    CHECK(mfa_debug_ivector_estep_host(d, d, 1, 1, 1, 1, d, d, 1.0, d, nullptr, nullptr, d, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == -1);                     // some but not all accumulators
    CHECK(mfa_debug_ivector_estep_host(d, d, 1, 1, 1, 1, d, d, 1.0, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr) == 0);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures == 0 ? 0 : 1;
}
