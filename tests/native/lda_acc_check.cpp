// The host twin of the LDA statistics (csrc/lda_acc_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_lda_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: utterances of 1, 2, ctx and ctx + 1 frames (every splice row clamps), an empty
// utterance between them, spliced dimensions 15, 91 and 128, CMVN on and off, pruning on and off, ids outside the table,
// an empty call, the refusals.
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

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

struct Batch {
  int dim, ctx, C, n_tids;
  std::vector<int64_t> fo;
  std::vector<float> x, tw;
  std::vector<int32_t> ali, t2c, u2s;
  std::vector<double> cmvn;
  std::vector<uint32_t> keys;
  int S() const { return (2 * ctx + 1) * dim; }
};

static Batch make(int dim, int ctx, const std::vector<int> &lengths, int C, uint32_t seed) {
  Batch b;
  b.dim = dim; b.ctx = ctx; b.C = C; b.n_tids = 2 * C + 1;
  b.fo.push_back(0);
  for (int n : lengths) b.fo.push_back(b.fo.back() + n);
  const int64_t T = b.fo.back();
  b.x.resize((size_t)T * dim);
  for (auto &v : b.x) v = (float)((int)(lcg(seed) >> 24) % 17 - 8);          // integers in [-8, 8]
  b.ali.resize((size_t)T);
  for (auto &a : b.ali) a = (int)(lcg(seed) >> 16) % (b.n_tids + 4) - 2;       // some outside [1, n_tids)
  b.t2c.resize(b.n_tids); b.tw.resize(b.n_tids);
  for (int i = 0; i < b.n_tids; i++) {
    b.t2c[i] = i == 0 ? 0 : (i - 1) / 2;
    b.tw[i] = i % 5 == 0 ? 0.0f : (i % 2 ? 1.0f : 0.5f);
  }
  b.t2c[b.n_tids - 1] = C;                                                     // a class outside [0, C)
  const int n_utt = (int)lengths.size(), n_spk = 2;
  b.u2s.resize(n_utt); b.keys.resize(n_utt);
  for (int u = 0; u < n_utt; u++) { b.u2s[u] = u % n_spk; b.keys[u] = 1000u + (uint32_t)u; }
  b.cmvn.assign((size_t)n_spk * 2 * (dim + 1), 0.0);
  for (int s = 0; s < n_spk; s++) {
    for (int d = 0; d < dim; d++) b.cmvn[(size_t)s * 2 * (dim + 1) + d] = 8.0 * (double)(d % 3 - 1 + s);   // mean: an integer
    b.cmvn[(size_t)s * 2 * (dim + 1) + dim] = 8.0;
  }
  return b;
}

struct Acc {
  std::vector<double> zero, first, second;
  std::vector<int64_t> cnt;
  Acc(const Batch &b) : zero(b.C, 0.0), first((size_t)b.C * b.S(), 0.0), second((size_t)b.S() * b.S(), 0.0), cnt(b.n_tids, 0) {}
};

static int run(const Batch &b, bool cmvn, float theta, Acc &a, bool counts = true) {
  return mfa_debug_lda_acc_host(b.x.empty() ? nullptr : b.x.data(), b.fo.data(), (int32_t)b.fo.size() - 1, b.dim,
                                cmvn ? b.u2s.data() : nullptr, cmvn ? b.cmvn.data() : nullptr, b.ctx,
                                b.ali.empty() ? nullptr : b.ali.data(), b.t2c.data(), b.tw.data(), b.n_tids, b.C, theta,
                                theta > 0.0f ? b.keys.data() : nullptr, 77u, a.zero.data(), a.first.data(), a.second.data(),
                                counts ? a.cnt.data() : nullptr);
}

static void check_shape(int dim, int ctx, uint32_t seed) {
  const std::vector<int> lengths = {1, 2, 0, ctx > 0 ? ctx : 1, ctx + 1, 37};
  const Batch b = make(dim, ctx, lengths, 5, seed);
  const int S = b.S();
  for (int cm = 0; cm < 2; cm++) {
    Acc a(b);
    CHECK(run(b, cm != 0, 0.0f, a) == 0);
    // Σ_c zero = the summed weights of the frames that take part; the counts are their number
    double wsum = 0.0, zsum = 0.0;
    int64_t n = 0, counted = 0;
    for (size_t t = 0; t < b.ali.size(); t++) {
      const int id = b.ali[t];
      if (id <= 0 || id >= b.n_tids || b.tw[id] == 0.0f || b.t2c[id] >= b.C) continue;
      wsum += (double)b.tw[id]; n++;
    }
    for (double z : a.zero) zsum += z;
    for (int64_t c : a.cnt) counted += c;
    CHECK(zsum == wsum && counted == n && n > 0);
    // symmetric to the bit, a non-negative diagonal whose trace is Σ w·|x|² (exact here: integers)
    for (int i = 0; i < S; i++) {
      CHECK(a.second[(size_t)i * S + i] >= 0.0);
      for (int j = 0; j < i; j++) CHECK(a.second[(size_t)i * S + j] == a.second[(size_t)j * S + i]);
    }
    // a second call adds the same again (integers: exact)
    Acc twice = a;
    CHECK(run(b, cm != 0, 0.0f, twice) == 0);
    for (size_t k = 0; k < a.second.size(); k++) CHECK(twice.second[k] == 2.0 * a.second[k]);
    for (size_t k = 0; k < a.first.size(); k++) CHECK(twice.first[k] == 2.0 * a.first[k]);
    // pruned at theta = 4: every frame that stays weighs 4
    Acc p(b);
    CHECK(run(b, cm != 0, 4.0f, p, false) == 0);
    for (double z : p.zero) CHECK(std::fmod(z, 4.0) == 0.0);
  }
}

int main() {
  check_shape(5, 1, 3u);       // S = 15
  check_shape(13, 3, 5u);      // S = 91
  check_shape(128, 0, 7u);     // S = 128, no splice
  check_shape(8, 7, 9u);       // S = 120, a context longer than most utterances
  {  // one frame, by hand: x = (2, -3), ctx 1 → (2, -3, 2, -3, 2, -3), weight ½
    Batch b = make(2, 1, {1}, 1, 1u);
    b.x = {2.0f, -3.0f}; b.ali = {1}; b.tw[1] = 0.5f;
    Acc a(b);
    CHECK(run(b, false, 0.0f, a) == 0);
    CHECK(a.zero[0] == 0.5 && a.first[0] == 1.0 && a.first[5] == -1.5 && a.cnt[1] == 1);
    CHECK(a.second[0] == 2.0 && a.second[1] == -3.0 && a.second[6 * 1 + 0] == -3.0 && a.second[6 * 5 + 5] == 4.5);
  }
  {  // empty input: nothing is read, nothing is written
    Batch b = make(13, 3, {0, 0}, 3, 1u);
    Acc a(b);
    a.zero[1] = 1.5;
    CHECK(run(b, false, 0.0f, a) == 0);
    CHECK(a.zero[1] == 1.5 && a.second[0] == 0.0);
  }
  {  // refusals
    Batch b = make(43, 1, {3}, 2, 1u);              // S = 129
    std::vector<double> z(2), f((size_t)2 * 129), s((size_t)129 * 129);
    CHECK(mfa_debug_lda_acc_host(b.x.data(), b.fo.data(), 1, 43, nullptr, nullptr, 1, b.ali.data(), b.t2c.data(), b.tw.data(), b.n_tids,
                                 2, 0.0f, nullptr, 0u, z.data(), f.data(), s.data(), nullptr) == -2);
    Batch c = make(4, 1, {3}, 2, 1u);
    Acc a(c);
    CHECK(mfa_debug_lda_acc_host(c.x.data(), c.fo.data(), 1, 0, nullptr, nullptr, 1, c.ali.data(), c.t2c.data(), c.tw.data(), c.n_tids,
                                 2, 0.0f, nullptr, 0u, a.zero.data(), a.first.data(), a.second.data(), nullptr) == -1);
    CHECK(mfa_debug_lda_acc_host(c.x.data(), c.fo.data(), 1, 4, nullptr, nullptr, 1, c.ali.data(), c.t2c.data(), c.tw.data(), c.n_tids,
                                 0, 0.0f, nullptr, 0u, a.zero.data(), a.first.data(), a.second.data(), nullptr) == -1);
    CHECK(run(c, false, 0.0f, a) == 0);
    CHECK(mfa_debug_lda_acc_host(c.x.data(), c.fo.data(), 1, 4, nullptr, c.cmvn.data(), 1, c.ali.data(), c.t2c.data(), c.tw.data(),
                                 c.n_tids, 2, 0.0f, nullptr, 0u, a.zero.data(), a.first.data(), a.second.data(), nullptr) == -1);
    CHECK(mfa_debug_lda_acc_host(c.x.data(), c.fo.data(), 1, 4, nullptr, nullptr, 1, c.ali.data(), c.t2c.data(), c.tw.data(), c.n_tids,
                                 2, 4.0f, nullptr, 0u, a.zero.data(), a.first.data(), a.second.data(), nullptr) == -1);
    CHECK(mfa_debug_lda_acc_host(c.x.data(), c.fo.data(), 1, 4, nullptr, nullptr, 1, c.ali.data(), c.t2c.data(), c.tw.data(), c.n_tids,
                                 2, 0.0f, nullptr, 0u, a.zero.data(), a.first.data(), nullptr, nullptr) == -1);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
