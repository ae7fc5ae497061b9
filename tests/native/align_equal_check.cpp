// The host twin of the equal alignment (csrc/align_equal_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_align_equal_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly,
// so an index past an end is a report.  Inputs: an empty batch, utterances of 0 frames, a chain that cannot loop, a walk that
// is cut by its step bound (an epsilon cycle), a dead end, random graphs with loops and epsilon arcs at many lengths,
// malformed graphs (a next state, an arc range, a start state outside the graph), the refusals.
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

struct Batch {
  std::vector<int64_t> state_off{0}, arc_base{0}, frame_off{0};
  std::vector<int32_t> start, arc_off, next, ilabel;
  std::vector<float> final_cost;
  std::vector<uint32_t> key;

  // arcs: per state a list of (ilabel, next)
  void add(const std::vector<std::vector<std::pair<int32_t, int32_t>>> &states, const std::vector<int> &finals, int32_t st,
           int64_t T, uint32_t k) {
    int32_t a = 0;
    for (const auto &s : states) {
      arc_off.push_back(a);
      for (const auto &arc : s) { ilabel.push_back(arc.first); next.push_back(arc.second); a++; }
    }
    arc_off.push_back(a);
    const size_t f0 = final_cost.size();
    final_cost.resize(f0 + states.size(), INFINITY);
    for (int f : finals) final_cost[f0 + f] = 0.0f;
    state_off.push_back(state_off.back() + (int64_t)states.size());
    arc_base.push_back(arc_base.back() + a);
    frame_off.push_back(frame_off.back() + T);
    start.push_back(st);
    key.push_back(k);
  }
  int n() const { return (int)start.size(); }
  int run(uint32_t seed, std::vector<int32_t> &ali, std::vector<int32_t> &status) const {
    ali.assign((size_t)frame_off.back(), -7);
    status.assign(start.size(), -7);
    return mfa_debug_align_equal_host(n(), state_off.data(), arc_base.data(), start.data(), arc_off.data(), final_cost.data(),
                                      next.empty() ? nullptr : next.data(), ilabel.empty() ? nullptr : ilabel.data(),
                                      frame_off.data(), key.data(), seed, ali.empty() ? nullptr : ali.data(), status.data());
  }
};

using States = std::vector<std::vector<std::pair<int32_t, int32_t>>>;

// a left-to-right graph of n states: every state but the last has one or two forward arcs (to s + 1, sometimes s + 2, some of
// them epsilon) and, mostly, a labelled loop; the last state is final
static States random_graph(int n, uint32_t &seed) {
  States g((size_t)n);
  for (int s = 0; s + 1 < n; s++) {
    if (lcg(seed) >> 30) g[s].push_back({1000 + s, s});
    g[s].push_back({(lcg(seed) >> 29) == 0 ? 0 : 1 + 2 * s, s + 1});
    if (s + 2 < n && (lcg(seed) >> 31)) g[s].push_back({2 + 2 * s, s + 2});
  }
  return g;
}

int main() {
  std::vector<int32_t> ali, status;
  CHECK(mfa_debug_align_equal_host(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1u,
                                   nullptr, nullptr) == 0);
  CHECK(mfa_debug_align_equal_host(2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1u,
                                   nullptr, nullptr) == -1);
  {
    Batch b;
    const States chain = {{{5, 1}}, {{6, 2}}, {{7, 3}}, {}};
    b.add(chain, {3}, 0, 3, 0);                       // ok: exactly its labels
    b.add(chain, {3}, 0, 4, 1);                       // nothing can loop
    b.add(chain, {3}, 0, 2, 2);                       // one below the shortest path
    b.add(chain, {3}, 0, 0, 3);                       // no frames, labels to emit
    b.add({{{9, 0}}}, {0}, 0, 0, 4);                  // no frames, a final start state: ok, nothing written
    b.add({{{9, 0}}}, {0}, 0, 5, 5);                  // the only state loops five times
    b.add({{{0, 1}}, {{0, 0}, {3, 1}}, {}}, {2}, 0, 6, 6);   // epsilon cycle: cut by the step bound
    b.add({{{1, 1}}, {{2, 1}}, {}}, {2}, 0, 6, 7);    // dead end
    b.add({{{1, 1}}, {}}, {1}, 0, 1, 8);              // a single arc
    CHECK(b.run(99u, ali, status) == 0);
    const int want[] = {0, 2, 2, 2, 0, 0, 2, 2, 0};
    for (int u = 0; u < b.n(); u++) CHECK(status[u] == want[u]);
    CHECK(ali[0] == 5 && ali[1] == 6 && ali[2] == 7);
    for (int64_t t = b.frame_off[1]; t < b.frame_off[4]; t++) CHECK(ali[t] == 0);
    for (int64_t t = b.frame_off[5]; t < b.frame_off[6]; t++) CHECK(ali[t] == 9);
    for (int64_t t = b.frame_off[6]; t < b.frame_off[8]; t++) CHECK(ali[t] == 0);
    CHECK(ali[b.frame_off[8]] == 1);
  }
  {  // random graphs at many lengths: a success fills every frame, a failure zeroes them; the same bits in another batch
    uint32_t seed = 4242u;
    Batch b;
    std::vector<States> graphs;
    std::vector<int> sizes, lens;
    for (int i = 0; i < 60; i++) {
      const int n = 2 + (int)(lcg(seed) >> 27);
      graphs.push_back(random_graph(n, seed));
      sizes.push_back(n);
      lens.push_back((int)(lcg(seed) >> 24) % (i % 3 == 0 ? 8 : 200));
      b.add(graphs.back(), {n - 1}, 0, lens.back(), 1000u + (uint32_t)i);
    }
    CHECK(b.run(7u, ali, status) == 0);
    int ok = 0;
    for (int u = 0; u < b.n(); u++) {
      CHECK(status[u] == 0 || status[u] == 2);
      ok += status[u] == 0;
      for (int64_t t = b.frame_off[u]; t < b.frame_off[u + 1]; t++) CHECK(status[u] == 0 ? ali[t] > 0 : ali[t] == 0);
    }
    CHECK(ok > 10 && ok < b.n());
    Batch r;
    for (int i = 59; i >= 0; i--) r.add(graphs[i], {sizes[i] - 1}, 0, lens[i], 1000u + (uint32_t)i);
    std::vector<int32_t> ali_r, status_r;
    CHECK(r.run(7u, ali_r, status_r) == 0);
    for (int i = 0; i < 60; i++) {
      CHECK(status_r[59 - i] == status[i]);
      for (int t = 0; t < lens[i]; t++) CHECK(ali_r[r.frame_off[59 - i] + t] == ali[b.frame_off[i] + t]);
    }
  }
  {  // malformed graphs fail their utterance and touch nothing outside it
    Batch b;
    b.add({{{1, 5}}, {}}, {1}, 0, 3, 0);              // next state outside the graph
    b.add({{{1, 1}}, {}}, {1}, 2, 3, 1);              // start state outside the graph
    b.add({{{1, -1}}, {}}, {1}, 0, 3, 2);             // negative next state
    b.add({{{1, 1}}, {}}, {1}, 0, 1, 3);
    b.add({{{1, 1}}, {}}, {1}, 0, 2, 4);
    b.arc_off[(size_t)b.state_off[4] + 4 + 1] = 9;    // the last utterance's first state claims arcs it does not have
    CHECK(b.run(3u, ali, status) == 0);
    CHECK(status[0] == 2 && status[1] == 2 && status[2] == 2 && status[3] == 0 && status[4] == 2);
    for (int64_t t = 0; t < 9; t++) CHECK(ali[t] == 0);
    CHECK(ali[9] == 1 && ali[10] == 0 && ali[11] == 0);
  }
  {  // 2^31 frames: refused before anything is read
    const int64_t so[2] = {0, 1}, ab[2] = {0, 0}, fo[2] = {0, (int64_t)1 << 31};
    const int32_t st = 0, ao[2] = {0, 0};
    const float fin = 0.0f;
    const uint32_t key = 0;
    int32_t status1 = -7;
    CHECK(mfa_debug_align_equal_host(1, so, ab, &st, ao, &fin, nullptr, nullptr, fo, &key, 0u, nullptr, &status1) == -2);
    CHECK(status1 == -7);
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
