// The host twin of the tree statistics (csrc/tree_acc_host.cpp) as a stand-alone program for the host sanitizers:
// tests/test_tree_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized exactly, so an
// index past an end is a report.  Inputs: utterances of 0, 1, 2, 63, 64, 65 and 129 frames, one-frame phones, ids outside the
// table, an unfinished utterance, a phone change inside a segment, every row count from 0 to the number of events, an empty
// call, the refusals.  Phones have one state: id 2p - 1 is phone p's self-loop, id 2p its final arc, which comes first
// (reordered alignments); the pdf-class is p % 3.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mfa_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Batch {
  int dim, n_phones, n_tids;
  std::vector<int64_t> fo;
  std::vector<float> x;
  std::vector<int32_t> ali, phone, cls, fin;
  std::vector<uint8_t> ci;
};

static Batch make(int dim, int n_phones, const std::vector<int> &lengths, uint32_t seed) {
  Batch b;
  b.dim = dim; b.n_phones = n_phones; b.n_tids = 2 * n_phones + 1;
  b.phone.assign(b.n_tids, 0); b.cls.assign(b.n_tids, 0); b.fin.assign(b.n_tids, 0);
  for (int p = 1; p <= n_phones; p++)
    for (int k = 0; k < 2; k++) { b.phone[2 * p - 1 + k] = p; b.cls[2 * p - 1 + k] = p % 3; b.fin[2 * p - 1 + k] = k ? 1 : 2; }
  b.ci.assign(n_phones + 1, 0);
  b.ci[1] = 1;
  b.fo.push_back(0);
  for (int n : lengths) {
    int left = n;
    while (left > 0) {
      const int p = 1 + (int)(lcg(seed) >> 16) % n_phones;
      int d = 1 + (int)(lcg(seed) >> 16) % 5;
      if (d > left) d = left;
      b.ali.push_back(2 * p);
      for (int i = 0; i + 1 < d; i++) b.ali.push_back(2 * p - 1);
      left -= d;
    }
    b.fo.push_back(b.fo.back() + n);
  }
  b.x.resize((size_t)b.fo.back() * dim);
  for (auto &v : b.x) v = (float)((int)(lcg(seed) >> 24) % 17 - 8);          // integers in [-8, 8]
  return b;
}

struct Out {
  std::vector<int32_t> fe;
  int64_t n_events = -1, skipped = -1;
  std::vector<uint64_t> key;
  std::vector<int64_t> count;
  std::vector<double> sum, sumsq;
};

static int run(const Batch &b, int64_t cap, Out &o) {
  const int64_t T = b.fo.back();
  o.fe.assign((size_t)T, -7);
  o.key.assign((size_t)cap, 0); o.count.assign((size_t)cap, -1);
  o.sum.assign((size_t)cap * b.dim, -1.0); o.sumsq.assign((size_t)cap * b.dim, -1.0);
  return mfa_debug_tree_acc_host(b.x.data(), b.fo.data(), (int32_t)b.fo.size() - 1, b.dim, b.ali.data(), b.phone.data(), b.cls.data(),
                                 b.fin.data(), b.n_tids, b.ci.data(), b.n_phones, cap, o.fe.data(), &o.n_events, &o.skipped,
                                 o.key.data(), o.count.data(), o.sum.data(), o.sumsq.data());
}

// the rows against sums formed from frame_event
static void check_rows(const Batch &b, const Out &o) {
  const int64_t T = b.fo.back(), E = o.n_events;
  std::vector<int64_t> n((size_t)E, 0);
  std::vector<double> s((size_t)E * b.dim, 0.0), q((size_t)E * b.dim, 0.0);
  for (int64_t t = 0; t < T; t++) {
    const int e = o.fe[(size_t)t];
    CHECK(e >= -1 && e < E);
    if (e < 0) continue;
    n[e]++;
    for (int k = 0; k < b.dim; k++) {
      const double v = b.x[(size_t)t * b.dim + k];
      s[(size_t)e * b.dim + k] += v; q[(size_t)e * b.dim + k] += v * v;
    }
    const int p = b.phone[b.ali[(size_t)t]];
    CHECK((int)((o.key[e] >> 28) & 0xFFFFF) == p && (int)(o.key[e] & 0xFF) == p % 3);
    if (p == 1) CHECK((o.key[e] >> 48) == 0 && ((o.key[e] >> 8) & 0xFFFFF) == 0);
  }
  for (int64_t e = 0; e < E; e++) {
    CHECK(n[e] == o.count[e] && n[e] > 0);
    if (e) CHECK(o.key[e - 1] < o.key[e]);
    for (int k = 0; k < b.dim; k++) CHECK(s[(size_t)e * b.dim + k] == o.sum[(size_t)e * b.dim + k] && q[(size_t)e * b.dim + k] == o.sumsq[(size_t)e * b.dim + k]);
  }
}

int main() {
  const std::vector<int> lengths = {0, 1, 2, 63, 64, 65, 0, 129, 300};
  for (int dim : {1, 13, 48}) {
    Batch b = make(dim, 7, lengths, 17u + dim);
    Out full;
    CHECK(run(b, b.fo.back(), full) == 0);
    CHECK(full.skipped == 0 && full.n_events > 7);
    check_rows(b, full);
    for (int64_t cap : {(int64_t)0, full.n_events - 1, full.n_events}) {
      Out o;
      CHECK(run(b, cap, o) == 0);
      CHECK(o.n_events == full.n_events && o.fe == full.fe);
      if (cap < full.n_events) { for (auto c : o.count) CHECK(c == -1); }      // no row written
      else check_rows(b, o);
    }
    // utterances that take no part: an id outside the table, an id 0, an unfinished last phone, a phone change in a segment
    Batch bad = b;
    bad.ali[(size_t)bad.fo[3] + 5] = bad.n_tids;          // the 63-frame utterance
    bad.ali[(size_t)bad.fo[4] + 9] = 0;                   // the 64-frame utterance
    for (int64_t t = bad.fo[5]; t < bad.fo[6]; t++) bad.ali[(size_t)t] = 1;   // the 65-frame utterance: self-loops, no final id
    {
      size_t t = (size_t)bad.fo[7];                        // the 129-frame utterance: a segment of two phones
      bad.ali[t] = 1; bad.ali[t + 1] = 4; bad.ali[t + 2] = 3;
    }
    Out o;
    CHECK(run(bad, bad.fo.back(), o) == 0);
    CHECK(o.skipped == 4);
    for (int u : {3, 4, 5, 7})
      for (int64_t t = bad.fo[u]; t < bad.fo[u + 1]; t++) CHECK(o.fe[(size_t)t] == -1);
    check_rows(bad, o);
  }
  {
    Batch b = make(5, 3, {}, 1u);                          // no utterance
    Out o;
    CHECK(run(b, 4, o) == 0 && o.n_events == 0 && o.skipped == 0);
    Batch z = make(5, 3, {0, 0}, 1u);                      // utterances, no frame
    CHECK(run(z, 0, o) == 0 && o.n_events == 0 && o.skipped == 0);
  }
  {
    Batch b = make(49, 3, {10}, 3u);
    Out o;
    CHECK(run(b, 10, o) == -2);
    Batch c = make(4, 3, {10}, 3u);
    c.n_phones = 1 << 16;
    c.ci.assign((size_t)c.n_phones + 1, 0);
    CHECK(run(c, 10, o) == -4);
    Batch d = make(4, 3, {10}, 3u);
    int64_t ne, sk;
    CHECK(mfa_debug_tree_acc_host(d.x.data(), d.fo.data(), 1, 4, nullptr, d.phone.data(), d.cls.data(), d.fin.data(), d.n_tids,
                                  d.ci.data(), 3, 0, nullptr, &ne, &sk, nullptr, nullptr, nullptr, nullptr) == -1);
    Batch e = make(4, 3, {10, 5}, 3u);
    e.fo[1] = 16;                                          // offsets that do not ascend
    CHECK(run(e, 10, o) == -1);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures ? 1 : 0;
}
