// Host check of csrc/viterbi_plan.hpp: the wavefront decoder's launch plan swept over graph sizes, capacities and modes.
// Built and run by tests/test_viterbi_plan_cpu.py with the address and undefined-behaviour sanitizers; exit status 0 means
// every check held.  It prints what it measured (the tier thresholds, the reach of two suspected-dead branches).
//
// Sweep: max_states 1 … 20 000 (every value); max_tokens in {0, 64, 256, 512, 1024, 4096, max_states}; epsilon arcs or
// not; dense or lazy; with a retry beam (without one the plan is the same less its last launch: tried at one density).
// max_arcs runs from 1 to 8 × max_states.  The plan sees it only through the candidate capacity
// C = max(256, ceil64(min(k·N, max_arcs))), so it is stepped in multiples of 64 — up to sixteen of them per size, the stride
// growing with the size — plus the edges 1, 255 … 257, 3.8 × max_states (the fuzz graphs' density) and 8 × max_states.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../montreal_forced_aligner_amd/csrc/viterbi_plan.hpp"

namespace {

long failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      if (failures < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
      failures++;                                                           \
    }                                                                       \
  } while (0)

int ceil64(int v) { return (v + 63) & ~63; }

// The capacities asked for, restated independently of the header: max_tokens (1024 by default; four times that for the
// retry beam), at most one token per state, in 64s; four (retry: eight) candidates per token, at most one per arc.
void asked(const mfa_align_opts &o, int S, int A, int pass, int *N, int *C) {
  long n = o.max_tokens > 0 ? o.max_tokens : 1024;
  if (pass == 1) n *= 4;
  if (n > S) n = S;
  n = ceil64((int)n);
  if (n < 64) n = 64;
  long c = (pass == 1 ? 8 : 4) * n;
  if (c > A) c = A;
  c = ceil64((int)c);
  if (c < 256) c = 256;
  *N = (int)n; *C = (int)c;
}

struct Reach {
  long plans = 0, launches = 0, refused = 0, half_limit_decides = 0, hbm = 0, shrunk = 0, hashed = 0,
       lists_would_fit_after_shrink = 0;
};

void check_plan(const mfa_align_opts &o, int S, int A, bool eps, bool lazy, Reach &r) {
  const vplan::Plan pl = vplan::viterbi_plan(&o, S, A, eps, lazy);
  r.plans++;
  // the exported rows say the same
  int32_t rows[7 * vplan::kMaxLaunches];
  const int n_rows = vplan::viterbi_plan_rows(&o, S, A, eps, lazy, rows, vplan::kMaxLaunches);
  if (pl.refused >= 0) {
    r.refused++;
    CHECK(n_rows == -1, "S=%d A=%d: refused plan, rows returned %d", S, A, n_rows);
    return;
  }
  CHECK(n_rows == pl.n, "S=%d A=%d: %d launches, rows returned %d", S, A, pl.n, n_rows);
  const int passes = o.retry_beam != 0.0f ? 2 : 1;
  int N0, C0, N1, C1;
  asked(o, S, A, 0, &N0, &C0);
  asked(o, S, A, 1, &N1, &C1);
  const int first = lazy ? 64 : 128;
  const int want_n = (N0 > first ? 2 : 1) + (passes == 2 ? 1 : 0);
  CHECK(pl.n == want_n, "S=%d A=%d mt=%d: %d launches, expected %d", S, A, o.max_tokens, pl.n, want_n);
  for (int i = 0; i < pl.n; i++) {
    const vplan::Launch &L = pl.l[i];
    r.launches++;
    const int32_t *row = rows + 7 * i;
    CHECK(row[0] == L.pass && row[1] == L.code && row[2] == L.N && row[3] == L.C && row[4] == (int32_t)L.lds &&
          row[5] == (int)L.lists_in_lds && row[6] == L.hbits, "S=%d A=%d launch %d: row differs from the plan", S, A, i);
    // which launch this is, and the capacities it was asked for
    int aN, aC;
    if (L.pass == 1) { aN = N1; aC = C1; CHECK(L.code == vplan::kCodePending && i == pl.n - 1, "S=%d: retry launch %d code %d", S, i, L.code); }
    else if (L.grow) { aN = first; aC = C0 < 4 * first ? C0 : 4 * first; CHECK(i == 0 && L.code == 0, "S=%d: first tier at %d", S, i); }
    else { aN = N0; aC = C0; CHECK(L.code == (N0 > first ? vplan::kCodeGrow : 0), "S=%d: pass-0 launch %d code %d", S, i, L.code); }
    CHECK(L.lds <= vplan::kLdsLimit, "S=%d A=%d launch %d: %zu bytes of LDS", S, A, i, L.lds);
    CHECK(L.lds == vplan::lds_bytes(S, L.N, L.C, L.lists_in_lds, eps), "S=%d launch %d: lds is not the carve of its own row", S, i);
    CHECK(L.N % 64 == 0 && L.N >= 64, "S=%d A=%d launch %d: N=%d", S, A, i, L.N);
    CHECK(L.C >= 256 && L.C % 64 == 0, "S=%d A=%d launch %d: C=%d", S, A, i, L.C);
    CHECK(L.N <= aN && L.C <= aC, "S=%d launch %d: capacities (%d, %d) above those asked for (%d, %d)", S, i, L.N, L.C, aN, aC);
    CHECK(L.hbits == vplan::hash_bits(S, L.N), "S=%d launch %d: hbits %d is not that of N=%d", S, i, L.hbits, L.N);
    CHECK(L.hbits == 0 || ((1L << L.hbits) >= 4L * L.N && (1L << L.hbits) <= (long)S), "S=%d launch %d: N=%d hbits=%d", S, i, L.N, L.hbits);
    // lists in LDS exactly when the carve with lists, at the capacities asked for, fits
    const bool fits = vplan::lds_bytes(S, aN, aC, true, eps) <= vplan::kLdsLimit;
    CHECK(L.lists_in_lds == fits, "S=%d A=%d launch %d: lists_in_lds=%d, the carve with lists %s", S, A, i, (int)L.lists_in_lds,
          fits ? "fits" : "does not fit");
    // a launch that keeps its lists in LDS is never shrunk; a shrunk one was halved, 64 at a time, from what was asked
    if (L.lists_in_lds) CHECK(L.N == aN && L.C == aC, "S=%d launch %d: shrunk with lists in LDS", S, i);
    {
      // the shrink halves the capacity, 64 at a time, and stops at the first one whose list-free carve fits
      int n = aN, c = aC;
      while (!L.lists_in_lds && vplan::lds_bytes(S, n, c, false, eps) > vplan::kLdsLimit && n > 64) {
        n = ceil64(n / 2);
        if (c > 8 * n) c = 8 * n;
      }
      CHECK(n == L.N && c == L.C, "S=%d A=%d launch %d: capacities (%d, %d), expected (%d, %d)", S, A, i, L.N, L.C, n, c);
    }
    if (L.N < aN) {
      r.shrunk++;
      if (vplan::lds_bytes(S, L.N, L.C, true, eps) <= vplan::kLdsLimit) r.lists_would_fit_after_shrink++;
    }
    if (!L.lists_in_lds) r.hbm++;
    if (L.hbits) r.hashed++;
    // The expression this plan replaced: lists in LDS when the carve fits in HALF the limit, or — for every launch but a
    // pass-1 launch over all utterances — in the limit.  The first clause decides only for such a launch.
    const size_t with_lists = vplan::lds_bytes(S, aN, aC, true, eps);
    const bool was = with_lists <= vplan::kLdsLimit / 2 || ((L.pass == 0 || L.code != 0) && with_lists <= vplan::kLdsLimit);
    if (!(L.pass == 0 || L.code != 0)) r.half_limit_decides++;
    CHECK(was == L.lists_in_lds, "S=%d launch %d: the half-limit clause would have decided otherwise", S, i);
  }
}

// smallest max_states (graphs of 3.8 arcs a state, one token per state, beam and retry beam) at which some launch of the
// plan satisfies `pred`
template <class Pred>
int threshold(bool eps, bool lazy, Pred pred) {
  for (int S = 1; S <= 20000; S++) {
    mfa_align_opts o{10.0f, 40.0f, 0.1f, S, S};
    const vplan::Plan pl = vplan::viterbi_plan(&o, S, (int)(3.8 * S) + 1, eps, lazy);
    for (int i = 0; i < pl.n; i++) if (pred(pl.l[i], S)) return S;
  }
  return -1;
}

}  // namespace

int main() {
  Reach r;
  for (int S = 1; S <= 20000; S++) {
    std::vector<int> arcs = {1, 255, 256, 257, (int)(3.8 * S) + 1, 8 * S};
    const int steps = 8 * S / 64, stride = 64 * (steps / 8 + 1);
    for (int a = 64; a <= 8 * S; a += stride) arcs.push_back(a);
    const int tokens[7] = {0, 64, 256, 512, 1024, 4096, S};
    for (int a : arcs) {
      if (a < 1 || a > 8 * S) continue;
      for (int mt : tokens)
        for (int eps = 0; eps < 2; eps++)
          for (int lazy = 0; lazy < 2; lazy++)
            for (int retry = (a == (int)(3.8 * S) + 1 ? 0 : 1); retry < 2; retry++) {
              mfa_align_opts o{10.0f, retry ? 40.0f : 0.0f, 0.1f, mt, 512};
              check_plan(o, S, a, eps != 0, lazy != 0, r);
            }
    }
  }
  // bad arguments
  {
    mfa_align_opts o{10.0f, 40.0f, 0.1f, 1024, 512};
    int32_t rows[21];
    CHECK(vplan::viterbi_plan_rows(nullptr, 10, 10, false, false, rows, 3) == -2, "null options");
    CHECK(vplan::viterbi_plan_rows(&o, 0, 10, false, false, rows, 3) == -2, "no states");
    CHECK(vplan::viterbi_plan_rows(&o, 10, 0, false, false, rows, 3) == -2, "no arcs");
    rows[7] = 12345;
    CHECK(vplan::viterbi_plan_rows(&o, 5000, 19000, false, false, rows, 1) == 3 && rows[7] == 12345, "cap = 1 writes one row");
    CHECK(vplan::viterbi_plan_rows(&o, 5000, 19000, false, false, nullptr, 0) == 3, "a count without rows");
  }
  printf("plans %ld, launches %ld: lists in HBM %ld, shrunk %ld, hashed table %ld\n", r.plans, r.launches, r.hbm, r.shrunk, r.hashed);
  // The refusal (tables beyond 160 KiB at 64 tokens) cannot be reached: at 64 tokens the hashed table has 256 entries
  // whenever the graph has 256 states or more, and the carve is below 12 KB whatever the graph.  The branch stays in
  // viterbi_plan and align_impl as a guard for a layout that grows.
  printf("refused plans: %ld (the refusal branch is %s)\n", r.refused, r.refused ? "REACHABLE" : "unreachable in the sweep");
  CHECK(r.refused == 0, "the refusal branch was reached %ld times", r.refused);
  // The kLdsLimit / 2 clause of the former lists_in_lds expression could decide only for a pass-1 launch with code 0; the
  // retry launch always carries the pending code.  Never reached, never decided: the plan tests the limit alone.
  printf("launches the half-limit clause could decide for: %ld (the clause is %s)\n", r.half_limit_decides,
         r.half_limit_decides ? "LIVE" : "dead");
  CHECK(r.half_limit_decides == 0, "the half-limit clause had %ld launches to decide for", r.half_limit_decides);
  printf("shrunk launches whose lists would fit in LDS at the shrunk capacity: %ld\n", r.lists_would_fit_after_shrink);
  CHECK(r.hbm > 0 && r.shrunk > 0 && r.hashed > 0, "the sweep did not reach every tier");
  for (int eps = 0; eps < 2; eps++) {
    const int hbm = threshold(eps != 0, false, [](const vplan::Launch &L, int) { return !L.lists_in_lds; });
    const int shrink = threshold(eps != 0, false, [](const vplan::Launch &L, int S) { return !L.grow && L.N < ceil64(S); });
    printf("threshold %s: token lists in HBM from max_states %d, capacity shrink from max_states %d\n",
           eps ? "with epsilon arcs" : "epsilon-free", hbm, shrink);
    CHECK(hbm > 0 && shrink > hbm, "thresholds out of order");
  }
  if (failures) { printf("%ld checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
