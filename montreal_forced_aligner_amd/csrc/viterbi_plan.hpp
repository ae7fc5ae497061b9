// The wavefront decoder's launch plan: which launches align_impl (viterbi.hip) makes for a batch, with which token and
// candidate capacities, how many bytes of LDS each one carves, whether its token lists live in LDS or in HBM, and the size
// of its state→slot table.  Pure host code without HIP includes: align_impl consumes viterbi_plan(), mfa_debug_viterbi_plan
// exports it, and tests/native/viterbi_plan_check.cpp sweeps it on the CPU.
//
// The constants below restate the kernels' (viterbi_common.hpp, viterbi_eps.hpp, viterbi_small.hpp, which need the HIP
// headers); viterbi.hip holds them to those with static_asserts.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mfa_hip.h"

namespace vplan {

constexpr int kLlCap = 512;            // score-row cache of viterbi_kernel, in columns
constexpr int kBmWords = 64;           // bitmap of scored columns (viterbi_common.hpp)
constexpr int kEpsWordsPerSlot = 7;    // EpsArrays (viterbi_eps.hpp)
constexpr int kSmallN = 64;            // viterbi_small_kernel's token capacity (viterbi_small.hpp)
constexpr int kDenseFirstTier = 128;   // first-tier capacity of the dense path (viterbi_kernel)
constexpr int kCodePending = -1;       // ST_PENDING: the retry-beam launch decodes the utterances left with it
constexpr int kCodeGrow = -2;          // ST_GROW: the growth launch decodes the utterances the first tier gave up
constexpr size_t kLdsLimit = 160 * 1024;
constexpr int kMaxLaunches = 3;

// state→slot hash table: a power of two, at least four entries per live-token slot
// — unless one entry per graph state is smaller (the large tiers of the rare passes): then 0 = direct map.
// A hashed table never has more buckets than the graph has states (2^b ≤ S).
inline int hash_bits(int S, int N) {
  int b = 8;
  while ((1 << b) < 4 * N) b++;
  return ((size_t)1 << b) <= (size_t)S ? b : 0;
}
// Dynamic-LDS bytes of a viterbi_kernel launch.  Kept by hand in step with the "LDS carve" at the top of viterbi_kernel
// (viterbi_wave.hpp): an array added there needs its term here, or the kernel runs past its allocation.
inline size_t lds_bytes(int S, int N, int C, bool lists_in_lds, bool eps = false) {
  const int hb = hash_bits(S, N);
  const size_t table = hb ? ((size_t)4 << hb) : (size_t)((S + 1) & ~1) * 4;
  return (size_t)N * 8 + table + (size_t)N * 7 * 4 + (size_t)C * 4 + (size_t)kLlCap * 4 + 16 + (size_t)kBmWords * 4 +
         (lists_in_lds ? (size_t)N * 32 : 0) + (eps ? (size_t)N * kEpsWordsPerSlot * 4 : 0);   // eps: EpsArrays
}

// N = live-token capacity, C = per-frame candidate capacity.  One token per state and one candidate per arc are hard
// upper bounds, so the retry pass (whose beam keeps most of the graph alive) is given room that cannot overflow — as long
// as the tables fit (see the shrink in viterbi_plan).
inline void pick_caps(const mfa_align_opts *o, int max_states, int max_arcs, int pass, int *N, int *C) {
  int n = o->max_tokens > 0 ? o->max_tokens : 1024;
  if (pass == 1) n = n * 4;
  if (n > max_states) n = max_states;
  n = (n + 63) & ~63;
  if (n < 64) n = 64;
  int c = pass == 1 ? 8 * n : 4 * n;
  if (c > max_arcs) c = max_arcs;
  c = (c + 63) & ~63;
  if (c < 256) c = 256;
  *N = n; *C = c;
}

struct Launch {
  int pass;            // 0: beam, 1: retry beam
  int N, C;            // capacities of this launch (after the shrink)
  int code;            // 0: every utterance; otherwise the status that selects this launch's utterances
  int grow;            // first tier: an overflow marks the utterance ST_GROW instead of failing it
  size_t lds;          // lds_bytes of the launch
  bool lists_in_lds;   // viterbi_kernel<true, *> or <false, *>
  int hbits;           // log2 of the hashed table's size, 0 = direct map
};

struct Plan {
  int n;                       // launches, in order
  Launch l[kMaxLaunches];
  int N[2], C[2];              // what pick_caps gave per pass, before any shrink (the workspace is laid out for these)
  int refused;                 // index of the first launch whose tables do not fit even at 64 tokens, or -1
};

// `lazy`: mfa_align_features_batch.  Its first tier is viterbi_small_kernel, whose carve is its own and fixed; the row of
// that launch holds viterbi_kernel's figures for the same capacities (align_impl sets the function attribute from them).
inline Plan viterbi_plan(const mfa_align_opts *o, int max_states, int max_arcs, bool eps, bool lazy) {
  Plan pl;
  pl.n = 0; pl.refused = -1;
  for (int ps = 0; ps < 2; ps++) pick_caps(o, max_states, max_arcs, ps, &pl.N[ps], &pl.C[ps]);
  const int passes = o->retry_beam != 0.0f ? 2 : 1;
  // First-tier capacity.  With the hashed state→slot table nothing in the decoder's LDS scales with the graph: 64 tokens
  // need 9.5 KB → 16 wavefronts per CU (a whole batch of 4 096 resident at once on 256 CUs), 128 tokens 14.6 KB → 10.
  // The lazy path's first tier is viterbi_small_kernel (kSmallN tokens), the dense path's the general kernel.
  const int first_tier = lazy ? kSmallN : kDenseFirstTier;
  auto add = [&](int pass, int N, int C, int code, int grow) { pl.l[pl.n++] = Launch{pass, N, C, code, grow, 0, false, 0}; };
  if (pl.N[0] > first_tier) {
    add(0, first_tier, pl.C[0] < 4 * first_tier ? pl.C[0] : 4 * first_tier, 0, 1);
    add(0, pl.N[0], pl.C[0], kCodeGrow, 0);
  } else {
    add(0, pl.N[0], pl.C[0], 0, 0);
  }
  if (passes == 2) add(1, pl.N[1], pl.C[1], kCodePending, 0);
  for (int i = 0; i < pl.n; i++) {
    Launch &L = pl.l[i];
    // token lists in LDS when everything fits; in HBM for big graphs / the wide retry beam; and if even the atomically
    // updated tables do not fit, shrink the token capacity (an overflow is then reported per utterance: above that size
    // PackedGraphs.hard_bounds() cannot keep its promise, and the host's capacity ladder ends at the general decoder)
    // (the list passes — table growth, retry beam — hold a handful of utterances: occupancy does not matter there, the
    //  per-frame latency of HBM-resident lists does)
    L.lists_in_lds = lds_bytes(max_states, L.N, L.C, true, eps) <= kLdsLimit;
    while (lds_bytes(max_states, L.N, L.C, L.lists_in_lds, eps) > kLdsLimit && L.N > 64) {
      L.N = (L.N / 2 + 63) & ~63;
      if (L.C > 8 * L.N) L.C = 8 * L.N;
    }
    L.lds = lds_bytes(max_states, L.N, L.C, L.lists_in_lds, eps);
    L.hbits = hash_bits(max_states, L.N);
    if (L.lds > kLdsLimit && pl.refused < 0) pl.refused = i;
  }
  return pl;
}

// mfa_debug_viterbi_plan's body (include/mfa_hip.h): one row of seven int32 per launch.
inline int viterbi_plan_rows(const mfa_align_opts *o, int max_states, int max_arcs, bool eps, bool lazy, int32_t *out, int cap) {
  if (!o || max_states <= 0 || max_arcs <= 0) return -2;
  const Plan pl = viterbi_plan(o, max_states, max_arcs, eps, lazy);
  if (pl.refused >= 0) return -1;
  for (int i = 0; i < pl.n && i < cap && out; i++) {
    const Launch &L = pl.l[i];
    int32_t *r = out + 7 * i;
    r[0] = L.pass; r[1] = L.code; r[2] = L.N; r[3] = L.C; r[4] = (int32_t)L.lds; r[5] = L.lists_in_lds ? 1 : 0; r[6] = L.hbits;
  }
  return pl.n;
}

}  // namespace vplan
