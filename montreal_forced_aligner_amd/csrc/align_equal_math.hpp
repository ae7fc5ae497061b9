// The arithmetic of the equal alignment (align_equal.hip), host and device: the contract of include/mfa_hip.h ("Equal
// alignment") operation for operation.  The kernel and the host twin behind mfa_debug_align_equal_host
// (align_equal_host.cpp) both run exactly these functions, and everything here is integer arithmetic, so an utterance's
// result has the same bits on either side.  Plain C++: no HIP type, so the twin's translation unit also builds with a host
// compiler alone (tests/native/align_equal_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_AE_FN __host__ __device__ inline
#else
#define MFA_AE_FN inline
#endif

constexpr int kAeAttempts = 10;

MFA_AE_FN uint32_t mfa_ae_fmix(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// Draw `draw` of utterance `key` under `seed`: a function of the three numbers alone, no state.
MFA_AE_FN uint32_t mfa_ae_random(uint32_t seed, uint32_t key, uint32_t draw) {
  uint32_t h = mfa_ae_fmix(seed ^ 0x9E3779B9u);
  h = mfa_ae_fmix(h + key * 0x85EBCA6Bu + 0x165667B1u);
  return mfa_ae_fmix(h ^ (draw * 0xC2B2AE35u + 0x27D4EB2Fu));
}

// One of m candidates from a draw: multiply-high.
MFA_AE_FN uint32_t mfa_ae_pick(uint32_t u, uint32_t m) { return (uint32_t)(((uint64_t)u * (uint64_t)m) >> 32); }

// One utterance's graph: arc_off [S + 1] relative to the first of its A arcs; next / ilabel [A]; final [S] (+inf: not final).
struct MfaAeGraph {
  int32_t S, A, start;
  const int32_t *arc_off;
  const int32_t *next;
  const int32_t *ilabel;
  const float *final_cost;
};

// Path positions one utterance can need: a walk of at most 2 (T + S) steps and the state it ends in.
MFA_AE_FN int64_t mfa_ae_path_capacity(int64_t T, int64_t S) { return 2 * (T + S) + 1; }

// The walk, up to kAeAttempts attempts with the draws numbered on across them.  On success (returns 0) the path has
// *n_pos positions (its states, the final one included): loop_tid[i] = transition-id of position i's loop (0: the state
// cannot loop), out_tid[i] = input label of the arc the path leaves position i by (0: epsilon, and for the last position);
// *n_labels non-zero labels, *n_loopable positions that can loop.  Returns 2 when every attempt failed (or the graph is
// malformed: a state, an arc range or a next state outside it).  loop_tid / out_tid: mfa_ae_path_capacity(T, S) entries each.
MFA_AE_FN int mfa_ae_walk(const MfaAeGraph &g, int64_t T, uint32_t seed, uint32_t key, int32_t *loop_tid, int32_t *out_tid,
                          int32_t *n_pos, int32_t *n_labels, int32_t *n_loopable) {
  *n_pos = 0; *n_labels = 0; *n_loopable = 0;
  if (T < 0 || g.S <= 0 || g.start < 0 || g.start >= g.S) return 2;
  const int64_t max_steps = 2 * (T + (int64_t)g.S);
  uint32_t draw = 0;
  for (int attempt = 0; attempt < kAeAttempts; attempt++) {
    int32_t s = g.start, labels = 0, loopable = 0;
    int64_t steps = 0;
    for (;;) {
      const int32_t a0 = g.arc_off[s], a1 = g.arc_off[s + 1];
      if (a0 < 0 || a1 < a0 || a1 > g.A) return 2;
      int32_t loop = 0;
      uint32_t m = 0;
      for (int32_t a = a0; a < a1; a++) {
        if (g.next[a] == s) { if (loop == 0 && g.ilabel[a] != 0) loop = g.ilabel[a]; }
        else m++;
      }
      loop_tid[steps] = loop;
      if (loop != 0) loopable++;
      if (!(g.final_cost[s] == INFINITY)) {          // the first final state ends the walk
        out_tid[steps] = 0;
        *n_pos = (int32_t)(steps + 1); *n_labels = labels; *n_loopable = loopable;
        return 0;
      }
      if (m == 0 || steps >= max_steps) break;
      uint32_t pick = mfa_ae_pick(mfa_ae_random(seed, key, draw++), m);
      int32_t a = a0;
      for (;; a++) {
        if (g.next[a] == s) continue;
        if (pick == 0) break;
        pick--;
      }
      const int32_t il = g.ilabel[a], nx = g.next[a];
      if (nx < 0 || nx >= g.S) return 2;
      out_tid[steps] = il;
      if (il != 0 && ++labels > T) break;
      s = nx;
      steps++;
    }
  }
  return 2;
}

// Loops of the loopable position of rank `rank` (in path order among the n_loopable > 0 of them) when `extra` frames are
// to be spread: extra / n_loopable each, the first extra % n_loopable one more.
MFA_AE_FN int32_t mfa_ae_loops(int32_t extra, int32_t n_loopable, int32_t rank) {
  return extra / n_loopable + (rank < extra % n_loopable ? 1 : 0);
}
