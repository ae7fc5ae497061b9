// Shared by the decoder sources (viterbi.hip and its headers, viterbi_general.hip): constants, status codes, the launch
// parameters, wavefront primitives, the scored-column bitmap and the finalisation of one utterance.
#pragma once
#include <cmath>
#include <cstdint>

#include "ctx.hpp"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u32 kEmpty = 0xFFFFFFFFu;
constexpr u32 kClaim = 0xFFFFFFFEu;
constexpr u32 kOver = 0xFFFFFFFDu;   // hash bucket of a state that found no free slot (the frame is about to report overflow)
constexpr u64 kKeyInf = 0xFFFFFFFFFFFFFFFFull;
constexpr int kMinActive = 20;
constexpr float kBeamDelta = 0.5f;
constexpr float kHashRatio = 2.0f;
constexpr int kArcBits = 6;               // at most 64 arcs per state
constexpr int kMaxArcsPerState = 1 << kArcBits;

// d_status codes (include/mfa_hip.h; >= 0 are ABI), shared with viterbi_general.hip
enum { ST_OK = 0, ST_RETRIED = 1, ST_FAILED = 2, ST_TOKEN_OVERFLOW = 3, ST_BP_OVERFLOW = 4, ST_UNSUPPORTED = 5, ST_INTERNAL = 6, ST_WORDS = 7, ST_PENDING = -1, ST_GROW = -2 };

// decoder state of one utterance between two windows (the token list itself is parked in w_state / w_cost).  pad0 is the
// utterance's lag in the 64-token first tier: 1 — its window in this launch is the previous one (a failed speculation
// being redone with the proven band, by the first tier itself); the utterance stays one window behind from then on.
struct VitState { int32_t n, cur, done, pad0; u32 H, pad1; u64 bp_used; };

struct VitParams {
  mfa_graph_batch g;
  const float *ll; const int64_t *ll_off; const int32_t *ll_cols; const int64_t *frame_off;
  float beam, scale;
  int nmax, cmax, bpf;        // live-token capacity, candidate capacity, back-pointer tokens per frame
  int hbits;                  // log2 of the state→slot hash table size (>= 4 x nmax entries); 0: direct map, one entry per state
  const int32_t *utt_list;    // utterances to decode (NULL: identity)
  const int32_t *n_list;      // number of entries in utt_list (device scalar) or NULL
  int pass;                   // 0 first beam, 1 retry
  int grow;                   // 1: a token/candidate overflow is not final — the utterance is re-run with larger tables
  // workspace
  u32 *w_state; double *w_cost;        // [n_utt][2][nmax]
  u32 *w_stash_a; u64 *w_stash_key;    // [n_utt][cmax]: (slot<<32|cidx) packed in stash_a pair → two arrays
  u32 *w_stash_b;
  u64 *w_bp;                           // [total_frames*bpf] (arc index <<32 | prev pos)
  u32 *w_tokoff;                       // [total_frames + n_utt]
  u32 *w_hash;                         // [n_utt] hash size carried from pass 0 to the retry pass
  const uint4 *w_arcnext;              // [total_arcs] {next, (arc_off[next] << 7) | out-degree(next), col, weight}, built once per call
  // Graphs with epsilon input arcs (g.d_state_nemit != NULL: every state's arcs are stored [emitting | epsilon] and the
  // out-degree above counts the emitting ones): per state {first epsilon arc << 7 | number of epsilon arcs}, built once per call
  const u32 *w_epsinfo;                // [n_utt * max_states] at (utt * max_states + state), or NULL
  int eps_stride;                      // max_states
  int eps_pops;                        // pops of one frame's epsilon closure before the utterance is handed back with a capacity status (64 per token slot; Kaldi has no budget: the caller's last resort is the general decoder)
  unsigned long long *stamps;          // -DVIT_STAMPS builds: per-utterance phase cycles (mfa_debug_viterbi_stamps) or NULL
  int llcap;                           // score-row cache capacity in LDS (floats); rows longer than this are read from HBM
  // windowed (resumable) decoding — mfa_align_features_batch: one launch decodes frames [t_begin, t_end) of every utterance,
  // parks the live token list in the HBM workspace and leaves the band of graph depths the NEXT window can touch
  int windowed, t_begin, t_end, next_window;
  VitState *w_vstate;                  // [n_utt]
  // Speculative look-ahead (first-beam windowed pass): the window was scored for a band narrower than the proven one; the
  // decoder checks every score it reads against the column ranges that were scored (spec_ranges, see mfa_band_ranges).  The
  // moment one lies outside, the 64-token first tier puts the utterance one window behind (VitState.pad0) and redoes the
  // window with the proven band; the general kernel gives it up (ST_GROW: decoded again from frame 0 by the list pass).
  int spec;                            // 1: check
  const int32_t *spec_ranges;          // [n_utt][kMfaRangeSlots][2]
  const int32_t *spec_class_counts;    // [n_utt][6]
  int spec_groups;                     // runs of class 0 in the plan (0/1: one)
  const int32_t *state_depth;          // [total_states][2] {fewest arcs from start, most arcs from start} (mfa_score_plan)
  int32_t *band;                       // [n_utt][2] out: {min longest-path depth of a live token, max BFS depth + next_window - 1}
  // outputs
  int32_t *ali; int32_t *words; int32_t *n_words; float *like; float *frame_like; int32_t *status;
};

__device__ __forceinline__ u64 dkey(double d) {
  u64 b = (u64)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dunkey(u64 k) {
  u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// ---- wavefront primitives on the DPP crossbar (row_shr / row_bcast / wave_shr are single VALU operand modifiers on
// gfx950; the ds_bpermute-based __shfl costs an LDS round trip per step).  Inclusive scan: Kogge-Stone inside each row
// of 16 lanes, then row_bcast:15 / row_bcast:31 carry the row totals; lane 63 ends up holding the reduction.
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ u32 dpp_u32(u32 old, u32 v) {
  return (u32)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double old, double v) {
  int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, BANK_MASK, false);
  int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ u32 incl_scan_sum(u32 v) {
  v += dpp_u32<0x111>(0, v); v += dpp_u32<0x112>(0, v); v += dpp_u32<0x114>(0, v); v += dpp_u32<0x118>(0, v);
  v += dpp_u32<0x142, 0xA>(0, v); v += dpp_u32<0x143, 0xC>(0, v);
  return v;
}
__device__ __forceinline__ u32 incl_scan_max(u32 v) {
  v = max(v, dpp_u32<0x111>(0, v)); v = max(v, dpp_u32<0x112>(0, v)); v = max(v, dpp_u32<0x114>(0, v));
  v = max(v, dpp_u32<0x118>(0, v)); v = max(v, dpp_u32<0x142, 0xA>(0, v)); v = max(v, dpp_u32<0x143, 0xC>(0, v));
  return v;
}
// min of two costs as ONE instruction.  fmin() is llvm.minnum: with IEEE mode on it first canonicalises both operands
// (v_max_f64 x, x, x) in case one is a signalling NaN — the decoder's costs are finite or +inf, never NaN, and every DPP scan
// step paid two extra double-rate instructions for it (62 canonicalisations against 50 minima in the first-tier kernel).
__device__ __forceinline__ double min_f64(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double incl_scan_min(double v) {
  const double inf = INFINITY;
  v = min_f64(v, dpp_f64<0x111>(inf, v)); v = min_f64(v, dpp_f64<0x112>(inf, v)); v = min_f64(v, dpp_f64<0x114>(inf, v));
  v = min_f64(v, dpp_f64<0x118>(inf, v)); v = min_f64(v, dpp_f64<0x142, 0xA>(inf, v)); v = min_f64(v, dpp_f64<0x143, 0xC>(inf, v));
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) { return readlane_f64(incl_scan_min(v), 63); }
__device__ __forceinline__ u32 wave_max_u32(u32 v) { return (u32)__builtin_amdgcn_readlane((int)incl_scan_max(v), 63); }
// exclusive prefixes from an inclusive scan: shift the wavefront right by one lane (wave_shr:1), identity into lane 0
__device__ __forceinline__ double shift_in_min(double incl) { return dpp_f64<0x138>((double)INFINITY, incl); }

// Kaldi: ac_cost = -(scale * loglike) in float; new_weight = (double)arc.weight + tok.cost + ac_cost
__device__ __forceinline__ double cand_cost(float w, double cost, float ll, float scale) {
  float ac = -(scale * ll);
  return ((double)w + cost) + (double)ac;
}

// Optional per-phase cycle accounting (-DVIT_STAMPS builds): s_memtime deltas accumulated per phase over all frames of an
// utterance, written to the buffer given to mfa_debug_viterbi_stamps ([n_utt][12] uint64; tools/viterbi_phases.py):
// [0..8] phases, [9] frames that needed the exact min_active selection, [10] tokens entering the frames, [11] frames.
// The default build compiles every call to nothing.
#ifdef VIT_STAMPS
struct VitStamps {
  unsigned long long acc[12] = {0}, last;
  __device__ __forceinline__ unsigned long long now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
  }
  __device__ __forceinline__ void start() { last = now(); }
  __device__ __forceinline__ void mark(int k) { const unsigned long long t = now(); acc[k] += t - last; last = t; }
  __device__ __forceinline__ void count(int k, unsigned long long v) { acc[k] += v; }
  // accumulated over the windows of the first tier (the caller zeroes the buffer)
  __device__ __forceinline__ void flush(const VitParams &p, int utt, int lane) {
    if (lane == 0 && p.pass == 0 && p.stamps && p.utt_list == nullptr)
      for (int k = 0; k < 12; k++) p.stamps[(size_t)utt * 12 + k] += acc[k];
  }
};
#else
struct VitStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void count(int, unsigned long long) {}
  __device__ __forceinline__ void flush(const VitParams &, int, int) {}
};
#endif

// hand-over point between lanes of one wavefront (see the LDS carve comment in the kernel)
#define WSYNC()                                            \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

// Columns scored for the current window as a bitmap in LDS (one wavefront; kBmWords × 32 columns).
constexpr int kBmWords = 64;
__device__ __forceinline__ void build_scored_bitmap(const VitParams &p, int utt, int lane, u32 *bm) {
  for (int i = lane; i < kBmWords; i += 64) bm[i] = 0u;
  WSYNC();
  const int32_t *rg = p.spec_ranges + (size_t)utt * kMfaRangeSlots * 2;
  const int32_t *cc6 = p.spec_class_counts + (size_t)utt * 6;
  const int runs = p.spec_groups > 1 ? p.spec_groups : 1;
  for (int slot = 0; slot < kMfaRangeSlots; slot++) {
    if (slot < kMfaRunSlots && slot >= runs) continue;
    int base = 0;                                                            // first column of the slot's class
    if (slot == kMfaRunSlots + 3) base = cc6[0];                             // class 1
    else if (slot == kMfaRunSlots + 4) base = cc6[0] + cc6[1] + cc6[2] + cc6[3] + cc6[4];   // class 5
    else if (slot >= kMfaRunSlots) { base = cc6[0] + cc6[1]; for (int k = 2; k < slot - kMfaRunSlots + 2; k++) base += cc6[k]; }
    const int a = base + rg[2 * slot], b = base + rg[2 * slot + 1];
    for (int c = a + lane; c < b; c += 64)
      if (c >= 0 && c < 32 * kBmWords) atomicOr(&bm[c >> 5], 1u << (c & 31));
  }
  WSYNC();
}
__device__ __forceinline__ bool column_scored(const u32 *bm, int col) {
  return (u32)col < (u32)(32 * kBmWords) && ((bm[col >> 5] >> (col & 31)) & 1u) != 0u;
}

// Band of graph depths the next window's frames can reach, from the live tokens' depths at a window's end.  A token on
// state s at frame t' >= t descends from a live token l of frame t, so
//   bfs_depth(s) <= bfs_depth(l) + (t' - t)   and   longest_depth(s) >= longest_depth(l):
// a pdf can be asked for in [t, t + K) only if some arc emitting it leaves a state inside those two bounds.
// dmax: max of bfs depth; dmin_inv: max of ~longest (= min of longest).  One lane calls it.
__device__ __forceinline__ void publish_band(const VitParams &p, int utt, u32 dmax, u32 dmin_inv) {
  const long long hi = (long long)dmax + (long long)p.next_window - 1;
  p.band[2 * utt] = p.state_depth ? (int32_t)~dmin_inv : 0;
  p.band[2 * utt + 1] = p.state_depth ? (int32_t)min(hi, (long long)INT32_MAX) : INT32_MAX;
}

// ReachedFinal / best final token, traceback, outputs (transition-ids, words, likelihood) of one utterance whose frame
// loop has ended with `n` tokens in (c_state, c_cost) after `t` frames.  One wavefront; shared by the frame-loop kernels
// and by viterbi_finish_kernel.
template <class StateP, class CostP>
__device__ __forceinline__ void finalize_utterance(const VitParams &p, int utt, int lane, int status, int t, int T, int n,
                                                   StateP c_state, CostP c_cost, const float *final_w, const u64 *bp,
                                                   const u32 *tokoff, int64_t f0, int64_t ab_, const float *a_w,
                                                   const int32_t *a_col, const float *ll, int P, bool eps = false,
                                                   u64 bp_used = 0, u64 bp_cap = 0) {
  // ---------------- ReachedFinal / best final token (first in list order on ties)
  int32_t out_status = status;
  double bestc = INFINITY; u32 bpos = kEmpty;
  if (status == ST_OK) {
    if (t < T || n == 0) out_status = ST_FAILED;
    else {
      for (int c0 = 0; c0 < n; c0 += 64) {
        int i = c0 + lane;
        double tc = INFINITY;
        if (i < n) {
          float fw = final_w[c_state[i]];
          if (fw != INFINITY) tc = c_cost[i] + (double)fw;
        }
        double m = wave_min_f64(tc);
        if (m < bestc) {
          const u64 hit = __ballot(i < n && tc == m);
          bpos = (u32)c0 + (u32)__ffsll((long long)hit) - 1u;
          bestc = m;
        }
      }
      if (bpos == kEmpty) out_status = ST_FAILED;
    }
  }
  if (out_status != ST_OK) {
    if (lane == 0) {
      // a first-pass failure stays pending for the retry pass; other codes are final
      p.status[utt] = (p.pass == 0 && out_status == ST_FAILED) ? ST_PENDING
                      : (p.grow && out_status == ST_TOKEN_OVERFLOW) ? ST_GROW : out_status;
      p.n_words[utt] = 0; p.like[utt] = 0.0f;
    }
    return;
  }

  int32_t *ali = p.ali + f0;
  const u32 fstate = c_state[bpos];
  const int32_t *a_il = p.g.d_arc_ilabel + ab_, *a_ol = p.g.d_arc_olabel + ab_;
  int32_t *words = p.words + f0;
  float *flike = p.frame_like ? p.frame_like + f0 : nullptr;
  u32 nw_out = 0;
  double cost = 0.0; float w1 = 0.0f, w2 = 0.0f;
  const float inv_scale = -1.0f / p.scale;
  if (eps) {
    // ---------------- graphs with epsilon input arcs: a frame's record may be followed by records of the SAME frame's list
    // (tokens that came over epsilon arcs), so the path has T + E arcs.  Traceback writes their arc indices, back to front,
    // into the unused tail of the utterance's back-pointer area; the forward pass below reads them in path order: words from
    // any arc, a transition-id and a frame only from the emitting ones, the float accumulation of Kaldi's
    // GetLinearSymbolSequence over all of them (an epsilon arc adds its weight and the rounding residue of its cost step).
    u32 *path = (u32 *)(bp + bp_used);
    const u64 pcap64 = (bp_cap - bp_used) * 2ull;
    const u32 pcap = pcap64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (u32)pcap64;
    u32 wpos = pcap, pos = bpos;
    bool full = false;
    for (int tt = T - 1; tt >= 0 && !full; tt--) {
      const u32 to = tokoff[tt];
      for (int hop = 0; ; hop++) {
        const u64 rec = bp[(u64)to + pos];
        const u32 arc = (u32)(rec >> 32);
        pos = (u32)(rec & 0xFFFFFFFFu);
        if (wpos == 0u || hop > 4096) { full = true; break; }
        wpos--;
        if (lane == 0) path[wpos] = arc;
        if (a_il[arc] != 0) break;              // an emitting arc: `pos` now refers to the previous frame's list
      }
    }
    // the initial list (InitDecoding's closure): records bp[0 .. n_init), the start token's carries arc 0xFFFFFFFF
    for (int hop = 0; !full; hop++) {
      const u64 rec = bp[pos];
      const u32 arc = (u32)(rec >> 32);
      if (arc == 0xFFFFFFFFu) break;
      if (wpos == 0u || hop > 4096) { full = true; break; }
      wpos--;
      if (lane == 0) path[wpos] = arc;
      pos = (u32)(rec & 0xFFFFFFFFu);
    }
    if (full) {
      if (lane == 0) { p.status[utt] = ST_BP_OVERFLOW; p.n_words[utt] = 0; p.like[utt] = 0.0f; }
      return;
    }
    __threadfence_block();
    WSYNC();
    const u32 L = pcap - wpos;
    u32 frames_done = 0;
    for (u32 c0 = 0; c0 < L; c0 += 64) {
      const u32 i = c0 + (u32)lane;
      int arc = 0, il = 0, ol = 0; float w = 0.0f, ac = 0.0f;
      if (i < L) { arc = (int)path[wpos + i]; il = a_il[arc]; ol = a_ol[arc]; w = a_w[arc]; }
      const u64 em = __ballot(i < L && il != 0);
      const u32 tt = frames_done + (u32)__popcll(em & ((1ull << lane) - 1ull));
      if (i < L && il != 0 && tt < (u32)T) ac = -(p.scale * ll[(size_t)tt * P + a_col[arc]]);
      const u64 mask = __ballot(ol != 0);
      const u32 wat = nw_out + (u32)__popcll(mask & ((1ull << lane) - 1ull));
      if (ol != 0 && wat < (u32)T) words[wat] = ol;
      nw_out += (u32)__popcll(mask);
      float my_fl = 0.0f;
      const int lim = (int)min(64u, L - c0);
      for (int j = 0; j < lim; j++) {
        float wj = __shfl(w, j), acj = __shfl(ac, j);
        double nc = ((double)wj + cost) + (double)acj;
        float tot = (float)(nc - cost);
        float acost = tot - wj;
        w1 += wj; w2 += acost;
        cost = nc;
        if (lane == j) my_fl = acost * inv_scale;
      }
      if (i < L && il != 0 && tt < (u32)T) { ali[tt] = il; if (flike) flike[tt] = my_fl; }
      frames_done += (u32)__popcll(em);
    }
    if (nw_out > (u32)T) {   // more word labels than frames (output labels on epsilon arcs): the output layout cannot hold them
      if (lane == 0) { p.status[utt] = ST_WORDS; p.n_words[utt] = 0; p.like[utt] = 0.0f; }
      return;
    }
  } else {
  // ---------------- traceback, arc index per frame parked in ali[].  The chain is pos → record → pos; the per-frame offsets
  // do not depend on it, so 64 of them are fetched at once and handed out by v_readlane: one dependent load per frame
  // instead of two (every lane walks the same chain on broadcast addresses; lane 0 stores).
  {
    u32 pos = bpos;
    for (int c0 = T - 1; c0 >= 0; c0 -= 64) {
      const int tl = c0 - lane;
      const u32 tokv = tl >= 0 ? tokoff[tl] : 0u;
      const int cnt = min(64, c0 + 1);
      for (int k = 0; k < cnt; k++) {
        const u32 to = (u32)__builtin_amdgcn_readlane((int)tokv, k);
        const u64 rec = bp[(u64)to + pos];
        if (lane == 0) ali[c0 - k] = (int32_t)(rec >> 32);
        pos = (u32)(rec & 0xFFFFFFFFu);
      }
    }
  }
  __threadfence_block();
  WSYNC();
  // ---------------- outputs: transition-ids, words (ordered compaction), likelihood (Kaldi's float accumulation)
  for (int c0 = 0; c0 < T; c0 += 64) {
    const int tt = c0 + lane;
    int arc = tt < T ? ali[tt] : 0;
    int il = 0, ol = 0; float w = 0.0f, ac = 0.0f;
    if (tt < T) {
      il = a_il[arc]; ol = a_ol[arc]; w = a_w[arc];
      ac = -(p.scale * ll[(size_t)tt * P + a_col[arc]]);
    }
    // words in path order
    const u64 mask = __ballot(ol != 0);
    if (ol != 0) words[nw_out + __popcll(mask & ((1ull << lane) - 1ull))] = ol;
    nw_out += (u32)__popcll(mask);
    // cost chain, sequential in frame order (every lane runs the same chain on broadcast operands)
    float my_fl = 0.0f;
    const int lim = min(64, T - c0);
    for (int j = 0; j < lim; j++) {
      float wj = __shfl(w, j), acj = __shfl(ac, j);
      double nc = ((double)wj + cost) + (double)acj;
      float tot = (float)(nc - cost);
      float acost = tot - wj;
      w1 += wj; w2 += acost;
      cost = nc;
      if (lane == j) my_fl = acost * inv_scale;
    }
    if (tt < T) { ali[tt] = il; if (flike) flike[tt] = my_fl; }
  }
  }
  if (lane == 0) {
    w1 += final_w[fstate];
    p.like[utt] = -(w1 + w2) / p.scale;
    p.n_words[utt] = (int32_t)nw_out;
    p.status[utt] = p.pass == 0 ? ST_OK : ST_RETRIED;
  }
}

}  // namespace
