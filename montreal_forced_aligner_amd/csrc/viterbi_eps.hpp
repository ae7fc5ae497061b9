// FasterDecoder's epsilon closures for the frame-loop kernels' kEps instantiations (graphs with epsilon input arcs):
// InitDecoding's ProcessNonemitting before frame 0 and the per-frame ProcessNonemitting, with the state → slot table they
// file tokens into and their LDS arrays.  One wavefront; the callers are viterbi_kernel<·, true> and
// viterbi_small_kernel<·, true> (viterbi_kernel's emitting phases use the slot table in every instantiation).
#pragma once
#include "viterbi_common.hpp"

namespace {

// ---- state → slot: an open-addressing hash table (linear probing) over the states that received a candidate THIS frame —
// at most N of them, whatever the size of the graph.  Hash policies: viterbi_kernel's runtime table of 2^hbits entries (or
// one entry per graph state, addressed by state id: `direct`, no collisions), viterbi_small_kernel's 256 entries.
// Two copies of the probe rule remain outside this type, because through it the epsilon-free kernels' machine code changed:
// the claim loop of viterbi_small_kernel's emitting phase, and the read-only lookup (`find`) of both kernels' ordering pass.
struct HashRuntime {
  bool direct; u32 mask; int shift;
  __device__ __forceinline__ u32 operator()(u32 d) const { return direct ? d : (d * 2654435761u) >> shift; }
};
struct Hash256 {
  static constexpr u32 mask = 255u;
  __device__ __forceinline__ u32 operator()(u32 d) const { return (d * 2654435761u) >> 24; }
};
template <class Hash>
struct SlotTable {
  u32 *hmap;                                      // slot index | kEmpty | kClaim | kOver
  u32 *nslots;                                    // slots handed out this frame (may run past N: overflow)
  int N;                                          // slots
  u32 *s_state, *s_an;                            // per slot: state, its packed arc range
  u64 *s_cost;                                    // per slot: best cost key
  u32 *s_F, *s_W, *s_bucket;                      // per slot: first creator, winner, hash bucket
  Hash hash;
  // One probe step of find-or-insert for a pending candidate (wavefront-collective loops call it in rounds with a
  // hand-over point between rounds; `res` starts as kEmpty): an empty bucket is claimed by compare-and-swap, the winner
  // allocates a slot, initialises it and publishes the index; a lane that lost the race (kClaim seen, or its own CAS
  // failed) looks again next round and finds either its own state (done) or a different one (moves on to the next bucket).
  __device__ __forceinline__ void probe(bool &pend, u32 &h, u32 &res, u32 d, u32 dan) const {
    if (!pend) return;
    const u32 v = hmap[h];
    if (v == kEmpty) {
      if (atomicCAS(&hmap[h], kEmpty, kClaim) == kEmpty) {
        const u32 my = atomicAdd(nslots, 1u);
        if (my < (u32)N) {
          s_state[my] = d; s_an[my] = dan; s_cost[my] = kKeyInf; s_F[my] = kEmpty; s_W[my] = kEmpty; s_bucket[my] = h;
          hmap[h] = my;
          res = my;
        } else {
          hmap[h] = kOver;            // no slot left: nslots > N is reported right after the expansion
          res = kEmpty;
        }
        pend = false;
      }
    } else if (v == kOver) {
      res = kEmpty; pend = false;
    } else if (v != kClaim) {
      if (s_state[v] == d) { res = v; pend = false; }
      else h = (h + 1u) & hash.mask;
    }
  }
};

// Per-slot arrays of the epsilon closures at the end of a kEps kernel's dynamic LDS, N words each unless noted: the slot's
// list position, the inverse, the winning epsilon arc, a scratch word for the winner vote, the state's epsilon-arc info;
// the stack of ProcessNonemitting [2N].  kEpsWordsPerSlot is what the host adds per slot to a launch's LDS bytes
// (lds_bytes() in viterbi.hip, SmallLds in viterbi_small.hpp).
constexpr int kEpsWordsPerSlot = 7;
struct EpsArrays {
  u32 *pos, *inv, *arc, *tmp, *info, *stk;
  __device__ __forceinline__ EpsArrays(unsigned char *base, int N)
      : pos((u32 *)base), inv(pos + N), arc(inv + N), tmp(arc + N), info(tmp + N), stk(info + N) {}
};

// ---------------- InitDecoding's ProcessNonemitting(cutoff = FLT_MAX), as Kaldi runs it: a stack, the popped token's
// epsilon arcs one after the other.  Once per utterance and a handful of tokens, so the wavefront simply walks the
// sequential algorithm (every lane the same scalars, lane 0 stores, destinations looked up by a ballot over the tokens
// created so far — one ballot when the table holds 64 slots).  Tokens in creation order: s_state / s_cost (cost bits) /
// e.arc / e.inv (creator) / s_an; then the hash-list order (buckets by first occupancy, creation order inside) gives the
// initial list (l_state, l_cost, l_an) and its back-pointer records — bp[0 .. n): the start token's carries arc 0xFFFFFFFF,
// the others an epsilon arc and a position in this list.  Returns n, or -1: more tokens than slots, or pops than p.eps_pops.
template <class Tab>
__device__ __forceinline__ int init_closure(const VitParams &p, int utt, int lane, int start, int64_t so, const int32_t *arc_off,
                                            const uint4 *a_rec, u32 H, const Tab &tab, const EpsArrays &e, u32 *l_state,
                                            double *l_cost, u32 *l_an, u64 *bp) {
  const u32 N = (u32)tab.N;
  u32 *s_state = tab.s_state, *s_an = tab.s_an;
  u64 *s_cost = tab.s_cost;
  u32 nc_ = 1u;
  if (lane == 0) {
    s_state[0] = (u32)start; s_cost[0] = (u64)__double_as_longlong(0.0); e.arc[0] = 0xFFFFFFFFu; e.inv[0] = 0u;
    s_an[0] = ((u32)arc_off[start] << 7) | min((u32)p.g.d_state_nemit[so + start], 127u);
    e.stk[0] = 0u;
  }
  WSYNC();
  u32 sp = 1u;
  int guard = 0;
  while (sp > 0u) {
    if (++guard > p.eps_pops) return -1;
    const u32 pe = e.stk[sp - 1u];
    sp--;
    const double ce = __longlong_as_double((long long)s_cost[pe]);
    const u32 ei = p.w_epsinfo[(size_t)utt * p.eps_stride + s_state[pe]];
    const u32 n_eps = ei & 127u, first = ei >> 7;
    for (u32 k = 0; k < n_eps; k++) {
      const uint4 rec = a_rec[first + k];
      const u32 d = rec.x;
      const double ncst = ce + (double)__uint_as_float(rec.w);
      if (ncst > (double)3.4028234663852886e38f) continue;      // cutoff = numeric_limits<float>::max()
      u32 found = kEmpty;
      for (u32 c0 = 0; c0 < min(nc_, N); c0 += 64) {
        const u32 c_ = c0 + (u32)lane;
        const u64 hit = __ballot(c_ < nc_ && s_state[c_] == d);
        if (hit) { found = c0 + (u32)__ffsll((long long)hit) - 1u; break; }
      }
      bool pushed = false; u32 who = 0u;
      if (found == kEmpty) {
        if (nc_ >= N) return -1;
        if (lane == 0) {
          s_state[nc_] = d; s_cost[nc_] = (u64)__double_as_longlong(ncst); e.arc[nc_] = first + k; e.inv[nc_] = pe; s_an[nc_] = rec.y;
        }
        who = nc_; nc_++; pushed = true;
      } else if (__longlong_as_double((long long)s_cost[found]) > ncst) {
        if (lane == 0) { s_cost[found] = (u64)__double_as_longlong(ncst); e.arc[found] = first + k; e.inv[found] = pe; }
        who = found; pushed = true;
      }
      if (pushed) {
        if (sp >= 2u * N) return -1;
        if (lane == 0) e.stk[sp] = who;
        sp++;
      }
      WSYNC();
    }
  }
  // hash-list order: position of token c = number of tokens whose (bucket's first creator, own index) is smaller
  for (u32 c0 = 0; c0 < min(nc_, N); c0 += 64) {
    const u32 c_ = c0 + (u32)lane;
    if (c_ < nc_) {
      const u32 bc = s_state[c_] % H;
      u32 lead_c = c_;
      for (u32 x = 0; x < c_; x++) if (s_state[x] % H == bc) { lead_c = x; break; }
      u32 pos_ = 0;
      for (u32 x = 0; x < nc_; x++) {
        if (x == c_) continue;
        const u32 bx = s_state[x] % H;
        u32 lead_x = x;
        for (u32 y = 0; y < x; y++) if (s_state[y] % H == bx) { lead_x = y; break; }
        if (lead_x < lead_c || (lead_x == lead_c && x < c_)) pos_++;
      }
      e.pos[c_] = pos_;
    }
  }
  WSYNC();
  for (u32 c0 = 0; c0 < min(nc_, N); c0 += 64) {
    const u32 c_ = c0 + (u32)lane;
    if (c_ < nc_) {
      const u32 pos_ = e.pos[c_];
      l_state[pos_] = s_state[c_];
      l_cost[pos_] = __longlong_as_double((long long)s_cost[c_]);
      l_an[pos_] = s_an[c_];
      bp[pos_] = ((u64)e.arc[c_] << 32) | (u64)(c_ == 0u ? 0u : e.pos[e.inv[c_]]);
    }
  }
  __threadfence_block();
  WSYNC();
  return (int)nc_;
}

// ---------------- FasterDecoder::ProcessNonemitting(next_weight_cutoff).  The new tokens live in the slot table
// (state, cost key, first creator, winner) and the ordering pass has just given each its list position.  Kaldi pushes the
// list on a stack (last token on top) and pops: a popped token's epsilon arcs, in arc order, insert their destination
// (end of its hash bucket's chain) or replace its token when strictly cheaper, and push it.  Costs come out the same
// whatever the order (label-correcting search, epsilon weights >= 0); the order of insertion — hence the list order the
// next frame walks — and the back-pointer on ties do not, so the pops run one after the other as Kaldi's do; the popped
// state's epsilon arcs are relaxed by the lanes in parallel with arc order restored where it matters (first creator
// by atomicMin on the ordinal, earlier duplicates of a destination by a lane loop, pushes by ballot prefix).  States
// without epsilon arcs are never pushed: popping them does nothing.
// The caller has filled e.info for the frame's slots and e.stk[0 .. sp) with those that have epsilon arcs, in list order.
// New slots get first-creator ordinals ord_base + 0, 1, … (s_F = 0x80000000 | k); `eord` returns how many were handed out.
enum EpsClosure { kEpsDone, kEpsCapacity, kEpsDegree };   // finished / a table, the stack, the pop budget or C exceeded / a state with more than 64 epsilon arcs
template <class Tab>
__device__ __forceinline__ EpsClosure process_nonemitting(const VitParams &p, int utt, int lane, const uint4 *a_rec, const Tab &tab,
                                                          const EpsArrays &e, double eps_cut, u32 sp, u32 ord_base, u32 C, u32 &eord) {
  const u32 N = (u32)tab.N;
  u64 *s_cost = tab.s_cost;
  eord = 0;
  int guard = 0;
  while (sp > 0u) {
    if (++guard > p.eps_pops) return kEpsCapacity;
    const u32 pe = e.stk[sp - 1u];
    sp--;
    const double ce = dunkey(s_cost[pe]);
    if (ce > eps_cut) continue;
    const u32 ei = e.info[pe];
    const u32 n_eps = ei & 127u, first = ei >> 7;
    if (n_eps == 0u) continue;
    if (n_eps > 64u) return kEpsDegree;
    const bool valid = (u32)lane < n_eps;
    u32 nx = 0u, nan_ = 0u; float w = 0.0f;
    if (valid) { const uint4 rec = a_rec[first + (u32)lane]; nx = rec.x; nan_ = rec.y; w = __uint_as_float(rec.w); }
    const double nc = ce + (double)w;           // Kaldi: new_tok->cost_ = tok->cost_ + arc.weight (no acoustic term)
    const bool ok0 = valid && !(nc > eps_cut);
    u32 sl = kEmpty;
    {
      bool pend = ok0; u32 h = tab.hash(nx);
      while (__any(pend)) { tab.probe(pend, h, sl, nx, nan_); WSYNC(); if (*tab.nslots > N) break; }
    }
    if (*tab.nslots > N) return kEpsCapacity;
    const bool ok = ok0 && sl != kEmpty;
    const u64 okm = __ballot(ok);
    const u64 pre = ok ? s_cost[sl] : kKeyInf;  // before this pop: infinite = the state was not in the list
    const bool is_new = ok && pre == kKeyInf;
    if (is_new) e.info[sl] = p.w_epsinfo[(size_t)utt * p.eps_stride + nx];
    // earlier arcs of this pop into the same state (rare): what Kaldi's sequential loop would have left there
    double pm = INFINITY; bool first_dup = true;
    for (u32 j = 0; j < n_eps; j++) {
      const u32 nxj = (u32)__builtin_amdgcn_readlane((int)nx, (int)j);
      const double ncj = readlane_f64(nc, (int)j);
      if (((okm >> j) & 1ull) && (u32)lane > j && nxj == nx) { pm = min_f64(pm, ncj); first_dup = false; }
    }
    const bool push = ok && (is_new ? (first_dup || nc < pm) : (nc < min_f64(dunkey(pre), pm)));
    WSYNC();                                    // every lane has read `pre`
    if (push) atomicMin(&s_cost[sl], dkey(nc));
    if (is_new) atomicMin(&tab.s_F[sl], 0x80000000u | (eord + (u32)__popcll(okm & ((1ull << lane) - 1ull))));
    WSYNC();
    const bool win = push && dkey(nc) == s_cost[sl];
    if (win) atomicMin(&e.tmp[sl], (u32)lane);
    WSYNC();
    if (win && e.tmp[sl] == (u32)lane) { tab.s_W[sl] = 0x80000000u | pe; e.arc[sl] = first + (u32)lane; }
    WSYNC();
    if (win) e.tmp[sl] = 0xFFFFFFFFu;
    const bool pp = push && (e.info[sl] & 127u) != 0u;
    const u64 pmk = __ballot(pp);
    const u32 at = sp + (u32)__popcll(pmk & ((1ull << lane) - 1ull));
    if (pp && at < 2u * N) e.stk[at] = sl;
    sp += (u32)__popcll(pmk);
    if (sp > 2u * N) return kEpsCapacity;
    eord += (u32)__popcll(okm);
    if (ord_base + eord > C) return kEpsCapacity;
    WSYNC();
  }
  return kEpsDone;
}

}  // namespace
