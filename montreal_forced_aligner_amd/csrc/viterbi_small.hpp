// viterbi_small_kernel: the 64-token first tier of the windowed first-beam pass, and viterbi_finish_kernel, which
// finalises the utterances it decoded to their last frame.  Included by viterbi.hip only.
#pragma once
#include "viterbi_common.hpp"
#include "viterbi_eps.hpp"

namespace {

// Dynamic-LDS layout of viterbi_small_kernel: byte offsets in carve order and the total.  The kernel takes its pointers
// from it, align_impl the launch's LDS size.  As viterbi_kernel's carve with its token capacity fixed at N = 64 and a
// 256-entry table; no staged score row: a candidate reads its score straight from L2 — measured faster than that kernel's
// LDS row cache here, and 2 KB less LDS per wavefront leaves room for a scoring workgroup next to sixteen of these.
// P: unsigned char * in the kernel (the start of its dynamic LDS: the members are the arrays), size_t on the host (0: the
// members are byte offsets, `end` the launch's dynamic-LDS bytes).
template <class P>
struct SmallLds {
  P s_cost, l_cost0, hmap, s_state, s_F, s_W, t_cbase, s_an, s_bucket, l_state0, l_an0, cntord, ctr, bm, eps, end;
  __host__ __device__ SmallLds(P at, int N, int C, bool with_eps) {
    auto take = [&](size_t bytes) { const P r = at; at += bytes; return r; };
    const size_t n4 = (size_t)N * 4;
    s_cost = take(2 * n4);
    l_cost0 = take(4 * n4);
    hmap = take(256 * 4);
    s_state = take(n4);
    s_F = take(n4);
    s_W = take(n4);
    t_cbase = take(n4);
    s_an = take(n4);
    s_bucket = take(n4);
    l_state0 = take(2 * n4);
    l_an0 = take(2 * n4);
    cntord = take((size_t)C * 4);               // [C]: owner map of the candidate ordinals, then bucket sizes → exclusive sums
    ctr = take(16);
    bm = take((size_t)kBmWords * 4);
    eps = take(with_eps ? kEpsWordsPerSlot * n4 : 0);
    end = at;
  }
};

// First tier of the windowed first-beam pass (mfa_align_features_batch), written for what that tier actually sees: at
// most 64 live tokens (one per lane) and at most 64·kRounds candidates per frame (one per lane and round).  Same decoder,
// same decisions, bit for bit — but straight-line wavefront code: viterbi_kernel (viterbi_wave.hpp) carries a token-chunk loop, an
// arc cache of eight per lane, an HBM candidate stash and the retry/grow bookkeeping through every frame (6 000
// instructions, 139 spilled scalars), this one a third of that.  Anything outside its envelope (more tokens, more
// candidates, a state of more than 64 arcs) hands the utterance over to the table-growth list pass (ST_GROW).  An utterance
// that reaches its last frame is parked with done = 2; viterbi_finish_kernel then does ReachedFinal, traceback and outputs.
//   GetCutoff's min_active rule: the (min_active + 1 − k)-th smallest cost outside the beam by ballot quickselect (a
//   handful of compare+ballot steps) instead of ranking every token against every other.
constexpr int kSmallN = 64;
template <int kRounds, bool kEps = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void viterbi_small_kernel(VitParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int N = kSmallN, C = 64 * kRounds;
  constexpr u32 HM = 256u, hmask = Hash256::mask;
  const int lane = threadIdx.x;
  const int utt = blockIdx.x;
  const VitState vs0 = p.w_vstate[utt];
  // an utterance whose speculative window failed is one window behind from then on (VitState.pad0): this launch redoes
  // that window for it — scored again with the proven band by the scoring launch before this one — without the check
  const int K_ = p.t_end - p.t_begin;
  const int lag = (p.t_begin > 0 && vs0.pad0 != 0) ? 1 : 0;
  const int t_begin_u = p.t_begin - lag * K_;
  const bool resume = t_begin_u > 0;
  if (p.t_begin > 0 && vs0.done) return;           // finished (or failed, or waiting for the finish kernel)
  const int64_t so = p.g.d_state_off[utt];
  const int S = (int)(p.g.d_state_off[utt + 1] - so);
  const int64_t ab_ = p.g.d_arc_base[utt];
  const int32_t *arc_off = p.g.d_arc_off + so + utt;
  const uint4 *a_rec = p.w_arcnext + ab_;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const float *ll = p.ll + p.ll_off[utt];
  const int P = p.ll_cols[utt];
  // parked lists: the host lays this launch's workspace out for nmax = kSmallN tokens
  u32 *park_state = p.w_state + (size_t)utt * 2 * N;
  u32 *park_an = p.w_state + (size_t)p.g.n_utt * 2 * N + (size_t)utt * 2 * N;
  double *park_cost = p.w_cost + (size_t)utt * 2 * N;
  // Outside this kernel's envelope (more than 64 tokens, more than 64·kRounds candidates, a malformed graph): the utterance
  // leaves the fast track for good and is decoded from its first frame by the table-growth list pass that follows the
  // windowed pass (general kernel, the caller's full capacity) — rare: none of the 4 096 utterances of the bench workload
  // ever holds more than 64 tokens at beam 10.
  auto hand_over = [&]() {
    if (lane != 0) return;
    VitState vs; vs.n = 0; vs.cur = 0; vs.done = 1; vs.pad0 = 0; vs.H = 1000u; vs.pad1 = 0; vs.bp_used = 0;
    p.w_vstate[utt] = vs;
    p.status[utt] = ST_GROW; p.n_words[utt] = 0; p.like[utt] = 0.0f;
  };

  int n = 1, t = 0;
  u32 H = 1000u;
  u64 bp_used = 0;
  const int start = p.g.d_start[utt];
  if (S <= 0 || start < 0 || start >= S || T <= 0) { hand_over(); return; }   // (the general kernel reports the failure)
  if (resume) {
    n = vs0.n; H = vs0.H; bp_used = vs0.bp_used; t = t_begin_u;
    if (n > N || n <= 0) { hand_over(); return; }
  }

  // ---- LDS carve (SmallLds)
  const SmallLds<unsigned char *> lds(smem, N, C, kEps);
  u64 *s_cost = (u64 *)lds.s_cost;
  double *l_cost0 = (double *)lds.l_cost0;
  u32 *hmap = (u32 *)lds.hmap;
  u32 *s_state = (u32 *)lds.s_state;
  u32 *s_F = (u32 *)lds.s_F;
  u32 *s_W = (u32 *)lds.s_W;
  u32 *t_cbase = (u32 *)lds.t_cbase;
  u32 *s_an = (u32 *)lds.s_an;
  u32 *s_bucket = (u32 *)lds.s_bucket;
  u32 *l_state0 = (u32 *)lds.l_state0;
  u32 *l_an0 = (u32 *)lds.l_an0;
  u32 *cntord = (u32 *)lds.cntord;
  u32 *ctr = (u32 *)lds.ctr;
  u32 *bm = (u32 *)lds.bm;
  // the epsilon closures' (kEps) arrays and their view of the slot table
  const EpsArrays e(lds.eps, N);
  const SlotTable<Hash256> tab{hmap, ctr, N, s_state, s_an, s_cost, s_F, s_W, s_bucket, {}};

  u64 *bp = p.w_bp + (size_t)f0 * p.bpf;
  const u64 bp_cap = (u64)T * (u64)p.bpf;
  u32 *tokoff = p.w_tokoff + f0 + utt;

  for (u32 i = lane; i < HM; i += 64) hmap[i] = kEmpty;
  for (int i = lane; i < C; i += 64) cntord[i] = 0;
  if (lane == 0) ctr[0] = 0;
  if constexpr (kEps) e.tmp[lane] = 0xFFFFFFFFu;
  int cur = 0;
  if (!resume) {
    if constexpr (kEps) {
      n = init_closure(p, utt, lane, start, so, arc_off, a_rec, H, tab, e, l_state0, l_cost0, l_an0, bp);
      if (n < 0) { hand_over(); return; }
      bp_used = (u64)n;
    } else {
      if (lane == 0) { l_state0[0] = (u32)start; l_cost0[0] = 0.0; l_an0[0] = ((u32)arc_off[start] << 7) | (u32)(arc_off[start + 1] - arc_off[start]); }
    }
  } else if (lane < n) {
    l_state0[lane] = park_state[lane]; l_an0[lane] = park_an[lane]; l_cost0[lane] = park_cost[lane];
  }
  const int t_stop = min(T, t_begin_u + K_);
  WSYNC();
  const bool spec = p.spec != 0 && lag == 0;
  if (spec) build_scored_bitmap(p, utt, lane, bm);

  bool overflow = false, spec_fail = false;
  bool have_best = false;
  double best_carry = 0.0;
  for (; t < t_stop; t++) {
    const float *llt = ll + (size_t)t * P;
    u32 *n_state = l_state0 + (cur ^ 1) * N;
    u32 *c_an = l_an0 + cur * N, *n_an = l_an0 + (cur ^ 1) * N;
    double *c_cost = l_cost0 + cur * N, *n_cost = l_cost0 + (cur ^ 1) * N;
    // ---------------- GetCutoff
    const double cst = lane < n ? c_cost[lane] : INFINITY;
    const u32 an = lane < n ? c_an[lane] : 0u;
    // The cheapest token's cost is the cheapest candidate of the previous frame (the global minimum is always created and
    // wins its slot, and a slot's cost is its candidate's, bit for bit): carried over instead of a wavefront reduction.
    const double best = (have_best && !kEps) ? best_carry : wave_min_f64(cst);   // (a closure token can undercut every candidate)
    const u32 best_i = (u32)__ffsll((long long)__ballot(lane < n && cst == best)) - 1u;
    double wcut = INFINITY; float abeam = INFINITY;
    if (n > kMinActive) {
      const double beam_cut = best + p.beam;
      const u64 inside = __ballot(lane < n && cst <= beam_cut);
      const int kle = __popcll(inside);
      if (kle > kMinActive) { wcut = beam_cut; abeam = p.beam; }
      else {
        // the (min_active + 1 − kle)-th smallest cost outside the beam: ballot quickselect (ties resolved by counting < and <=)
        u64 A = __ballot(lane < n) & ~inside;
        int r = kMinActive + 1 - kle;
        double v = INFINITY;
        while (A != 0ull) {
          const int pl = __ffsll((long long)A) - 1;
          const double pv = readlane_f64(cst, pl);
          const u64 lt = __ballot(cst < pv) & A, le = __ballot(cst <= pv) & A;
          const int clt = __popcll(lt), cle = __popcll(le);
          if (r <= clt) A = lt;
          else if (r <= cle) { v = pv; break; }
          else { A &= ~le; r -= cle; }
        }
        wcut = v;
        abeam = (float)(v - best + (double)kBeamDelta);
      }
    }
    { u32 want = (u32)((float)n * kHashRatio); if (want > H) H = want; }
    // ---------------- candidate layout: ordinal base per token, owner of every ordinal
    const bool act = lane < n && cst < wcut;
    const u32 narc = act ? (an & 127u) : 0u;
    const u32 narc_incl = incl_scan_sum(narc);
    const u32 cb = narc_incl - narc;
    const u32 ctot = (u32)__builtin_amdgcn_readlane((int)narc_incl, 63);
    if (__any(narc > (u32)kMaxArcsPerState) || ctot > (u32)C) { overflow = true; break; }
    if (lane < n) t_cbase[lane] = cb;
    if (narc > 0u) cntord[cb] = (u32)lane + 1u;       // head of each token's candidate run (cntord is all zero between frames)
    WSYNC();
    const int rounds = (int)((ctot + 63u) >> 6);
    // ---------------- arc gather (all rounds' loads in flight together)
    u32 cidx[kRounds], nx[kRounds], nan_[kRounds]; int colv[kRounds]; float wv[kRounds]; double tcost[kRounds];
    {
      u32 carry = 0;
#pragma unroll
      for (int r = 0; r < kRounds; r++) {
        cidx[r] = 0; nx[r] = 0; nan_[r] = 0; colv[r] = 0; wv[r] = 0.0f; tcost[r] = INFINITY;
        if (r < rounds) {   // uniform
          const u32 c = (u32)lane + 64u * r;
          const u32 own = max(incl_scan_max(cntord[c]), carry);
          carry = (u32)__builtin_amdgcn_readlane((int)own, 63);
          const bool valid = c < ctot;
          const u32 tok = valid ? own - 1u : 0u;
          tcost[r] = valid ? c_cost[tok] : INFINITY;
          const u32 tan = c_an[tok];
          const u32 k_ = valid ? c - t_cbase[tok] : 0u;
          cidx[r] = (tok << kArcBits) | k_;            // (token, arc) of the candidate: what the winner records
          if (valid) { const uint4 rec = a_rec[(tan >> 7) + k_]; nx[r] = rec.x; nan_[r] = rec.y; colv[r] = (int)rec.z; wv[r] = __uint_as_float(rec.w); }
        }
      }
    }
    WSYNC();
    if (spec) {   // every score read below must be one that was computed for this window
      bool viol = false;
#pragma unroll
      for (int r = 0; r < kRounds; r++) viol |= (u32)lane + 64u * r < ctot && !column_scored(bm, colv[r]);
      if (__any(viol)) { spec_fail = true; break; }
    }
    const u32 cb2 = t_cbase[min(lane, N - 1)];        // (= cb for the lanes that hold a token; re-read: one register less across the gather)
    if (narc > 0u) cntord[cb2] = 0u;                  // owner map read by every round: back to zero for the ordering pass
    double nw[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; r++)
      nw[r] = ((u32)lane + 64u * r < ctot) ? cand_cost(wv[r], tcost[r], llt[colv[r]], p.scale) : INFINITY;
    // ---------------- running cutoff: seed from the best token's candidates, then an exclusive prefix-min in ordinal order
    // (the best token's candidates sit at ordinals cb[best] .. + narc[best]: a few broadcast reads instead of a masked
    //  wavefront reduction per round)
    double run = INFINITY;
    {
      const u32 ob = (u32)__builtin_amdgcn_readlane((int)cb2, (int)best_i), nb_ = (u32)__builtin_amdgcn_readlane((int)narc, (int)best_i);
      for (u32 k = 0; k < nb_; k++) {
        const u32 ord = ob + k;
        const int ln = (int)(ord & 63u);
        double v = readlane_f64(nw[0], ln);
#pragma unroll
        for (int r = 1; r < kRounds; r++) if ((ord >> 6) == (u32)r) v = readlane_f64(nw[r], ln);
        run = min_f64(run, v);
      }
    }
    bool created[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
      created[r] = false;
      if (r < rounds) {
        const double m_incl = incl_scan_min(nw[r]);
        const double local = min_f64(run, shift_in_min(m_incl));
        run = min_f64(run, readlane_f64(m_incl, 63));
        created[r] = ((u32)lane + 64u * r < ctot) && nw[r] < local + (double)abeam;
      }
    }
    // ---------------- find-or-insert the destination's slot, lower its cost / first creator, settle the winner
    u32 sl[kRounds], hk[kRounds];
    bool pend[kRounds];
    bool any_pend = false;
#pragma unroll
    for (int r = 0; r < kRounds; r++) { sl[r] = kEmpty; pend[r] = created[r]; hk[r] = tab.hash(nx[r]); any_pend |= pend[r]; }
    while (__any(any_pend)) {
      any_pend = false;
#pragma unroll
      for (int r = 0; r < kRounds; r++) {
        if (r >= rounds) continue;      // (uniform: a frame of one round does not walk the other rounds' masks)
        if (pend[r]) {
          const u32 v = hmap[hk[r]];
          if (v == kEmpty) {
            if (atomicCAS(&hmap[hk[r]], kEmpty, kClaim) == kEmpty) {
              const u32 my = atomicAdd(&ctr[0], 1u);
              if (my < (u32)N) {
                s_state[my] = nx[r]; s_an[my] = nan_[r]; s_cost[my] = kKeyInf; s_F[my] = kEmpty; s_W[my] = kEmpty; s_bucket[my] = hk[r];
                hmap[hk[r]] = my;
                sl[r] = my;
              } else {
                hmap[hk[r]] = kOver;
              }
              pend[r] = false;
            }
          } else if (v == kOver) {
            pend[r] = false;
          } else if (v != kClaim) {
            if (s_state[v] == nx[r]) { sl[r] = v; pend[r] = false; }
            else hk[r] = (hk[r] + 1u) & hmask;
          }
        }
        any_pend |= pend[r];
      }
      WSYNC();
      if (ctr[0] > (u32)N) break;
    }
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
      if (r < rounds && sl[r] != kEmpty) { atomicMin(&s_cost[sl[r]], dkey(nw[r])); atomicMin(&s_F[sl[r]], cidx[r]); }
    }
    WSYNC();
#pragma unroll
    for (int r = 0; r < kRounds; r++)
      if (r < rounds && sl[r] != kEmpty && dkey(nw[r]) == s_cost[sl[r]]) atomicMin(&s_W[sl[r]], cidx[r]);
    WSYNC();
    const u32 nslots = ctr[0];
    if (nslots > (u32)N || bp_used + nslots > bp_cap) { overflow = true; break; }
    if (nslots == 0) { n = 0; t++; break; }            // everything pruned: no surviving token
    // ---------------- Kaldi list order of the new tokens (one slot per lane): ordinal of the hash bucket's first creator and
    // rank inside the bucket; bucket sizes at the leaders' ordinals, then exclusive sums = where every bucket starts.
    // (kEps: slots created by the epsilon closure carry ordinals past the candidates': s_F = 0x80000000 | k.)
    u32 aux = 0;
    auto order_lanes = [&](u32 ns, u32 n_ord) {
      aux = 0;
      if ((u32)lane < ns) {
        const u32 d = s_state[lane], Fj = s_F[lane];
        u32 Fb = Fj, nb = 1, rank = 0;
        if ((u32)S > H) {
          nb = 0;
          for (u32 m = d % H; m < (u32)S; m += H) {
            u32 h = tab.hash(m), sm = kEmpty;
            for (;;) {
              const u32 v = hmap[h];
              if (v == kEmpty) break;
              if (v < (u32)N && s_state[v] == m) { sm = v; break; }
              h = (h + 1u) & hmask;
            }
            if (sm < (u32)N) {
              const u32 Fm = s_F[sm];
              nb++;
              if (Fm < Fj) rank++;
              if (Fm < Fb) Fb = Fm;
            }
          }
        }
        u32 ord_b = t_cbase[(Fb >> kArcBits) & (u32)(N - 1)] + (Fb & (kMaxArcsPerState - 1));
        if constexpr (kEps) { if (Fb >> 31) ord_b = ctot + (Fb & 0x7FFFFFFFu); }
        aux = (rank << 24) | ord_b;
        if (Fb == Fj) cntord[ord_b] = nb;
      }
      WSYNC();
      {
        u32 carry = 0;
        const int rounds_ord = (int)((n_ord + 63u) >> 6);
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
          if (r < rounds_ord) {
            const u32 o = (u32)lane + 64u * r;
            const u32 v = cntord[o];
            const u32 inc = incl_scan_sum(v);
            if (v != 0) cntord[o] = carry + inc - v;
            carry += (u32)__builtin_amdgcn_readlane((int)inc, 63);
          }
        }
      }
      WSYNC();
    };
    order_lanes(nslots, ctot);
    u32 nslots_f = nslots;
    if constexpr (kEps) {
      // ---------------- FasterDecoder::ProcessNonemitting(next_weight_cutoff): process_nonemitting() after the stack fill
      const double eps_cut = run + (double)abeam;
      u32 my_info = 0;
      if ((u32)lane < nslots) { my_info = p.w_epsinfo[(size_t)utt * p.eps_stride + s_state[lane]]; e.info[lane] = my_info; }
      if (__any((my_info & 127u) != 0u)) {
        bool eps_broken = false;
        if ((u32)lane < nslots) {
          const u32 pos = cntord[aux & 0xFFFFFFu] + (aux >> 24);
          if (pos < nslots) e.inv[pos] = (u32)lane; else eps_broken = true;
        }
        if (__any(eps_broken)) { overflow = true; break; }
        WSYNC();
        u32 sp = 0;
        {
          const u32 j = (u32)lane < nslots ? e.inv[lane] : 0u;
          const bool has = (u32)lane < nslots && (e.info[j] & 127u) != 0u;
          const u64 m = __ballot(has);
          if (has) e.stk[(u32)__popcll(m & ((1ull << lane) - 1ull))] = j;
          sp = (u32)__popcll(m);
        }
        WSYNC();
        u32 eord;
        if (process_nonemitting(p, utt, lane, a_rec, tab, e, eps_cut, sp, ctot, (u32)C, eord) != kEpsDone) { overflow = true; break; }
        nslots_f = ctr[0];
        if (nslots_f > (u32)N || bp_used + nslots_f > bp_cap) { overflow = true; break; }
        if (nslots_f > nslots) {
          // new states: the list order is worked out again over all slots (a new state goes to the end of its bucket's chain)
          if ((u32)lane < nslots) cntord[aux & 0xFFFFFFu] = 0u;
          WSYNC();
          order_lanes(nslots_f, ctot + eord);
        }
      }
    }
    // ---------------- write the new list + back-pointers, reset the tables
    bool broken = false;
    if constexpr (kEps) {
      if ((u32)lane < nslots_f) e.pos[lane] = cntord[aux & 0xFFFFFFu] + (aux >> 24);
      WSYNC();
    }
    if ((u32)lane < nslots_f) {
      const u32 pos = cntord[aux & 0xFFFFFFu] + (aux >> 24);
      const u32 d = s_state[lane], W = s_W[lane];
      bool eps_w = false;
      if constexpr (kEps) eps_w = (W >> 31) != 0u;
      if (eps_w) {
        // the token came over an epsilon arc: its predecessor is a token of THIS frame's list (no frame consumed)
        const u32 src = W & 0x7FFFFFFFu;
        if (pos >= nslots_f || src >= nslots_f || d >= (u32)S) broken = true;
        else {
          n_state[pos] = d;
          n_an[pos] = s_an[lane];
          n_cost[pos] = dunkey(s_cost[lane]);
          bp[bp_used + pos] = ((u64)e.arc[lane] << 32) | (u64)e.pos[src];
        }
      } else {
        const u32 ppos = W >> kArcBits, k = W & (kMaxArcsPerState - 1);
        if (pos >= nslots_f || ppos >= (u32)n || d >= (u32)S) broken = true;
        else {
          const u32 arc = (c_an[ppos] >> 7) + k;
          n_state[pos] = d;
          n_an[pos] = s_an[lane];
          n_cost[pos] = dunkey(s_cost[lane]);
          bp[bp_used + pos] = ((u64)arc << 32) | (u64)ppos;
        }
      }
    }
    if (__any(broken)) { overflow = true; break; }     // (cannot happen; the list pass would report ST_INTERNAL)
    WSYNC();
    if ((u32)lane < nslots_f) { hmap[s_bucket[lane]] = kEmpty; cntord[aux & 0xFFFFFFu] = 0; }
    if (lane == 0) { tokoff[t] = (u32)bp_used; ctr[0] = 0; }
    bp_used += nslots_f;
    n = (int)nslots_f;
    cur ^= 1;
    best_carry = run; have_best = true;
    WSYNC();
  }
  if (overflow) { hand_over(); return; }
  // the narrow band did not hold.  Nothing parked has been touched (lists and decoder state are written at a window's END
  // only; the back-pointer records of this window are simply written again), so the parked state is as it was at the
  // window's start: mark the utterance as one window behind — the next scoring launch scores this window again with the
  // proven band, the next launch of this kernel redoes it (no separate launch for a handful of wavefronts, which with
  // several batches in flight left the chip empty a tenth of the time)
  if (spec_fail) {
    if (lane == 0) {
      VitState vs = vs0;
      if (!resume) { vs.n = 1; vs.cur = 0; vs.H = 1000u; vs.pad1 = 0; vs.bp_used = 0; }   // (window 0: nothing was parked yet)
      vs.done = 0; vs.pad0 = 1;
      p.w_vstate[utt] = vs;
    }
    return;
  }
  __threadfence_block();
  u32 *c_state = l_state0 + cur * N;
  double *c_costp = l_cost0 + cur * N;
  const u32 *c_anp = l_an0 + cur * N;
  if (n == 0) {   // no surviving token: pending for the retry pass, as the general kernel's finalisation reports it
    if (lane == 0) {
      VitState vs; vs.n = 0; vs.cur = 0; vs.done = 1; vs.pad0 = lag; vs.H = H; vs.pad1 = 0; vs.bp_used = bp_used;
      p.w_vstate[utt] = vs;
      p.w_hash[utt] = H;
      p.status[utt] = ST_PENDING; p.n_words[utt] = 0; p.like[utt] = 0.0f;
    }
    return;
  }
  // ---------------- park the list (window end, or last frame: done = 2 hands the utterance to viterbi_finish_kernel)
  u32 dmax = 0, dmin_inv = 0;
  if (lane < n) {
    const u32 s_ = c_state[lane];
    park_state[lane] = s_; park_an[lane] = c_anp[lane]; park_cost[lane] = c_costp[lane];
    if (p.state_depth && t < T) {
      const int32_t *sd = p.state_depth + 2 * (so + (int64_t)s_);
      dmax = (u32)sd[0]; dmin_inv = ~(u32)sd[1];
    }
  }
  dmax = wave_max_u32(dmax);
  dmin_inv = wave_max_u32(dmin_inv);
  if (lane == 0) {
    VitState vs;
    vs.n = n; vs.cur = 0; vs.done = t < T ? 0 : 2; vs.pad0 = lag; vs.H = H; vs.pad1 = 0; vs.bp_used = bp_used;
    p.w_vstate[utt] = vs;
    if (t >= T) p.w_hash[utt] = H;
    if (p.band && t < T) publish_band(p, utt, dmax, dmin_inv);
  }
}

// ReachedFinal, traceback and outputs for the utterances viterbi_small_kernel decoded to their last frame (done = 2).
__global__ __launch_bounds__(64) void viterbi_finish_kernel(VitParams p) {
  const int lane = threadIdx.x;
  const int utt = blockIdx.x;
  const VitState vs = p.w_vstate[utt];
  if (vs.done != 2) return;
  const int64_t so = p.g.d_state_off[utt];
  const int64_t ab_ = p.g.d_arc_base[utt];
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const u32 *c_state = p.w_state + (size_t)utt * 2 * kSmallN;   // parked with viterbi_small_kernel's stride
  const double *c_cost = p.w_cost + (size_t)utt * 2 * kSmallN;
  if (lane == 0) { VitState d = vs; d.done = 1; p.w_vstate[utt] = d; }
  finalize_utterance(p, utt, lane, ST_OK, T, T, vs.n, c_state, c_cost, p.g.d_final + so, p.w_bp + (size_t)f0 * p.bpf,
                     p.w_tokoff + f0 + utt, f0, ab_, p.g.d_arc_weight + ab_, p.g.d_arc_col + ab_, p.ll + p.ll_off[utt],
                     p.ll_cols[utt], p.w_epsinfo != nullptr, vs.bp_used, (u64)T * (u64)p.bpf);
}

}  // namespace
