// viterbi_kernel: the general wavefront-per-utterance frame loop (any token capacity; token lists in LDS or HBM).
// Included by viterbi.hip only.
#pragma once
#include "viterbi_common.hpp"
#include "viterbi_eps.hpp"

namespace {

constexpr int kArcCache = 8;  // arcs per token kept in registers during expansion (deeper states take a slow tail loop)

// kListsInLds: the two token lists (state, cost) live in LDS (fast path) or, for graphs/beams whose tables would not
// fit in 160 KiB, in the per-utterance HBM workspace.
// (waves_per_eu 4: at most 128 VGPRs, so that the 9.5 KB first tier really gets its 16 wavefronts per CU)
// kEps: the instantiation for batches that hold graphs with epsilon input arcs (g.d_state_nemit): every frame's emitting phase
// is followed by FasterDecoder::ProcessNonemitting — see the closure block in the frame loop.  The epsilon-free instantiation
// is the code it always was.
template <bool kListsInLds, bool kEps = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void viterbi_kernel(VitParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  int utt = blockIdx.x;
  if (p.utt_list) {
    if (p.n_list && (int)blockIdx.x >= *p.n_list) return;
    utt = p.utt_list[blockIdx.x];
  }
  const int64_t so = p.g.d_state_off[utt];
  const int S = (int)(p.g.d_state_off[utt + 1] - so);
  const int64_t ab_ = p.g.d_arc_base[utt];
  const int32_t *arc_off = p.g.d_arc_off + so + utt;
  const float *final_w = p.g.d_final + so;
  const float *a_w = p.g.d_arc_weight + ab_;
  const int32_t *a_col = p.g.d_arc_col + ab_;
  const uint4 *a_rec = p.w_arcnext + ab_;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const float *ll = p.ll + p.ll_off[utt];
  const int P = p.ll_cols[utt];
  const int N = p.nmax, C = p.cmax;

  // ---- LDS carve (8-byte items first).  These tables carry values between lanes of ONE wavefront: LDS operations of
  // a wavefront execute in program order, so plain accesses are enough provided the compiler keeps them on the right
  // side of each hand-over point — that is what WSYNC() (a wavefront-scope fence pair + scheduling barrier) is for.
  // Within a phase the loads stay free to be issued back to back (the volatile version of round 1 waited on every one).
  // The host sizes the launch's LDS with lds_bytes() (viterbi.hip), a second statement of this layout kept by hand: an
  // array added here needs its term there.
  u64 *s_cost = (u64 *)smem;                  // [N] best cost key per slot
  double *l_cost0 = kListsInLds ? (double *)(s_cost + N)   // [2][N] token costs (current / next list)
                                         : (double *)(p.w_cost + (size_t)utt * 2 * N);
  // state → slot: an open-addressing hash table (linear probing) over the states that received a candidate THIS frame —
  // at most N of them, whatever the size of the graph, so the table is 4N entries instead of one per graph state
  // (round 1: a direct map, 10.8 KB of the 23 KB a 2 700-state graph needed → 6 wavefronts per CU; now 16).
  u32 *hmap = (u32 *)(s_cost + (kListsInLds ? 3 : 1) * (size_t)N);  // [HM] slot index | kEmpty | kClaim | kOver
  // (large tiers, whose 4N-entry table would be bigger than one entry per graph state, address the table by state id:
  //  hbits = 0 — same code, no collisions)
  const bool hdirect = p.hbits == 0;
  const u32 HM = hdirect ? (u32)((S + 1) & ~1) : 1u << p.hbits, hmask = hdirect ? 0xFFFFFFFFu : HM - 1u;
  const int hshift = hdirect ? 0 : 32 - p.hbits;
  u32 *s_state = hmap + HM;         // [N]
  u32 *s_F = s_state + N;           // [N] first creating candidate (pos<<6|k)
  u32 *s_W = s_F + N;               // [N] winning candidate
  u32 *s_aux = s_W + N;             // [N] (rank<<24)|ordinal of the bucket leader's first candidate
  u32 *t_cbase = s_aux + N;         // [N] candidate ordinal base per source token
  u32 *s_an = t_cbase + N;          // [N] (first arc << 7 | out-degree) of the slot's state
  u32 *s_bucket = s_an + N;         // [N] hash bucket the slot's state was filed under (reset at the end of the frame)
  u32 *l_state0 = kListsInLds ? s_bucket + N : (u32 *)(p.w_state + (size_t)utt * 2 * N);  // [2][N] token states
  u32 *l_an0 = kListsInLds ? l_state0 + 2 * N : (u32 *)(p.w_state + (size_t)p.g.n_utt * 2 * N + (size_t)utt * 2 * N);
  u32 *cntord = s_bucket + N + (kListsInLds ? 4 * N : 0);  // [C] bucket sizes at leader ordinals → exclusive sums
  float *ll_row = (float *)(cntord + C);      // [llcap] this frame's score row
  u32 *ctr = (u32 *)(ll_row + p.llcap);       // [2]: nslots, nstash
  u32 *bm = ctr + 4;                          // [kBmWords] columns scored for this window (speculative look-ahead only)
  // the epsilon closures' (kEps) arrays and their view of the slot table
  const EpsArrays e((unsigned char *)(bm + kBmWords), N);
  const SlotTable<HashRuntime> tab{hmap, ctr, N, s_state, s_an, s_cost, s_F, s_W, s_bucket, {hdirect, hmask, hshift}};
  if constexpr (kEps) {
    for (int i = lane; i < N; i += 64) e.tmp[i] = 0xFFFFFFFFu;
  }

  u32 *st_a = p.w_stash_a + (size_t)utt * C;
  u32 *st_b = p.w_stash_b + (size_t)utt * C;
  u64 *st_key = p.w_stash_key + (size_t)utt * C;
  u64 *bp = p.w_bp + (size_t)f0 * p.bpf;
  const u64 bp_cap = (u64)T * (u64)p.bpf;
  u32 *tokoff = p.w_tokoff + f0 + utt;

  for (u32 i = lane; i < HM; i += 64) hmap[i] = kEmpty;
  for (int i = lane; i < C; i += 64) cntord[i] = 0;
  if (lane == 0) { ctr[0] = 0; ctr[1] = 0; }

  int status = ST_OK;
  const int start = p.g.d_start[utt];
  if (S <= 0 || start < 0 || start >= S || T <= 0) status = ST_FAILED;
  const bool resume = p.windowed && p.t_begin > 0;
  int cur = 0, n = 1;
  u32 H = p.pass == 0 ? 1000u : p.w_hash[utt];
  u64 bp_used = 0;
  int t = 0;
  // token lists parked in HBM between windows (the kListsInLds = false variant keeps them there all the time)
  u32 *park_state = p.w_state + (size_t)utt * 2 * N;
  u32 *park_an = p.w_state + (size_t)p.g.n_utt * 2 * N + (size_t)utt * 2 * N;
  double *park_cost = p.w_cost + (size_t)utt * 2 * N;
  if (!resume) {
    // InitDecoding: one token at the start state with cost 0 (epsilon-free graphs: ProcessNonemitting is a no-op)
    if (lane == 0) {
      const int s0 = start < 0 || start >= S ? 0 : start;
      l_state0[0] = (u32)s0; l_cost0[0] = 0.0;
      u32 deg0 = S > 0 ? (u32)(arc_off[s0 + 1] - arc_off[s0]) : 0u;
      if constexpr (kEps) { if (S > 0 && p.g.d_state_nemit) deg0 = (u32)p.g.d_state_nemit[so + s0]; }
      l_an0[0] = S > 0 ? ((u32)arc_off[s0] << 7) | min(deg0, 127u) : 0u;
    }
    if constexpr (kEps) {
      if (status == ST_OK) {
        const int n0 = init_closure(p, utt, lane, start, so, arc_off, a_rec, H, tab, e, l_state0, l_cost0, l_an0, bp);
        if (n0 < 0) status = ST_TOKEN_OVERFLOW;
        else { n = n0; bp_used = (u64)n0; }
      }
    }
  } else {
    const VitState vs = p.w_vstate[utt];
    if (vs.done) return;                           // finished (or failed) in an earlier window: outputs are final
    n = vs.n; H = vs.H; bp_used = vs.bp_used; t = p.t_begin;
    if (n < 0 || n > N) { n = 0; status = ST_INTERNAL; }
    if (kListsInLds) {
      cur = 0;
      for (int i = lane; i < n; i += 64) { l_state0[i] = park_state[i]; l_an0[i] = park_an[i]; l_cost0[i] = park_cost[i]; }
    } else {
      cur = vs.cur & 1;
    }
  }
  const int t_stop = p.windowed ? min(T, p.t_end) : T;
  // score rows are staged through LDS one frame ahead (registers hold row t+1 while frame t is processed)
  constexpr int kPre = 8;
  const bool row_cached = P <= p.llcap && P <= 64 * kPre;
  float pre[kPre];
#pragma unroll
  for (int r = 0; r < kPre; r++) pre[r] = (row_cached && t < T && lane + 64 * r < P) ? ll[(size_t)t * P + lane + 64 * r] : 0.0f;
  WSYNC();
  const bool spec = p.spec != 0 && p.windowed;
  if (spec) build_scored_bitmap(p, utt, lane, bm);
  bool viol = false;   // a score outside the scored columns was read this window

  VitStamps stamps;
  stamps.start();
  for (; t < t_stop && status == ST_OK; t++) {
    const float *llt = ll + (size_t)t * P;
    // The frame's score row moves registers → LDS right before its first use, not here: on this target stores count in
    // vmcnt like loads and retire in order, so a wait for the row (requested during the previous frame) at the top of the
    // frame would also sit out the previous frame's back-pointer stores.  By the arc gather's wait they have long landed
    // (measured against staging the row at the top of the frame: 5.91 → 5.80 ms per 2 048 utterances).
    auto stage_row = [&]() {
      if (row_cached) {
#pragma unroll
        for (int r = 0; r < kPre; r++) if (lane + 64 * r < P) ll_row[lane + 64 * r] = pre[r];
        WSYNC();
      }
    };
    stamps.count(10, (unsigned long long)n);   // tokens entering the frame
    stamps.count(11, 1);                       // frames
    stamps.mark(0);   // score row staged
    // Two address spaces, two loads, never a pointer select: a select turns into a FLAT load, whose wait
    // (vmcnt(0) lgkmcnt(0)) drains every outstanding vector-memory operation — including the next row's prefetch.
    auto score = [&](int col) -> float {
      float v = ll_row[row_cached ? col : 0];   // LDS read, always (column 0 when the row is not staged)
      if (!row_cached) v = *(const volatile float *)&llt[col];  // rows wider than the LDS cache: straight from HBM/L2
      // (volatile: otherwise the two loads are merged back into one FLAT load of a selected address)
      if (spec) viol |= !column_scored(bm, col);
      return v;
    };
    // Next frame's score row: requested after this frame's last dependent global load (vmcnt retires in order, so a
    // prefetch issued before the arc gather would have to land before the gather's wait returns); it then has the
    // claim / order / write phases and the next GetCutoff to arrive.
    auto prefetch_next_row = [&]() {
      if (row_cached && t + 1 < t_stop) {   // (rows past the window are not scored yet)
        const float *nx_row = llt + P;
#pragma unroll
        for (int r = 0; r < kPre; r++) if (lane + 64 * r < P) pre[r] = nx_row[lane + 64 * r];
      }
    };
    u32 *n_state = l_state0 + (cur ^ 1) * N;
    u32 *c_an = l_an0 + cur * N, *n_an = l_an0 + (cur ^ 1) * N;
    double *c_cost = l_cost0 + cur * N, *n_cost = l_cost0 + (cur ^ 1) * N;
    // ---------------- GetCutoff: best cost (first index on ties), count
    double best = INFINITY; u32 best_i = kEmpty;
    for (int c0 = 0; c0 < n; c0 += 64) {
      int i = c0 + lane;
      double cst = i < n ? c_cost[i] : INFINITY;
      double m = wave_min_f64(cst);
      if (m < best) {  // uniform
        const u64 hit = __ballot(i < n && cst == m);
        best_i = (u32)c0 + (u32)__ffsll((long long)hit) - 1u;  // first index holding the minimum
        best = m;
      }
    }
    double wcut; float abeam;
    if (n <= kMinActive) { wcut = INFINITY; abeam = INFINITY; }
    else {
      const double beam_cut = best + p.beam;
      u32 kle = 0;
      for (int c0 = 0; c0 < n; c0 += 64) {
        int i = c0 + lane;
        kle += (u32)__popcll(__ballot(i < n && c_cost[i] <= beam_cut));
      }
      if (kle > (u32)kMinActive) { wcut = beam_cut; abeam = p.beam; }
      else {
        stamps.count(9, 1);   // frames that needed the exact min_active selection
        // sorted[min_active] (> beam_cut) = the smallest cost that has at least min_active+1 costs ≤ it
        double v = INFINITY;
        if (n <= 64) {  // costs are in registers: broadcast each with v_readlane, no LDS traffic
          const double cst = lane < n ? c_cost[lane] : INFINITY;
          u32 le = 0;
          for (int j = 0; j < n; j++) le += (readlane_f64(cst, j) <= cst) ? 1u : 0u;
          if (lane < n && le > (u32)kMinActive) v = cst;
        } else {
          for (int c0 = 0; c0 < n; c0 += 64) {
            int i = c0 + lane;
            double cst = i < n ? c_cost[i] : INFINITY;
            u32 le = 0;
            for (int j = 0; j < n; j++) le += (c_cost[j] <= cst) ? 1u : 0u;  // LDS broadcast reads
            if (i < n && le > (u32)kMinActive) v = min_f64(v, cst);
          }
        }
        v = wave_min_f64(v);
        wcut = v;
        abeam = (float)(v - best + (double)kBeamDelta);
      }
    }
    stamps.mark(1);   // GetCutoff
    // PossiblyResizeHash
    { u32 want = (u32)((float)n * kHashRatio); if (want > H) H = want; }

    // Candidate creation in three wavefront phases (each phase's LDS operations are issued back to back):
    //   look up the destination's slot → claim missing slots (CAS; the winner allocates, initialises, publishes)
    //   → re-read the published slot and lower its cost / first-creator with LDS atomics.
    // The hash and the claim step are SlotTable's (tab.hash, tab.probe: wavefront-collective loops below call probe in
    // rounds with a hand-over point between rounds).
    // read-only lookup (after every candidate of the frame has been filed): slot of state d, or kEmpty.  It stays a lambda
    // of this kernel (viterbi_small_kernel has its own): as a SlotTable member it changed the epsilon-free machine code.
    auto find = [&](u32 d) -> u32 {
      u32 h = tab.hash(d);
      for (;;) {
        const u32 v = hmap[h];
        if (v == kEmpty) return kEmpty;
        if (v < (u32)N && s_state[v] == d) return v;
        h = (h + 1u) & hmask;
      }
    };
    auto lower = [&](u32 s, double cnw, u32 cidx) {
      atomicMin(&s_cost[s], dkey(cnw));
      atomicMin(&s_F[s], cidx);
    };
    u32 cand_base = 0;
    bool bad_degree = false;
    bool used_stash = false;
    bool fast = false;
    double frame_min = INFINITY;   // (kEps) cheapest candidate of the frame: next_weight_cutoff = frame_min + adaptive_beam
    // ---------------- fast path (the common case): at most 64 tokens and at most 64 candidates this frame → ONE
    // candidate per lane.  The running cutoff is then a plain exclusive prefix-min across lanes, every candidate does one
    // arc fetch, one slot lookup, one claim/lower, and the winner check comes straight from its registers.
    if (n <= 64) {
      const double cst = lane < n ? c_cost[lane] : INFINITY;
      const u32 an = lane < n ? c_an[lane] : 0u;
      const bool act = lane < n && cst < wcut;
      const u32 narc = act ? (an & 127u) : 0u;
      const u32 narc_incl = incl_scan_sum(narc);
      const u32 cb = narc_incl - narc;
      const u32 ctot = (u32)__builtin_amdgcn_readlane((int)narc_incl, 63);
      if (ctot <= 64u) {
        fast = true;
        cand_base = ctot;
        if (lane < n) t_cbase[lane] = cb;
        s_aux[lane] = 0u;                       // s_aux is free until the ordering pass: owner map of the 64 ordinals
        WSYNC();
        if (narc > 0u) s_aux[cb] = (u32)lane + 1u;  // head of each token's candidate run
        WSYNC();
        stamps.mark(2);   // candidate layout (scan, owner map)
        const u32 tok1 = incl_scan_max(s_aux[lane]);
        const bool valid = (u32)lane < ctot;
        const u32 tok = valid ? tok1 - 1u : 0u;
        const double tcost = c_cost[tok];
        const u32 tan = c_an[tok];
        const u32 k = valid ? (u32)lane - t_cbase[tok] : 0u;
        const u32 a = (tan >> 7) + k;
        float w = 0.0f; int col = 0; u32 nx = 0u, nan_ = 0u;
        if (valid) { const uint4 rec = a_rec[a]; nx = rec.x; nan_ = rec.y; col = (int)rec.z; w = __uint_as_float(rec.w); }
        stage_row();
        const double nw = valid ? cand_cost(w, tcost, score(col), p.scale) : INFINITY;
        stamps.mark(3);   // arc gather + score + cost
        const double seed = wave_min_f64((valid && tok == best_i) ? nw : INFINITY);  // the best token's candidates
        const double m_incl = incl_scan_min(nw);
        const double local = min_f64(seed, shift_in_min(m_incl));
        if constexpr (kEps) frame_min = min_f64(seed, readlane_f64(m_incl, 63));
        const bool created = valid && nw < local + (double)abeam;
        const u32 cidx = (tok << kArcBits) | k;
        stamps.mark(4);   // running cutoff (seed, prefix-min)
        u32 sl = kEmpty;
        {
          bool pend = created; u32 h = tab.hash(nx);
          while (__any(pend)) {                           // slots are published before anybody re-reads
            tab.probe(pend, h, sl, nx, nan_);
            WSYNC();
            if (ctr[0] > (u32)N) break;                   // out of slots: the frame reports the overflow below
          }
        }
        if (sl != kEmpty) lower(sl, nw, cidx);
        WSYNC();  // every candidate of the frame has lowered its slot's cost
        if (sl != kEmpty && dkey(nw) == s_cost[sl]) atomicMin(&s_W[sl], cidx);
        stamps.mark(5);   // claim / lower / winner
      }
    }
    if (!fast) {
      stage_row();
      // ---------------- seed of the running cutoff: the best token's cheapest candidate.  With a single chunk it is
      // taken from the expansion's registers below; otherwise computed here.
      const bool single = n <= 64;
      double run = INFINITY;  // min over candidate costs seen so far (seed + earlier candidates)
      if (!single && best_i != kEmpty) {
        const u32 ban = c_an[best_i];
        const int a0 = (int)(ban >> 7), a1 = a0 + (int)(ban & 127u);
        double m = INFINITY;
        for (int a = a0 + lane; a < a1; a += 64) m = min_f64(m, cand_cost(a_w[a], best, score(a_col[a]), p.scale));
        run = wave_min_f64(m);
      }

      // ---------------- expand tokens in list order (general path: token per lane, arcs in a per-lane loop)
      used_stash = !single;
      for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const double cst = i < n ? c_cost[i] : INFINITY;
        const bool act = i < n && cst < wcut;
        int a0 = 0, narc = 0;
        if (act) { const u32 an = c_an[i]; a0 = (int)(an >> 7); narc = (int)(an & 127u); }
        if (narc > kMaxArcsPerState) bad_degree = true;
        const int maxarc = (int)wave_max_u32((u32)narc);
        if (maxarc > kArcCache) used_stash = true;
        const u32 narc_incl = incl_scan_sum((u32)narc);
        const u32 cb = cand_base + narc_incl - (u32)narc;
        if (i < n) t_cbase[i] = cb;
        cand_base += (u32)__builtin_amdgcn_readlane((int)narc_incl, 63);
        // arcs → registers (independent loads, one round trip), then their scores (second round trip)
        float w[kArcCache]; int col[kArcCache]; u32 nx[kArcCache]; u32 nan_[kArcCache]; double nw[kArcCache]; u32 sl[kArcCache];
  #pragma unroll
        for (int k = 0; k < kArcCache; k++) {
          w[k] = 0.0f; col[k] = 0; nx[k] = 0; nan_[k] = 0;
          if (k < narc) { const uint4 rec = a_rec[a0 + k]; nx[k] = rec.x; nan_[k] = rec.y; col[k] = (int)rec.z; w[k] = __uint_as_float(rec.w); }
        }
        double m = INFINITY;
  #pragma unroll
        for (int k = 0; k < kArcCache; k++) {
          nw[k] = (k < narc) ? cand_cost(w[k], cst, score(col[k]), p.scale) : INFINITY;
          m = min_f64(m, nw[k]);
          sl[k] = kEmpty;
        }
        for (int k = kArcCache; k < maxarc; k++)
          if (k < narc) m = min_f64(m, cand_cost(a_w[a0 + k], cst, score(a_col[a0 + k]), p.scale));
        if (single) run = best_i != kEmpty ? readlane_f64(m, __builtin_amdgcn_readfirstlane((int)best_i)) : INFINITY;  // best token is always expanded
        const double m_incl = incl_scan_min(m);
        double local = min_f64(run, shift_in_min(m_incl));
        run = min_f64(run, readlane_f64(m_incl, 63));

        // Candidate creation in three wavefront phases (each phase's LDS operations are issued back to back):
        //   look up the destination's slot → claim missing slots (CAS; the winner allocates, initialises, publishes)
        //   → re-read the published slot and lower its cost / first-creator with LDS atomics.
        bool cr[kArcCache]; u32 hk[kArcCache];
        bool any_pend = false;
  #pragma unroll
        for (int k = 0; k < kArcCache; k++) {
          cr[k] = (k < narc) && (nw[k] < local + (double)abeam);
          if (k < narc) local = min_f64(local, nw[k]);
          hk[k] = tab.hash(nx[k]);
          any_pend |= cr[k];
        }
        {
          bool pend[kArcCache];
  #pragma unroll
          for (int k = 0; k < kArcCache; k++) pend[k] = cr[k];
          while (__any(any_pend)) {     // all arcs of all tokens of the chunk are filed in the same rounds
            any_pend = false;
  #pragma unroll
            for (int k = 0; k < kArcCache; k++) {
              tab.probe(pend[k], hk[k], sl[k], nx[k], nan_[k]);
              any_pend |= pend[k];
            }
            WSYNC();
            if (ctr[0] > (u32)N) break;                   // out of slots: the frame reports the overflow below
          }
        }
  #pragma unroll
        for (int k = 0; k < kArcCache; k++) {
          if (k < maxarc) {  // uniform
            if (sl[k] != kEmpty) lower(sl[k], nw[k], ((u32)i << kArcBits) | (u32)k);
            if (!single && sl[k] != kEmpty) {
              u32 q = atomicAdd(&ctr[1], 1u);
              if (q < (u32)C) { st_a[q] = sl[k]; st_b[q] = ((u32)i << kArcBits) | (u32)k; st_key[q] = dkey(nw[k]); }
            }
          }
        }
        for (int k = kArcCache; k < maxarc; k++) {  // slow tail: states with more than kArcCache arcs
          bool created = false; double cnw = 0.0; u32 d = 0, dan = 0;
          if (k < narc) {
            cnw = cand_cost(a_w[a0 + k], cst, score(a_col[a0 + k]), p.scale);
            created = cnw < local + (double)abeam;
            local = min_f64(local, cnw);
            d = a_rec[a0 + k].x;
            dan = a_rec[a0 + k].y;
          }
          u32 s = kEmpty;
          {
            bool pend = created; u32 h = tab.hash(d);
            while (__any(pend)) { tab.probe(pend, h, s, d, dan); WSYNC(); if (ctr[0] > (u32)N) break; }
          }
          if (s != kEmpty) lower(s, cnw, ((u32)i << kArcBits) | (u32)k);
          if (s != kEmpty) {  // tail candidates always go through the stash
            u32 q = atomicAdd(&ctr[1], 1u);
            if (q < (u32)C) { st_a[q] = s; st_b[q] = ((u32)i << kArcBits) | (u32)k; st_key[q] = dkey(cnw); }
          }
        }
        if (single) {
          WSYNC();  // every candidate of the frame has lowered its slot's cost
          // winners straight from registers: earliest candidate among those that reached the slot's final best cost
  #pragma unroll
          for (int k = 0; k < kArcCache; k++)
            if (sl[k] != kEmpty && dkey(nw[k]) == s_cost[sl[k]]) atomicMin(&s_W[sl[k]], ((u32)i << kArcBits) | (u32)k);
        }
      }
      if constexpr (kEps) frame_min = run;
    }
    prefetch_next_row();
    // the stash lives in HBM: make its stores visible before other lanes read them back (workgroup-scope fence waits for
    // them); frames that kept everything in registers/LDS only need the wavefront hand-over
    if (used_stash) __threadfence_block();
    WSYNC();
    const u32 nslots = ctr[0], nstash = ctr[1];
    if (__any(bad_degree)) { status = ST_UNSUPPORTED; break; }
    if (spec && __any(viol)) { status = ST_TOKEN_OVERFLOW; break; }   // given up as a capacity overflow is (ST_GROW)
    if (nslots > (u32)N || nstash > (u32)C || cand_base > (u32)C) { status = ST_TOKEN_OVERFLOW; break; }
    if (nslots == 0) { n = 0; t++; break; }  // everything pruned: no surviving token

    // ---------------- winners for stashed candidates (multi-chunk frames and deep states)
    for (u32 q0 = 0; q0 < nstash; q0 += 64) {
      u32 q = q0 + lane;
      if (q < nstash) {
        u32 s = st_a[q];
        if (st_key[q] == s_cost[s]) atomicMin(&s_W[s], st_b[q]);
      }
    }
    WSYNC();  // winners settled
    stamps.mark(6);   // general path + stash winners (zero when the fast path ran)
    // ---------------- Kaldi list order of the new tokens: for every slot the ordinal of its hash bucket's first creator and
    // its rank inside the bucket; bucket sizes at the leaders' ordinals, then exclusive sums = where every bucket starts.
    // (kEps: slots created by the epsilon closure carry ordinals past the candidates': s_F = 0x80000000 | k.)
    auto ord_of = [&](u32 F) -> u32 {
      if constexpr (kEps) { if (F >> 31) return cand_base + (F & 0x7FFFFFFFu); }
      return t_cbase[F >> kArcBits] + (F & (kMaxArcsPerState - 1));
    };
    auto order_pass = [&](u32 ns, u32 n_ord) {
      for (u32 j0 = 0; j0 < ns; j0 += 64) {
        u32 j = j0 + lane;
        if (j < ns) {
          const u32 d = s_state[j], Fj = s_F[j];
          u32 Fb = Fj, nb = 1, rank = 0;
          if ((u32)S > H) {
            nb = 0;
            for (u32 m = d % H; m < (u32)S; m += H) {
              u32 sm = find(m);
              if (sm < (u32)N) {
                u32 Fm = s_F[sm];
                nb++;
                if (Fm < Fj) rank++;
                if (Fm < Fb) Fb = Fm;
              }
            }
          }
          const u32 ord_b = ord_of(Fb);
          s_aux[j] = (rank << 24) | ord_b;
          if (Fb == Fj) cntord[ord_b] = nb;
        }
      }
      WSYNC();
      {
        u32 carry = 0;
        for (u32 o0 = 0; o0 < n_ord; o0 += 64) {
          u32 o = o0 + lane;
          u32 v = o < n_ord ? cntord[o] : 0u;
          const u32 inc = incl_scan_sum(v);
          if (o < n_ord && v != 0) cntord[o] = carry + inc - v;  // only leader ordinals are ever non-zero (and reset below)
          carry += (u32)__builtin_amdgcn_readlane((int)inc, 63);
        }
      }
      WSYNC();
    };
    order_pass(nslots, cand_base);
    stamps.mark(7);   // list order (bucket ranks, ordinal scan)
    u32 nslots_f = nslots;      // slots after the epsilon closure (kEps)
    if constexpr (kEps) {
      // ---------------- FasterDecoder::ProcessNonemitting(next_weight_cutoff): process_nonemitting() after the stack fill
      const double eps_cut = frame_min + (double)abeam;
      bool any_eps = false;
      for (u32 j0 = 0; j0 < nslots; j0 += 64) {
        const u32 j = j0 + lane;
        u32 ei = 0;
        if (j < nslots) { ei = p.w_epsinfo[(size_t)utt * p.eps_stride + s_state[j]]; e.info[j] = ei; }
        if (__any((ei & 127u) != 0u)) any_eps = true;
      }
      if (any_eps) {
        bool eps_broken = false;
        for (u32 j0 = 0; j0 < nslots; j0 += 64) {
          const u32 j = j0 + lane;
          if (j < nslots) {
            const u32 aux = s_aux[j];
            const u32 pos = cntord[aux & 0xFFFFFFu] + (aux >> 24);
            if (pos < nslots) e.inv[pos] = j; else eps_broken = true;
          }
        }
        if (__any(eps_broken)) { status = ST_INTERNAL; break; }
        WSYNC();
        u32 sp = 0;
        for (u32 q0 = 0; q0 < nslots; q0 += 64) {
          const u32 q = q0 + lane;
          const u32 j = q < nslots ? e.inv[q] : 0u;
          const bool has = q < nslots && (e.info[j] & 127u) != 0u;
          const u64 m = __ballot(has);
          if (has) e.stk[sp + (u32)__popcll(m & ((1ull << lane) - 1ull))] = j;
          sp += (u32)__popcll(m);
        }
        WSYNC();
        u32 eord;
        const EpsClosure ec = process_nonemitting(p, utt, lane, a_rec, tab, e, eps_cut, sp, cand_base, (u32)C, eord);
        if (ec == kEpsDegree) { status = ST_UNSUPPORTED; break; }
        if (ec == kEpsCapacity) { status = ST_TOKEN_OVERFLOW; break; }
        nslots_f = ctr[0];
        if (nslots_f > nslots) {
          // new states: the list order is worked out again over all slots (a new state goes to the end of its bucket's
          // chain, which may lie in the middle of the list)
          for (u32 j0 = 0; j0 < nslots; j0 += 64) {
            const u32 j = j0 + lane;
            if (j < nslots) cntord[s_aux[j] & 0xFFFFFFu] = 0u;
          }
          WSYNC();
          order_pass(nslots_f, cand_base + eord);
        }
      }
    }
    // ---------------- write the new list + back-pointers, reset the tables
    if (bp_used + nslots_f > bp_cap) { status = ST_BP_OVERFLOW; break; }
    bool broken = false;  // defensive: an inconsistent table must never turn into an out-of-range store
    if constexpr (kEps) {
      for (u32 j0 = 0; j0 < nslots_f; j0 += 64) {
        const u32 j = j0 + lane;
        if (j < nslots_f) { const u32 aux = s_aux[j]; e.pos[j] = cntord[aux & 0xFFFFFFu] + (aux >> 24); }
      }
      WSYNC();
    }
    for (u32 j0 = 0; j0 < nslots_f; j0 += 64) {
      u32 j = j0 + lane;
      if (j < nslots_f) {
        const u32 aux = s_aux[j];
        const u32 pos = cntord[aux & 0xFFFFFFu] + (aux >> 24);
        const u32 d = s_state[j], W = s_W[j];
        bool eps_w = false;
        if constexpr (kEps) eps_w = (W >> 31) != 0u;
        if (eps_w) {
          // the token came over an epsilon arc: its predecessor is a token of THIS frame's list (no frame consumed)
          const u32 src = W & 0x7FFFFFFFu;
          if (pos >= nslots_f || src >= nslots_f || d >= (u32)S) broken = true;
          else {
            n_state[pos] = d;
            n_an[pos] = s_an[j];
            n_cost[pos] = dunkey(s_cost[j]);
            bp[bp_used + pos] = ((u64)e.arc[j] << 32) | (u64)e.pos[src];
          }
        } else {
          const u32 ppos = W >> kArcBits, k = W & (kMaxArcsPerState - 1);
          if (pos >= nslots_f || ppos >= (u32)n || d >= (u32)S) broken = true;
          else {
            const u32 arc = (c_an[ppos] >> 7) + k;
            n_state[pos] = d;
            n_an[pos] = s_an[j];
            n_cost[pos] = dunkey(s_cost[j]);
            bp[bp_used + pos] = ((u64)arc << 32) | (u64)ppos;
          }
        }
      }
    }
    if (__any(broken)) { status = ST_INTERNAL; break; }
    WSYNC();
    for (u32 j0 = 0; j0 < nslots_f; j0 += 64) {
      u32 j = j0 + lane;
      if (j < nslots_f) { hmap[s_bucket[j]] = kEmpty; cntord[s_aux[j] & 0xFFFFFFu] = 0; }
    }
    if (lane == 0) { tokoff[t] = (u32)bp_used; ctr[0] = 0; ctr[1] = 0; }
    bp_used += nslots_f;
    n = (int)nslots_f;
    cur ^= 1;
    if (!kListsInLds) __threadfence_block();  // token lists in HBM: stores must land before the next frame reads them
    WSYNC();
    stamps.mark(8);   // new list, back-pointers, table reset
  }
  stamps.flush(p, utt, lane);
  __threadfence_block();  // back-pointer records (HBM) are read back by the traceback below
  u32 *c_state = l_state0 + cur * N;
  double *c_cost = l_cost0 + cur * N;
  if (p.windowed && status == ST_OK && t < T && n > 0) {
    // ---------------- end of a window, utterance not finished: park the token list and publish the band of depths the
    // next window's frames can reach.  A token on state s at frame t' >= t descends from a live token l of frame t, so
    //   bfs_depth(s) <= bfs_depth(l) + (t' - t)   and   longest_depth(s) >= longest_depth(l):
    // a pdf can be asked for in [t, t + K) only if some arc emitting it leaves a state inside those two bounds.
    const u32 *c_an = l_an0 + cur * N;
    u32 dmax = 0, dmin_inv = 0;   // max of bfs depth; max of ~longest (= min of longest)
    for (int i = lane; i < n; i += 64) {
      const u32 s_ = c_state[i];
      if (kListsInLds) { park_state[i] = s_; park_an[i] = c_an[i]; park_cost[i] = c_cost[i]; }
      if (p.state_depth) {
        const int32_t *sd = p.state_depth + 2 * (so + (int64_t)s_);
        dmax = max(dmax, (u32)sd[0]);
        dmin_inv = max(dmin_inv, ~(u32)sd[1]);
      }
    }
    dmax = wave_max_u32(dmax);
    dmin_inv = wave_max_u32(dmin_inv);
    if (lane == 0) {
      VitState vs;
      vs.n = n; vs.cur = kListsInLds ? 0 : cur; vs.done = 0; vs.pad0 = 0; vs.H = H; vs.pad1 = 0; vs.bp_used = bp_used;
      p.w_vstate[utt] = vs;
      if (p.band) publish_band(p, utt, dmax, dmin_inv);
    }
    return;
  }
  if (p.windowed && lane == 0) {   // finished one way or the other: later windows of this pass skip the utterance
    VitState vs;
    vs.n = 0; vs.cur = 0; vs.done = 1; vs.pad0 = 0; vs.H = H; vs.pad1 = 0; vs.bp_used = bp_used;
    p.w_vstate[utt] = vs;
  }
  if (p.pass == 0 && lane == 0) p.w_hash[utt] = H;

  finalize_utterance(p, utt, lane, status, t, T, n, c_state, c_cost, final_w, bp, tokoff, f0, ab_, a_w, a_col, ll, P, kEps, bp_used,
                     bp_cap);
}

}  // namespace
