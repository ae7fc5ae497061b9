"""Directed cases for viterbi_small_kernel, the 64-token first tier of the lazy path (csrc/viterbi_small.hpp), shared by
tests/test_small_tier_cpu.py (the oracle alone: every case is what it claims to be, and can tell right from wrong) and
tests/test_gpu_small_tier.py (the device against the oracle, bit for bit).

Exact scores.  The model (``model()``) holds single Gaussians with unit variances, integer means that are permutations and
sign flips of one vector, and one gconst rounded to 1/256; the frames are integer vectors.  Every log-likelihood is then a
multiple of 1/256 that no order of summation can change.  Graph weights are multiples of 0.25.  A directed graph uses ONE
pdf on all its arcs: the acoustic cost of a frame is the same for every token, so which tokens are inside the beam, which
tie and which win is decided by the graph weights alone, at every acoustic scale — path costs are sums of floats, exact in
double.  Arcs that compete carry different transition-ids (``R`` ids per pdf), so ``ali`` names the winner.

A case is a dict: name, fst, T, feats, claims(trace, ref) — the host-side facts, as assertions on the oracle's trace
(oracle.align_feats_trace) — and ``wrong``: the decoder rules (oracle.VARIANTS) under which the oracle's alignment of the
case must change.  A batch is a dict: name, cases, beam, retry, caps, scales, eps.
"""
from __future__ import annotations

import types
import zlib

import numpy as np

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import model as M
from oracle import oracle as O

DIM, P, R = 39, 8, 128
MIN_STATES = 72           # every graph is padded past 64 states: the plan then starts with the 64-token tier
N_IN, N_UNDER, N_CAND, N_CREATED, N_CLOSED, MIN_ACTIVE, N_AT_CUT, MAX_NARC = range(8)
CAPS = dict(max_tokens=128, bp_tokens_per_frame=512)
H0 = 1000                 # FasterDecoder's initial hash size: below 500 tokens it never grows


def tm():
    n = R * P
    return types.SimpleNamespace(num_transition_ids=n, num_pdfs=P, id2pdf=np.concatenate([[-1], np.arange(n) % P]).astype(np.int32))


_MODEL = None


def model():
    """P single-Gaussian pdfs, unit variances, means ± permutations of (2, -1, 1, 0, …): one gconst, a multiple of 1/256."""
    global _MODEL
    if _MODEL is None:
        rng = np.random.default_rng(5)
        base = np.zeros(DIM, np.float32)
        base[:3] = (2.0, -1.0, 1.0)
        means = np.stack([rng.permutation(base) * rng.choice([-1.0, 1.0], size=DIM) for _ in range(P)]).astype(np.float32)
        g = -0.5 * (DIM * np.log(2 * np.pi) + float((base * base).sum()))
        gconsts = np.full(P, np.round(g * 256.0) / 256.0, np.float32)
        _MODEL = M.DiagGmmModel(DIM, gconsts, means, np.ones((P, DIM), np.float32), np.arange(P + 1, dtype=np.int32))
    return _MODEL


def feats(name, T):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return rng.integers(-2, 3, size=(T, DIM)).astype(np.float32)


class Builder:
    """A graph by hand.  ``new()`` hands out auxiliary states from ``aux`` upwards; a case that needs particular state numbers
    simply uses them.  Every emitting arc gets its own label r: transition-id 1 + pdf + P·(r mod R)."""

    def __init__(self, pdf=0, aux=0):
        self.pdf, self.next, self.out, self.final, self.r = pdf, aux, {}, {}, 0

    def new(self):
        s = self.next
        self.next += 1
        self.out.setdefault(s, [])
        return s

    def arc(self, s, d, w=0.0, eps=False, pdf=None):
        assert float(w) * 4 == int(float(w) * 4)
        if eps:
            il = 0
        else:
            il = 1 + (self.pdf if pdf is None else pdf) + P * (self.r % R)
            self.r += 1
        self.out.setdefault(s, []).append((il, 0 if (eps or s == d) else il, float(w), d))
        self.out.setdefault(d, [])
        return il

    def chain(self, s, n):
        for _ in range(n):
            d = self.new()
            self.arc(s, d)
            s = d
        return s

    def fst(self, start, S=None):
        S = max(max(self.out) + 1, MIN_STATES, S or 0)
        offs, arcs = [0], []
        for s in range(S):
            arcs += self.out.get(s, [])
            offs.append(len(arcs))
        a = np.zeros(len(arcs), dtype=K.ARC_DTYPE)
        for i, t in enumerate(arcs):
            a[i] = t
        final = np.full(S, np.inf, np.float32)
        for s, w in self.final.items():
            final[s] = w
        return K.Fst(start, np.asarray(offs, np.int64), a, final)


def _case(name, b, start, T, claims, wrong=(), S=None, inside=True, **extra):
    """``inside``: the first beam's pass stays within the small kernel's envelope (``envelope``); False: it hands over."""
    return dict(name=name, inside=inside, fst=b.fst(start, S), T=T, feats=feats(name, T), claims=claims, wrong=tuple(wrong), **extra)


def hash_list_order(inserted, H=H0):
    """Kaldi's HashList order of states inserted in this order: buckets (state mod H) by first occupancy, insertion order
    inside a bucket."""
    buckets = {}
    for s in inserted:
        buckets.setdefault(s % H, []).append(s)
    return [s for members in buckets.values() for s in members]


def hash256(d):
    return ((d * 2654435761) & 0xFFFFFFFF) >> 24


# ---- 1 tokens -------------------------------------------------------------------------------------------------------------
def fan(name, k, delay, T, eps=False):
    """A chain of ``delay`` arcs, a hub with k arcs to k leaves (through one state's epsilon arcs when ``eps``), every leaf
    with a self-loop and an arc to the final state F, which has no arcs: k tokens are created at frame ``delay``, k + 1 at every
    later frame, all leaves on one cost.  F's winner is the first leaf in list order."""
    b = Builder(pdf=zlib.crc32(name.encode()) % P)
    s0 = b.new()
    h = b.chain(s0, delay)
    F = b.new()
    b.final[F] = 0.0
    if eps:
        x = b.new()
        b.arc(h, x)
        h = x
    leaves = [b.new() for _ in range(k)]
    for L in leaves:
        b.arc(h, L, eps=eps)
    for L in leaves:
        b.arc(L, L)
        b.arc(L, F)
    first = k + (1 if eps else 0)      # tokens after frame `delay` (with the closure's: the k leaves and their source)
    col = N_CLOSED

    def claims(tr, ref):
        assert tr[:delay, col].max(initial=1) == 1
        assert tr[delay, col] == first and tr[delay, N_CREATED] == (1 if eps else k)
        later = tr[delay + 1:, col]
        assert len(later) >= 1 and (later == k + 1).all(), later
        assert tr[:, N_CREATED].max() <= max(k + 1, 1)
    return _case(name, b, s0, T, claims, wrong=("last_arc_wins",), inside=k + 1 <= 64, peak=max(first, k + 1))


def tokens_batch():
    cases = [fan("t63", 62, 3, 70), fan("t64_hold_and_last", 63, 3, 100), fan("t64_at_last_frame", 63, 66, 68),
             fan("t65_frame1", 64, 0, 6), fan("t65_second_window", 64, 70, 80), fan("t65_last_frame", 64, 30, 32)]
    return dict(name="tokens", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0, 0.1))


# ---- 2 candidates ----------------------------------------------------------------------------------------------------------
CAND_BEAM = 1.0


def cand(name, a, hot, delay=2, T=None, seed_probe=False):
    """Hub → m = len(a) tokens P_i (24 or more: the beam is in force); P_i has a[i] arcs into a pool of max(a) states, the
    pool goes to F.  Frame delay + 1 has sum(a) candidates in runs of a[i]; the candidate with ordinal ``hot`` is 0.25 cheaper
    than all others, so the alignment passes through it: its owner, its arc index and its slot must be right.

    ``seed_probe``: P_1 (whose run straddles ordinals 63|64) is the best token by 0.5 and its arc at ordinal 65 another 1.0
    cheaper: the running cutoff is −1.5 + beam from the start — only for a decoder whose seed loop sees the best token's
    candidates of the second round.  P_0's first arc (ordinal 0) goes to X at −0.25: not below that cutoff, pruned.  Seeded
    from less, X is created, survives the next frame's min_active cutoff and wins by 5."""
    T = T or delay + 5
    assert len(a) >= 24 and T >= delay + 4
    b = Builder(pdf=zlib.crc32(name.encode()) % P)
    s0 = b.new()
    h = b.chain(s0, delay)
    F = b.new()
    b.final[F] = 0.0
    b.arc(F, F)
    toks = [b.new() for _ in a]
    pool = [b.new() for _ in range(max(a))]
    for i, t in enumerate(toks):
        b.arc(h, t, -0.5 if (seed_probe and i == 1) else 0.0)
    X = b.new() if seed_probe else None
    o, hot_tid = 0, None
    for i, t in enumerate(toks):
        for j in range(a[i]):
            w = (-1.0 if seed_probe else -0.25) if o == hot else 0.0
            d = pool[j]
            if seed_probe and o == 0:
                w, d = -0.25, X
            tid_ = b.arc(t, d, w)
            if o == hot:
                hot_tid = tid_
            o += 1
    for q in pool:
        b.arc(q, F)
    if seed_probe:
        b.arc(X, F, -5.0)
    total, f = sum(a), delay + 1

    def claims(tr, ref):
        assert tr[f, N_IN] == len(a) > 20 and tr[f, N_UNDER] == len(a) and tr[f, N_CAND] == total, tr[f]
        assert tr[f, MAX_NARC] == max(a) and tr[:, N_CAND].max() == total and tr[:, N_CREATED].max() <= 64
        if total <= 192:
            assert ref["status"] == 0 and ref["ali"][f] == hot_tid     # the hot candidate is on the path
    return _case(name, b, s0, T, claims, wrong=("no_seed",) if seed_probe else (), inside=total <= 192, total=total, narc=max(a))


def _pad(a, m=24):
    return list(a) + [0] * (m - len(a))


def candidates_batch():
    runs = {64: [60, 4], 65: [60, 5], 128: [60, 8, 58, 2], 129: [60, 8, 58, 3], 192: [60, 8, 58, 6, 60], 193: [60, 8, 58, 6, 61]}
    hots = {64: (63,), 65: (63, 64), 128: (64, 127), 129: (127, 128), 192: (128, 191), 193: (192,)}
    cases = [cand(f"c{total}_hot{hot}", _pad(a), hot) for total, a in runs.items() for hot in hots[total]]
    cases.append(cand("c64arcs_hot63", _pad([64, 30, 1]), 63))           # k = 63 of a 64-arc state
    cases.append(cand("c64arcs_second_run", _pad([3, 64, 64]), 3 + 64 + 63))   # a 64-arc run across 63|64, another across 127|128
    cases.append(cand("c_seed_round1", _pad([60, 8, 58, 6]), 65, seed_probe=True))
    return dict(name="candidates", cases=cases, beam=CAND_BEAM, retry=40.0, caps=CAPS, scales=(1.0, 0.5, 0.1))


# ---- 3 min_active -----------------------------------------------------------------------------------------------------------
MA_BEAM = 2.0


def minact(name, costs, juicy_cost, n_under, at_cut, min_active, delay=2, eps=False):
    """Hub → one token per entry of ``costs`` (shuffled over the lanes), each with one arc to G; the tokens whose cost is
    ``juicy_cost`` — the chosen cutoff: they must NOT expand — have that arc 100 cheaper, so a decoder that expands them
    aligns through one of them.  ``eps``: G has an epsilon arc to a second final state (the kEps kernel, which finds the
    best cost by reduction instead of carrying it)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    costs = [float(c) for c in rng.permutation(costs)]
    assert len(costs) > 20 and min(costs) == 0.0 and costs.count(0.0) == 1
    b = Builder(pdf=zlib.crc32(name.encode()) % P)
    s0 = b.new()
    h = b.chain(s0, delay)
    G = b.new()
    b.final[G] = 0.0
    b.arc(G, G)
    if eps:
        G2 = b.new()
        b.arc(G, G2, 0.25, eps=True)
        b.final[G2] = 0.0
        b.arc(G2, G2)
    toks = [b.new() for _ in costs]
    for t, c in zip(toks, costs):
        b.arc(h, t, c)
    best_tid = None
    for t, c in zip(toks, costs):
        tid_ = b.arc(t, G, -100.0 if c == juicy_cost else 0.0)
        if c == 0.0:
            best_tid = tid_
    f = delay + 1
    srt = sorted(costs)
    inside = sum(c <= MA_BEAM for c in costs)

    def claims(tr, ref):
        assert tr[f, N_IN] == len(costs) and tr[f, MIN_ACTIVE] == int(min_active) == int(inside <= 20), tr[f]
        assert tr[f, N_UNDER] == n_under and tr[f, N_AT_CUT] == at_cut == costs.count(juicy_cost), tr[f]
        assert juicy_cost == (srt[20] if min_active else MA_BEAM)
        assert ref["status"] == 0 and ref["ali"][f] == best_tid
    return _case(name, b, s0, delay + 5, claims, wrong=("select_lt", "expand_le") if min_active else ("expand_le",),
                 in_beam=inside)


def _ma_costs(inside, outside):
    """``inside`` tokens within the beam (one at 0, the others on 0.25 … 2.0 with ties), then the ``outside`` costs."""
    return [0.0] + [0.25 * (i % 7 + 1) for i in range(inside - 1)] + list(outside)


def minact_cases(eps=False):
    up = [3.0 + 0.25 * i for i in range(40)]
    e = "_eps" if eps else ""
    out = []
    for inside in (1, 19, 20):
        costs = _ma_costs(inside, up[: 30 - inside])
        out.append(minact(f"ma_in{inside}{e}", costs, sorted(costs)[20], 20, 1, True, eps=eps))
    # 21 inside, the 21st exactly at best + beam: the beam rule, and the token at the cutoff stays
    costs = _ma_costs(20, [MA_BEAM] + up[:9])
    out.append(minact(f"ma_in21_at_beam{e}", costs, MA_BEAM, 20, 1, False, eps=eps))
    # the 21st smallest tied among 2 (ranks 20, 21 and ranks 21, 22 of 30) and among 5 (ranks 19 … 23)
    costs = _ma_costs(5, up[:14] + [8.0, 8.0] + [9.0 + 0.25 * i for i in range(9)])
    out.append(minact(f"ma_tie2_low{e}", costs, 8.0, 19, 2, True, eps=eps))
    costs = _ma_costs(5, up[:15] + [8.0, 8.0] + [9.0 + 0.25 * i for i in range(8)])
    out.append(minact(f"ma_tie2_high{e}", costs, 8.0, 20, 2, True, eps=eps))
    costs = _ma_costs(5, up[:13] + [8.0] * 5 + [9.0 + 0.25 * i for i in range(7)])
    out.append(minact(f"ma_tie5{e}", costs, 8.0, 18, 5, True, eps=eps))
    # 64 tokens, 3 inside: the selection runs over 61 lanes
    costs = _ma_costs(3, up[:17] + [8.0] * 3 + [9.0 + 0.25 * i for i in range(41)])
    out.append(minact(f"ma_64_tokens{e}", costs, 8.0, 20, 3, True, eps=eps))
    return out


def minact_batch():
    return dict(name="min_active", cases=minact_cases(), beam=MA_BEAM, retry=40.0, caps=CAPS, scales=(1.0, 0.5, 0.1))


# ---- 4 list order, 5 slot table -----------------------------------------------------------------------------------------------
def order(name, S, created, k, delay=1, eps_from=None, hot=None, aux=400):
    """Hub → the states ``created``, in that order, all on one cost (``eps_from``: {state: [states its epsilon arcs create]},
    inserted by the closure after the emitting arcs' states).  Kaldi's list order L of those states follows from the hash
    (``hash_list_order``); the states L[k:] each have an arc to G, the others to a dead end.  G's winner is the first in
    list order among equal costs: the alignment names L[k].  ``hot``: that state's arc to G is 0.25 cheaper instead, and
    the alignment names it."""
    eps_from = eps_from or {}
    inserted = list(created) + [c for s in created for c in eps_from.get(s, [])]
    L = hash_list_order(inserted)
    b = Builder(pdf=zlib.crc32(name.encode()) % P, aux=aux)
    s0 = b.new()
    h = b.chain(s0, delay)
    G, dead = b.new(), b.new()
    b.final[G] = 0.0
    b.arc(G, G)
    assert b.next <= 1000 and not ({x % H0 for x in inserted} & {x % H0 for x in range(aux, b.next)})
    for x in created:
        b.arc(h, x)
        for c in eps_from.get(x, []):
            b.arc(x, c, eps=True)
    tids = {}
    for x in inserted:
        if hot is None:
            tids[x] = b.arc(x, G if x in L[k:] else dead)
        else:
            tids[x] = b.arc(x, G, -0.25 if x == hot else 0.0)
    want = L[k] if hot is None else hot
    f = delay + 1
    wrong = []
    if hot is None:
        for rule, Lw in (("order_by_state", sorted(inserted)), ("order_ignores_buckets", inserted)):
            if [x for x in Lw if x in L[k:]][0] != want:
                wrong.append(rule)

    def claims(tr, ref):
        assert tr[f, N_IN] == len(inserted) and tr[f - 1, N_CLOSED] == len(inserted), tr[f]
        assert ref["status"] == 0 and ref["ali"][f] == tids[want], (ref["ali"][f], tids, L)
    return _case(name, b, s0, delay + 4, claims, wrong=wrong, S=S, L=L, inserted=inserted)


ORDER_CONFIGS = [
    # (graph states, states in order of creation, delay)
    (1000, [5, 999, 7], 1), (1001, [0, 7, 1000], 1), (1001, [1000, 7, 0], 66), (1064, [63, 7, 1063], 1), (1064, [1063, 70, 63], 1),
    (1064, [10, 20, 1010, 1020], 1), (1064, [1020, 10, 20, 1010], 3),
    (2100, [50, 7, 2050, 1050], 1), (2100, [2050, 7, 50, 1050], 1), (2100, [1050, 60, 50, 2050, 1060], 66),
]


def order_batch():
    cases = []
    for S, created, delay in ORDER_CONFIGS:
        found = set()
        for k in range(len(created) - 1):
            c = order(f"o{S}_{'_'.join(map(str, created))}_k{k}", S, created, k, delay)
            if c["wrong"]:
                cases.append(c)
                found |= set(c["wrong"])
        assert "order_by_state" in found and (S == 1000 or "order_ignores_buckets" in found), (S, created, found)
    return dict(name="list_order", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0,))


def _probe_lengths(states):
    """Longest linear-probe walk when ``states`` are filed into the 256-entry table one after another."""
    tab, worst = {}, 0
    for s in states:
        hk, n = hash256(s), 0
        while hk in tab:
            hk, n = (hk + 1) & 255, n + 1
        tab[hk] = s
        worst = max(worst, n)
    return worst, tab


def slots_batch():
    S = 4096
    by = {}
    for d in range(64, S):
        if not 400 <= d % H0 < 500:          # (the auxiliary states' hash-list buckets)
            by.setdefault(hash256(d), []).append(d)
    bstar = max(by, key=lambda k: (len(by[k]), -k))
    longest = by[bstar]
    wrap = by[255] + by[254][:6]
    m_abs = [m for m in by[bstar] if m >= 1000 and (m % H0) not in {x % H0 for x in by[bstar] if x != m}][0]
    absent = [m_abs % H0] + [x for x in by[bstar] if x != m_abs]
    cases = []
    for nm, states in (("longest_chain", longest), ("wrap_255_to_0", wrap), ("absent_behind_chain", absent)):
        assert len(states) <= 64 and len(set(states)) == len(states)
        worst, tab = _probe_lengths(states)
        c = order(f"slots_{nm}", S, states, 0, hot=states[-1])
        c.update(chain=worst, table=tab)
        cases.append(c)
        c2 = order(f"slots_{nm}_tied", S, states, len(states) // 2)
        c2.update(chain=worst, table=tab)
        cases.append(c2)
    cases[0]["want_chain"] = len(longest) - 1
    meta = dict(longest=longest, wrap=wrap, absent=absent, m_abs=m_abs, bstar=bstar)
    return dict(name="slot_table", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0,), meta=meta)


# ---- 6 back-pointers ----------------------------------------------------------------------------------------------------------
BP_T, BP_BPF = 8, 4


def bp_case(name, extra, at_last):
    """A chain of T arcs to the final state plus ``extra`` dead ends created at the first (or the last) frame:
    T + extra back-pointer records."""
    b = Builder(pdf=zlib.crc32(name.encode()) % P)
    s0 = b.new()
    pre = b.chain(s0, BP_T - 1) if at_last else s0
    F = b.new() if at_last else None
    src = pre
    if at_last:
        b.arc(src, F)
    else:
        nxt = b.new()
        b.arc(src, nxt)
    for _ in range(extra):
        b.arc(src, b.new())
    if not at_last:
        F = b.chain(nxt, BP_T - 1)
    b.final[F] = 0.0
    records = BP_T + extra

    def claims(tr, ref):
        assert int(tr[:, N_CLOSED].sum()) == records and ref["status"] == 0
    return _case(name, b, s0, BP_T, claims, inside=records <= BP_T * BP_BPF, records=records)


def bp_batch():
    fit, over = BP_T * (BP_BPF - 1), BP_T * (BP_BPF - 1) + 1
    cases = [bp_case("bp_exact_first_frame", fit, False), bp_case("bp_exact_last_frame", fit, True),
             bp_case("bp_one_short_first_frame", over, False), bp_case("bp_one_short_last_frame", over, True)]
    return dict(name="back_pointers", cases=cases, beam=10.0, retry=40.0, caps=dict(max_tokens=128, bp_tokens_per_frame=BP_BPF),
                scales=(1.0,))


# ---- 7 dying out ----------------------------------------------------------------------------------------------------------------
def die(name, f, T, w_path, decoys=24):
    """At frame f the first pass holds ``decoys`` dead ends on cost 0 and the only real path ``w_path`` above them: beyond
    the beam, not expanded, nothing is created — the first pass dies at frame f.  The retry beam (40) reaches a path 20
    above (status 1), not one 50 above (status 2)."""
    b = Builder(pdf=zlib.crc32(name.encode()) % P)
    s0 = b.new()
    h = b.chain(s0, f - 1)
    for _ in range(decoys):
        b.arc(h, b.new())
    r = b.new()
    b.arc(h, r, w_path)
    F = b.new()
    b.final[F] = 0.0
    b.arc(r, r)
    b.arc(r, F)
    status = 1 if w_path < 40.0 else 2

    def claims(tr, ref):
        assert tr[f - 1, N_CREATED] == decoys + 1 > 21 and tr[f, N_IN] == decoys + 1 and tr[f, N_UNDER] == decoys
        assert tr[f, N_CAND] == 0 and tr[f, N_CREATED] == 0 and tr[:f, N_CREATED].min() >= 1
        assert ref["status"] == status
    return _case(name, b, s0, T, claims, dies_at=f)


def die_batch():
    cases = []
    for nm, f, T in (("mid_window", 30, 40), ("window_start", 64, 70), ("last_frame", 49, 50), ("second_frame", 1, 3)):
        cases += [die(f"die_{nm}_retry_aligns", f, T, 20.0), die(f"die_{nm}_retry_fails", f, T, 50.0)]
    return dict(name="dying_out", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0,))


# ---- 8 lengths and mixed batches ------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 192)


def ladder(name, T):
    """Left-to-right states with self-loops, forward and skip arcs over all pdfs, dyadic weights: a speech-shaped graph."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = min(T, 12)
    b = Builder()
    st = [b.new() for _ in range(n + 1)]
    for i in range(n):
        if T > n:
            b.arc(st[i], st[i], 0.25 * int(rng.integers(0, 8)), pdf=int(rng.integers(0, P)))
        b.arc(st[i], st[i + 1], 0.25 * int(rng.integers(0, 8)), pdf=int(rng.integers(0, P)))
        if i + 2 <= n and T > n:
            b.arc(st[i], st[i + 2], 0.25 * int(rng.integers(0, 12)), pdf=int(rng.integers(0, P)))
    b.final[st[n]] = 0.0
    if T > n:
        b.arc(st[n], st[n], 0.25, pdf=int(rng.integers(0, P)))

    def claims(tr, ref):
        assert ref["status"] == 0 and tr[:, N_CLOSED].max() <= 64 and tr[:, N_CAND].max() <= 192
    return _case(name, b, st[0], T, claims)


def mixed_batch():
    cases = [ladder(f"len{T}", T) for T in LENGTHS]
    cases += [fan("mix_t65_second_window", 64, 70, 80), fan("mix_t65_frame1", 64, 0, 6), fan("mix_t64", 63, 40, 130),
              die("mix_die_mid_aligns", 30, 90, 20.0), die("mix_die_window_start_fails", 64, 70, 50.0),
              die("mix_die_last_aligns", 127, 128, 20.0), fan("mix_chain_lags", 10, 100, 140),
              cand("mix_c193", _pad([60, 8, 58, 6, 61]), 192, delay=66), cand("mix_c192", _pad([60, 8, 58, 6, 60]), 128, delay=70, T=80)]
    return dict(name="mixed", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0, 0.1))


# ---- random graphs on exact scores ---------------------------------------------------------------------------------------------
RANDOM_SEEDS = (0, 1, 2, 3, 6, 7, 8, 9, 11)


def random_case(seed):
    """tests/test_gpu_parity.py's ``_random_graph`` (cycles, dead ends, 64-arc states, weights on the 0.25 grid) over all
    pdfs of the exact model: costs tie between paths through different pdfs, and a narrow beam keeps the min_active rule
    busy — most frames hold more than 20 tokens, and in many the chosen cutoff is shared by several."""
    from tests.test_gpu_parity import _random_graph
    rng = np.random.default_rng(9000 + seed)
    S, T = int(rng.choice([72, 90, 120, 150])), int(rng.choice([20, 64, 65, 100, 130]))
    f = _random_graph(rng, tm(), S)
    name = f"r{seed}"

    def claims(tr, ref):
        busy = (tr[:, N_IN] > 20) & (tr[:, MIN_ACTIVE] == 1)
        assert ref["status"] in (0, 1) and busy.sum() >= 10 and (tr[busy, N_AT_CUT] > 1).sum() >= 3, (busy.sum(),)
    return dict(name=name, fst=f, T=T, feats=feats(name, T), claims=claims, wrong=(), inside=None)      # (which side of the envelope depends on the scale)


def random_batch():
    return dict(name="random_ties", cases=[random_case(s) for s in RANDOM_SEEDS], beam=3.0, retry=40.0, caps=CAPS, scales=(1.0, 0.5))


# ---- 10 epsilon graphs -----------------------------------------------------------------------------------------------------------
def eps_batch():
    cases = [fan("eps_t64_by_closure", 63, 3, 70, eps=True), fan("eps_t65_by_closure", 64, 3, 12, eps=True),
             fan("eps_t65_second_window", 64, 70, 80, eps=True)]
    for S, created, eps_from in ((1064, [63, 300, 7], {300: [1063]}), (2100, [2050, 300, 7, 50], {300: [1050]})):
        found = set()
        for k in range(len(created)):
            c = order(f"eps_o{S}_{'_'.join(map(str, created))}_k{k}", S, created, k, eps_from=eps_from)
            if c["wrong"]:
                cases.append(c)
                found |= set(c["wrong"])
        assert found == {"order_by_state", "order_ignores_buckets"}, found
    return dict(name="epsilon", cases=cases, beam=10.0, retry=40.0, caps=CAPS, scales=(1.0,), eps=True)


def eps_minact_batch():
    return dict(name="epsilon_min_active", cases=minact_cases(eps=True), beam=MA_BEAM, retry=40.0, caps=CAPS, scales=(1.0,),
                eps=True)


_BUILDERS = dict(tokens=tokens_batch, candidates=candidates_batch, min_active=minact_batch, list_order=order_batch,
                 slot_table=slots_batch, back_pointers=bp_batch, dying_out=die_batch, mixed=mixed_batch, random_ties=random_batch, epsilon=eps_batch,
                 epsilon_min_active=eps_minact_batch)
NAMES = tuple(_BUILDERS)
LAG_FAMILIES = ("tokens", "candidates", "min_active", "list_order", "mixed", "random_ties")     # run under every look-ahead setting
_BATCHES: dict = {}
_REFS: dict = {}


def batch(name):
    if name not in _BATCHES:
        _BATCHES[name] = _BUILDERS[name]()
    return _BATCHES[name]


def ref(bname, i, scale=1.0, variant="exact"):
    """The oracle's result for case ``i`` of a batch, with its trace; computed once per process, read-only."""
    key = (bname, i, float(scale), variant)
    if key not in _REFS:
        bt = batch(bname)
        c, am = bt["cases"][i], model()
        f = c["fst"]
        _REFS[key] = O.align_feats_trace(f.num_states, f.start, f.arc_offsets, f.arcs, f.final, c["feats"], am.gconsts,
                                         am.means_invvars, am.inv_vars, am.pdf_offsets, tm().id2pdf, scale, bt["beam"],
                                         bt["retry"], variant=variant)
    return _REFS[key]


def assert_claims(bname, scale=1.0):
    """Every case of the batch lies where it claims to, by the oracle's trace at this scale.  Both test files call this:
    the device test before it launches, so that none of its comparisons passes vacuously."""
    bt = batch(bname)
    for i, c in enumerate(bt["cases"]):
        r = ref(bname, i, scale)
        assert r["trace"].shape == (c["T"], 8)
        try:
            c["claims"](r["trace"], r)
        except AssertionError as e:
            raise AssertionError(f"{bname}/{c['name']} at scale {scale}: {e}") from e
    for c, e in zip(bt["cases"], envelope(bname, scale)):
        assert c["inside"] is None or e["inside"] == c["inside"], (bname, c["name"], e)
    if bname == "random_ties":
        env = envelope(bname, scale)
        assert sum(e["inside"] for e in env) >= 6 and sum(e["peak"] > 40 for e in env) >= 4, env


def envelope(bname, scale=1.0):
    """Per case: does the first beam's pass stay inside the small kernel's envelope (64 tokens, 192 candidates, 64 arcs a
    state, the back-pointer records), and does it die.  From the trace alone."""
    bt = batch(bname)
    out = []
    for i, c in enumerate(bt["cases"]):
        tr = ref(bname, i, scale)["trace"]
        dead = np.flatnonzero(tr[:, N_CLOSED] == 0)
        end = int(dead[0]) + 1 if dead.size else c["T"]
        t = tr[:end]
        inside = bool(t[:, N_CLOSED].max() <= 64 and t[:, N_CREATED].max() <= 64 and t[:, N_CAND].max() <= 192
                      and t[:, MAX_NARC].max() <= 64
                      and int(t[:, N_CLOSED].sum()) <= c["T"] * bt["caps"]["bp_tokens_per_frame"])
        out.append(dict(inside=inside, dies=bool(dead.size), peak=int(t[:, N_CLOSED].max()), cand=int(t[:, N_CAND].max())))
    return out
