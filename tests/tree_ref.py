"""Restatements the tree tests hold the product to, with no code shared with it: a dict-of-events accumulator (a Python
loop over frames, segmentation by ``is_final`` and the self-loops after it), the brute-force best split (every leaf × key × question) and the exhaustive
window enumeration of the transition tuples — and the small cases the CPU and the GPU tests both run.  Alignments are in the
order of the project's graphs: a state's self-loops follow its forward arc."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd.model import TransitionModel

U64 = 2.0 ** -53
N_PHONES = 9
ONE_STATE = (3, 6, 9)          # phones of the one-state entry: a phone may last a single frame
CI = (1, 2)                    # the context-independent phones of the cases


def topology(n_phones: int = N_PHONES, one_state: Sequence[int] = ONE_STATE) -> K.HmmTopology:
    bakis = [K.HmmState(i, i, [(i, 0.75), (i + 1, 0.25)]) for i in range(3)] + [K.HmmState(-1, -1, [])]
    single = [K.HmmState(0, 0, [(0, 0.5), (1, 0.5)]), K.HmmState(-1, -1, [])]
    phones = np.arange(1, n_phones + 1, dtype=np.int32)
    phone2idx = np.full(n_phones + 1, -1, dtype=np.int32)
    for p in phones:
        phone2idx[p] = 1 if int(p) in one_state else 0
    return K.HmmTopology(phones, phone2idx, [bakis, single])


def mono_tm(n_phones: int = N_PHONES, one_state: Sequence[int] = ONE_STATE) -> TransitionModel:
    raw_tm, _am, _tree = mle.init_mono(topology(n_phones, one_state), 2)
    return TransitionModel(raw_tm)


def phone_path(tm: TransitionModel, phone: int, durations: Sequence[int]) -> List[int]:
    """The transition-ids of one pass through a phone's left-to-right entry, ``durations[k]`` frames in emitting state k, in
    the order of the project's graphs (Kaldi's reorder option): a state's forward arc first, then its self-loops."""
    entry = tm.topo.entry_for_phone(phone)
    state_of = {(int(r[0]), int(r[1])): ts + 1 for ts, r in enumerate(tm.tuples)}
    out = []
    for hs, d in enumerate(durations):
        ts = state_of[(phone, hs)]
        dsts = [dst for dst, _p in entry[hs].transitions]
        out += [tm.transition_id(ts, dsts.index(hs + 1))] + [tm.transition_id(ts, dsts.index(hs))] * (d - 1)
    return out


def n_states(tm: TransitionModel, phone: int) -> int:
    return sum(1 for st in tm.topo.entry_for_phone(phone) if st.transitions)


def utterance(rng, tm: TransitionModel, length: int, phones=None) -> np.ndarray:
    """Transition-ids of exactly ``length`` frames: random phones (``phones`` first) with random state durations; a phone that
    no longer fits gives way to a one-state phone, so the utterance ends with a whole phone."""
    ids = [int(p) for p in tm.topo.phones]
    single = [p for p in ids if n_states(tm, p) == 1]
    out: List[int] = []
    k = 0
    while len(out) < length:
        left = length - len(out)
        p = int(phones[k]) if phones is not None and k < len(phones) else int(rng.choice(ids))
        k += 1
        ns = n_states(tm, p)
        if ns > left:
            p, ns = int(rng.choice(single)), 1
        d = [1] * ns
        for _ in range(min(left - ns, int(rng.integers(0, 6)))):
            d[int(rng.integers(0, ns))] += 1
        out += phone_path(tm, p, d)                # whatever remains is at least one frame: a one-state phone fits
    return np.asarray(out, dtype=np.int32)


@dataclass
class Case:
    tm: TransitionModel
    feats: np.ndarray
    frame_off: np.ndarray
    ali: np.ndarray
    ci: tuple


def make_case(rng, lengths: Sequence[int], dim: int, integer: bool = True, tm: TransitionModel = None, ci=CI, phones=None) -> Case:
    tm = tm or mono_tm()
    fo = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
    ali = np.concatenate([utterance(rng, tm, int(n), phones) for n in lengths] + [np.zeros(0, np.int32)]).astype(np.int32)
    T = int(fo[-1])
    if integer:
        x = rng.integers(-8, 9, size=(T, dim)).astype(np.float32)
    else:
        x = (rng.normal(size=(T, dim)) * np.linspace(12.0, 1.5, dim) + rng.normal(0, 5.0, size=dim)).astype(np.float32)
    return Case(tm, x, fo, ali, tuple(ci))


LENGTHS = (0, 1, 2, 63, 64, 65, 129)


# ---- the accumulator -----------------------------------------------------------------------------------------------------------
def pdf_class_of(tm: TransitionModel, tid: int) -> int:
    ts = int(tm.id2state[tid])
    phone, hs = int(tm.tuples[ts - 1, 0]), int(tm.tuples[ts - 1, 1])
    st = tm.topo.entry_for_phone(phone)[hs]
    return st.self_loop_pdf_class if tm.is_self_loop[tid] else st.forward_pdf_class


def accumulate(case: Case, want_abs: bool = False):
    """Dict of events: (l, c, r, pdf-class) → frames.  Returns (keys uint64 [E] ascending, count, sum, sumsq, frame_event,
    skipped[, Σ|x|, Σx²]) with the sums formed by numpy over each event's rows."""
    tm, x, fo, ali = case.tm, case.feats.astype(np.float64), case.frame_off, case.ali
    n_tids = tm.num_transition_ids + 1
    events: Dict[tuple, List[int]] = {}
    skipped = 0
    for u in range(len(fo) - 1):
        f0, f1 = int(fo[u]), int(fo[u + 1])
        if f0 == f1:
            continue
        segs, cur, ok = [], [], all(0 < int(ali[t]) < n_tids for t in range(f0, f1))
        t = f0
        while ok and t < f1:                       # SplitToPhones, reordered: a final id takes the self-loops after it along
            cur.append(t)
            if tm.is_final[int(ali[t])]:
                while t + 1 < f1 and tm.is_self_loop[int(ali[t + 1])]:
                    t += 1
                    cur.append(t)
                segs.append(cur)
                cur = []
            t += 1
        ok = ok and not cur and all(len({int(tm.id2phone[ali[t]]) for t in seg}) == 1 for seg in segs)
        if not ok:
            skipped += 1
            continue
        ph = [int(tm.id2phone[ali[seg[0]]]) for seg in segs]
        for i, seg in enumerate(segs):
            l, r = (ph[i - 1] if i else 0), (ph[i + 1] if i + 1 < len(ph) else 0)
            if ph[i] in case.ci:
                l = r = 0
            for t in seg:
                events.setdefault((l, ph[i], r, pdf_class_of(tm, int(ali[t]))), []).append(t)
    order = sorted(events)
    keys = np.array([(l << 48) | (c << 28) | (r << 8) | pc for l, c, r, pc in order], dtype=np.uint64)
    dim = x.shape[1]
    count = np.array([len(events[k]) for k in order], dtype=np.int64)
    s = np.array([x[events[k]].sum(axis=0) for k in order]).reshape(-1, dim)
    q = np.array([(x[events[k]] ** 2).sum(axis=0) for k in order]).reshape(-1, dim)
    frame_event = np.full(int(fo[-1]), -1, dtype=np.int32)
    for e, k in enumerate(order):
        frame_event[events[k]] = e
    if not want_abs:
        return keys, count, s, q, frame_event, skipped
    a = np.array([np.abs(x[events[k]]).sum(axis=0) for k in order]).reshape(-1, dim)
    return keys, count, s, q, frame_event, skipped, a, q


def bound(count: np.ndarray, abs_sum: np.ndarray) -> np.ndarray:
    """Two summation orders of n terms, each term exact and each partial sum rounded once: (2n + 2)·2⁻⁵³·Σ|terms|, per event."""
    return (2 * count[:, None] + 2) * U64 * abs_sum


# ---- the tree ------------------------------------------------------------------------------------------------------------------
def set_loglike(n, s, q, var_floor=0.01):
    if n == 0:
        return 0.0
    mean = s / n
    var = np.maximum(q / n - mean * mean, var_floor)
    return float(-0.5 * n * (len(s) * (np.log(2 * np.pi) + 1) + np.log(var).sum()))


def best_split(stats, event_sets: Sequence[np.ndarray], questions_of_key: Dict[int, Sequence[Sequence[int]]], var_floor=0.01):
    """Every leaf × key × question: (gain, leaf, key, question) of the largest gain, the first in that order among equals."""
    W, pc = stats.windows(), stats.pdf_classes()
    best = (0.0, -1, 0, None)
    for li, ev in enumerate(event_sets):
        whole = set_loglike(stats.count[ev].sum(), stats.sum[ev].sum(axis=0), stats.sumsq[ev].sum(axis=0), var_floor)
        for key in (0, 1, 2, -1):
            vals = pc[ev] if key < 0 else W[ev, key]
            for qs in questions_of_key.get(key, ()):
                yes = np.isin(vals, list(qs))
                if not yes.any() or yes.all():
                    continue
                a, b = ev[yes], ev[~yes]
                g = (set_loglike(stats.count[a].sum(), stats.sum[a].sum(axis=0), stats.sumsq[a].sum(axis=0), var_floor)
                     + set_loglike(stats.count[b].sum(), stats.sum[b].sum(axis=0), stats.sumsq[b].sum(axis=0), var_floor) - whole)
                if g > best[0]:
                    best = (g, li, key, list(qs))
    return best


def transition_tuples(topo: K.HmmTopology, tree: K.ContextDependency):
    """(phone, hmm state, pdf, pdf) for every window (l, phone, r), l and r over the phones and 0, by enumeration."""
    phones = sorted(int(p) for p in topo.phones)
    out = set()
    for c in phones:
        for hs, st in enumerate(topo.entry_for_phone(c)):
            if not st.transitions:
                continue
            for l in [0] + phones:
                for r in [0] + phones:
                    pdf = tree.compute([l, c, r], st.forward_pdf_class)
                    out.add((c, hs, pdf, pdf))
    return sorted(out)
