"""Phonetic decision trees from tree statistics: the host half of the reference's triphone stage
(MFA/acoustic_modeling/triphone.py: ``automatically_obtain_questions``, ``build_tree``, ``gmm_init_model``,
``convert_alignments``).

The accumulation is the device's (``stats.tree_statistics``); everything here is float64 numpy on some 10⁴–10⁵ event rows.
The algorithms are Kaldi's (cluster-phones, build-tree, gmm-init-model, convert-ali), restated from their descriptions
(parity unpinned: DESIGN §2).  Two deviations, both chosen so that the result is a function of the statistics alone:
questions come from a bottom-up clustering (Kaldi: top-down, seeded 2-means), and every tie goes to the lowest index.

A set of events with count n, Σx and Σx² is scored by the log-likelihood of its own maximum-likelihood diagonal Gaussian,
variances floored at ``var_floor``:  L = −½·n·(dim·(log 2π + 1) + Σ_k log var_k).
"""
from __future__ import annotations

import copy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import kaldi_io
from .adapt import gconsts
from .stats import TreeStats

VAR_FLOOR = 0.01          # acc-tree-stats' --var-floor; a separate thing from mle.MIN_VARIANCE
KEYS = (0, 1, 2, -1)      # the order in which a leaf's questions are tried: left, centre, right phone, pdf-class
_LOG_2PI_1 = float(np.log(2.0 * np.pi) + 1.0)


def loglike(n, s, q, var_floor: float = VAR_FLOOR):
    """L of pooled events: ``n`` [...], ``s`` / ``q`` [..., dim].  0 where n is 0."""
    n = np.asarray(n, dtype=np.float64)
    s, q = np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    safe = np.where(n > 0, n, 1.0)[..., None]
    mean = s / safe
    var = np.maximum(q / safe - mean * mean, var_floor)
    return np.where(n > 0, -0.5 * n * (s.shape[-1] * _LOG_2PI_1 + np.log(var).sum(axis=-1)), 0.0)


def _pool(stats: TreeStats, mask: np.ndarray):
    return float(stats.count[mask].sum()), stats.sum[mask].sum(axis=0), stats.sumsq[mask].sum(axis=0)


def _agglomerate(n: np.ndarray, s: np.ndarray, q: np.ndarray, var_floor: float, threshold: Optional[float] = None):
    """Bottom-up clustering of rows (n [M], s / q [M, dim]): repeatedly merge the pair with the least likelihood loss — a row
    without data first, at loss 0 —, ties to the lowest indices; the merged row keeps the lower index.  With ``threshold``:
    only while the least loss is below it.  Returns the merges [(i, j, loss)] in order."""
    n, s, q = n.astype(np.float64).copy(), s.astype(np.float64).copy(), q.astype(np.float64).copy()
    M = n.shape[0]
    alive = np.ones(M, dtype=bool)
    own = loglike(n, s, q, var_floor)
    loss = np.full((M, M), np.inf)

    def row(i):
        """loss[i, j] for every live j != i, stored at [min, max]."""
        js = np.flatnonzero(alive)
        js = js[js != i]
        if js.size == 0:
            return
        l = own[i] + own[js] - loglike(n[i] + n[js], s[i] + s[js], q[i] + q[js], var_floor)
        l = np.where((n[js] == 0) | (n[i] == 0), -np.inf, l)
        lo, hi = np.minimum(js, i), np.maximum(js, i)
        loss[lo, hi] = l

    for i in range(M):
        row(i)
    merges = []
    for _ in range(M - 1):
        flat = int(np.argmin(loss))                 # the first minimum in row-major order: the lowest (i, j)
        i, j = divmod(flat, M)
        l = loss[i, j]
        if not l < np.inf:
            break
        value = 0.0 if l == -np.inf else float(l)
        if threshold is not None and not value < threshold:
            break
        merges.append((i, j, value))
        n[i] += n[j]; s[i] += s[j]; q[i] += q[j]
        own[i] = loglike(n[i], s[i], q[i], var_floor)
        alive[j] = False
        loss[j, :] = np.inf
        loss[:, j] = np.inf
        row(i)
    return merges


def automatic_questions(stats: TreeStats, phone_sets: Sequence[Sequence[int]], pdf_classes: Sequence[int] = (1,),
                        position: int = 1, var_floor: float = VAR_FLOOR) -> List[List[int]]:
    """Phone questions from the data.  Per phone set, the events whose phone at ``position`` is in the set and whose
    pdf-class is in ``pdf_classes`` are pooled; the sets are clustered bottom-up (``_agglomerate``).  The questions are the
    phone sets under every node of the resulting binary tree except the root, plus every input set — each sorted, duplicates
    dropped: the input sets in their order, then the merged nodes in the order they were made."""
    sets = [sorted(int(p) for p in s) for s in phone_sets]
    if not sets or any(not s for s in sets):
        raise ValueError("automatic_questions: empty phone set")
    dim = stats.dim
    W, pc = stats.windows(), stats.pdf_classes()
    in_class = np.isin(pc, np.asarray(list(pdf_classes), dtype=np.int32))
    n, s, q = np.zeros(len(sets)), np.zeros((len(sets), dim)), np.zeros((len(sets), dim))
    for i, ph in enumerate(sets):
        n[i], s[i], q[i] = _pool(stats, in_class & np.isin(W[:, position], ph))
    members = [list(ph) for ph in sets]
    out: List[List[int]] = []
    seen = set()

    def add(ph):
        key = tuple(sorted(set(ph)))
        if key not in seen:
            seen.add(key)
            out.append(list(key))

    for ph in sets:
        add(ph)
    merges = _agglomerate(n, s, q, var_floor)
    for k, (i, j, _loss) in enumerate(merges):
        members[i] = members[i] + members[j]
        if k < len(sets) - 2:                      # the last merge of a complete clustering is the root
            add(members[i])
    return out


# ---- the tree ------------------------------------------------------------------------------------------------------------------
class _Leaf:
    """A node of the tree under construction: a leaf (``events``) until it is split (``key``, ``yes_set``, ``yes``, ``no``)."""

    def __init__(self, events: np.ndarray, root: int, group: int, splittable: bool):
        self.events, self.root, self.group, self.splittable = events, root, group, splittable
        self.key: Optional[int] = None
        self.yes_set: frozenset = frozenset()
        self.yes: Optional["_Leaf"] = None
        self.no: Optional["_Leaf"] = None
        self.best: Tuple[float, int, int] = (0.0, 0, -1)      # gain, key, question index (-1: none)
        self.pdf = -1


def _pdf_classes(topology: kaldi_io.HmmTopology, phones: Sequence[int]) -> List[int]:
    return sorted({c for ph in phones for st in topology.entry_for_phone(ph)
                   for c in (st.forward_pdf_class, st.self_loop_pdf_class) if c >= 0 and st.transitions})


def _question_tables(questions, max_value: int) -> np.ndarray:
    """[Q, max_value + 1] bool: the value is in the question's set."""
    m = np.zeros((len(questions), max_value + 1), dtype=bool)
    for i, qs in enumerate(questions):
        v = np.asarray([x for x in qs if 0 <= x <= max_value], dtype=np.int64)
        m[i, v] = True
    return m


def build_tree(topology: kaldi_io.HmmTopology, questions: Sequence[Sequence[int]], stats: TreeStats,
               roots: Sequence[Tuple[Sequence[int], bool, bool]], max_leaves: int = 1000, cluster_thresh: float = -1.0,
               var_floor: float = VAR_FLOOR):
    """The decision tree of a width-3 context.  ``roots``: (phones, shared, split) as in the reference's ``roots.int`` —
    ``shared``: one initial leaf for all pdf-classes of the set, otherwise one per pdf-class; not ``split``: those leaves are
    never split.  Questions on keys 0, 1, 2 (left, centre, right phone): ``questions``; on key −1 (pdf-class): {0..k} for every
    k below the largest pdf-class.

    Greedy splitting: of all splittable leaves, the one whose best (key, question) has the largest gain is split, while that
    gain is positive and the leaves number fewer than ``max_leaves``; both sides of a split must hold data.  Ties: the key
    earlier in (0, 1, 2, −1), then the earlier question, then the earlier leaf.  Then, inside every initial leaf's subtree, the
    pair of leaves with the least loss is merged while the loss is below the threshold (``cluster_thresh`` < 0: the smallest
    gain of any split made): merged leaves share a pdf.  Pdfs are numbered 0..n−1 in order of first appearance in a depth-first
    walk (tables in index order, yes before no).

    Returns (``kaldi_io.ContextDependency(3, 1, …)`` of TE / SE / CE nodes, record): ``record`` holds ``splits`` (dicts of
    root, key, question, gain, in order; ``node`` and ``children`` number the nodes — the initial leaves first, then every
    split's two children — so that the order of the splits can be checked), ``initial_leaves``, ``merges`` (root, loss), ``total_gain`` = Σ gain, ``merge_loss`` = Σ loss,
    ``frames`` and ``leaves``."""
    phone_q = [sorted(int(p) for p in qs) for qs in questions]
    W, pc = stats.windows(), stats.pdf_classes()
    cnt, S, Q2 = stats.count.astype(np.float64), stats.sum, stats.sumsq
    max_phone = int(max(int(p) for p in topology.phones))
    all_classes = _pdf_classes(topology, [int(p) for p in topology.phones])
    max_class = max(all_classes) if all_classes else 0
    class_q = [list(range(k + 1)) for k in range(max_class)]
    q_of_key = {0: phone_q, 1: phone_q, 2: phone_q, -1: class_q}
    t_of_key = {k: _question_tables(q_of_key[k], max_phone if k >= 0 else max_class) for k in KEYS}

    def values(key, ev):
        return pc[ev] if key < 0 else W[ev, key]

    def evaluate(leaf: _Leaf) -> None:
        leaf.best = (0.0, 0, -1)
        ev = leaf.events
        if not leaf.splittable or ev.size < 2:
            return
        n, s, q = cnt[ev], S[ev], Q2[ev]
        N, Ss, Qs = n.sum(), s.sum(axis=0), q.sum(axis=0)
        whole = float(loglike(N, Ss, Qs, var_floor))
        for key in KEYS:
            tab = t_of_key[key]
            if tab.shape[0] == 0:
                continue
            yes = tab[:, values(key, ev)].astype(np.float64)           # [Q, events of the leaf]
            ny, sy, qy = yes @ n, yes @ s, yes @ q
            gain = loglike(ny, sy, qy, var_floor) + loglike(N - ny, Ss - sy, Qs - qy, var_floor) - whole
            # both sides must hold events (a side whose frames sum to 0 cannot occur: an event has at least one frame)
            both = (yes.sum(axis=1) > 0) & (yes.sum(axis=1) < ev.size)
            gain = np.where(both, gain, -np.inf)
            i = int(np.argmax(gain))
            if gain[i] > leaf.best[0]:
                leaf.best = (float(gain[i]), key, i)

    table: List[Optional[object]] = [None] * (max_phone + 1)
    leaves: List[_Leaf] = []
    tops = []
    seen_phones = set()
    for r, (phones, shared, split) in enumerate(roots):
        phones = sorted(int(p) for p in phones)
        if not phones or seen_phones & set(phones) or any(p < 1 or p > max_phone for p in phones):
            raise ValueError(f"build_tree: root {r} is empty, repeats a phone or names one outside the topology")
        seen_phones |= set(phones)
        classes = _pdf_classes(topology, phones)
        mine = np.flatnonzero(np.isin(W[:, 1], phones))
        if shared:
            top = _Leaf(mine, r, len(tops), bool(split))
            leaves.append(top)
        else:
            top = [None] * (max(classes) + 1 if classes else 0)
            for c in classes:
                top[c] = _Leaf(mine[pc[mine] == c], r, len(tops), bool(split))
                leaves.append(top[c])
        tops.append(top)
        for p in phones:
            table[p] = top
    for lf in leaves:
        evaluate(lf)
    n_leaves = len(leaves)
    splits = []
    while n_leaves < int(max_leaves):
        best = None
        for lf in leaves:
            if lf.key is None and lf.best[2] >= 0 and (best is None or lf.best[0] > best.best[0]):
                best = lf
        if best is None or not best.best[0] > 0:
            break
        gain, key, qi = best.best
        qs = q_of_key[key][qi]
        yes_mask = t_of_key[key][qi][values(key, best.events)]
        best.key, best.yes_set = key, frozenset(qs)
        best.yes = _Leaf(best.events[yes_mask], best.root, best.group, True)
        best.no = _Leaf(best.events[~yes_mask], best.root, best.group, True)
        node = next(i for i, lf in enumerate(leaves) if lf is best)
        for child in (best.yes, best.no):
            evaluate(child)
            leaves.append(child)
        splits.append(dict(root=best.root, key=key, question=list(qs), gain=gain, node=node,
                           children=(len(leaves) - 2, len(leaves) - 1)))
        n_leaves += 1

    # bottom-up clustering inside every initial leaf's subtree
    def final_leaves(node, out):
        if node is None:
            return out
        if isinstance(node, list):
            for t in node:
                final_leaves(t, out)
        elif node.key is None:
            out.append(node)
        else:
            final_leaves(node.yes, out)
            final_leaves(node.no, out)
        return out

    thresh = float(cluster_thresh) if cluster_thresh >= 0 else (min(sp["gain"] for sp in splits) if splits else 0.0)
    merges = []
    rep: Dict[int, _Leaf] = {}
    for top in tops:
        for start in (top if isinstance(top, list) else [top]):
            if start is None:
                continue
            fl = final_leaves(start, [])
            for lf in fl:
                rep[id(lf)] = lf
            if len(fl) < 2:
                continue
            n = np.array([cnt[lf.events].sum() for lf in fl])
            s = np.stack([S[lf.events].sum(axis=0) for lf in fl])
            q = np.stack([Q2[lf.events].sum(axis=0) for lf in fl])
            for i, j, loss in _agglomerate(n, s, q, var_floor, threshold=thresh):
                merges.append(dict(root=fl[i].root, loss=loss))
                for lf in fl:
                    if rep[id(lf)] is fl[j]:
                        rep[id(lf)] = fl[i]

    # pdfs in order of first appearance, and the EventMap
    n_pdfs = 0

    def emit(node):
        nonlocal n_pdfs
        if node is None:
            return None
        if isinstance(node, list):
            return kaldi_io.EventMap("TE", key=-1, table=[emit(t) for t in node])
        if node.key is None:
            r = rep[id(node)]
            if r.pdf < 0:
                r.pdf = n_pdfs
                n_pdfs += 1
            return kaldi_io.EventMap("CE", answer=r.pdf)
        yes = emit(node.yes)
        return kaldi_io.EventMap("SE", key=node.key, yes_set=node.yes_set, yes=yes, no=emit(node.no))

    done: Dict[int, kaldi_io.EventMap] = {}
    out_table: List[Optional[kaldi_io.EventMap]] = [None] * (max_phone + 1)
    for p in range(max_phone + 1):
        top = table[p]
        if top is None:
            continue
        if id(top) not in done:
            done[id(top)] = emit(top)
        out_table[p] = done[id(top)]
    tree = kaldi_io.ContextDependency(3, 1, kaldi_io.EventMap("TE", key=1, table=out_table))
    record = dict(splits=splits, merges=merges, total_gain=float(sum(sp["gain"] for sp in splits)),
                  merge_loss=float(sum(m["loss"] for m in merges)), frames=float(cnt.sum()), leaves=n_pdfs,
                  initial_leaves=len(leaves) - 2 * len(splits))
    return tree, record


def event_leaves(tree: kaldi_io.ContextDependency, stats: TreeStats) -> np.ndarray:
    """[E] int32: the pdf the tree gives every event (−1: the tree has no leaf for it)."""
    if (tree.context_width, tree.central_position) != (3, 1):
        raise ValueError(f"event_leaves: a tree of context width {tree.context_width}, position {tree.central_position}: only 3, 1")
    W, pc = stats.windows(), stats.pdf_classes()
    out = np.full(stats.num_events, -1, dtype=np.int32)

    def walk(node, idx):
        """The events ``idx`` go down from ``node`` together: one numpy selection per node, not a walk per event."""
        if node is None or idx.size == 0:
            return
        if node.kind == "CE":
            out[idx] = node.answer
            return
        v = pc[idx] if node.key == -1 else W[idx, node.key]
        if node.kind == "TE":
            for value in np.unique(v):
                if 0 <= value < len(node.table):
                    walk(node.table[int(value)], idx[v == value])
            return
        yes = np.isin(v, np.fromiter(node.yes_set, dtype=np.int64, count=len(node.yes_set)))
        walk(node.yes, idx[yes])
        walk(node.no, idx[~yes])

    walk(tree.to_pdf, np.arange(stats.num_events))
    return out


def reachable_leaves(tree: kaldi_io.ContextDependency, phone: int, pdf_class: int, context: Sequence[int]) -> List[int]:
    """Every pdf some window (l, ``phone``, r) with l, r in ``context`` reaches at ``pdf_class``: a walk of the tree that
    carries the values still possible for l and r, not an enumeration of windows."""
    P = tree.central_position
    found = set()

    def walk(node, allowed: Dict[int, frozenset]):
        if node is None:
            return
        if node.kind == "CE":
            found.add(int(node.answer))
            return
        fixed = pdf_class if node.key == -1 else (phone if node.key == P else None)
        if node.kind == "TE":
            if fixed is not None:
                if 0 <= fixed < len(node.table):
                    walk(node.table[fixed], allowed)
                return
            for v in sorted(allowed[node.key]):
                if 0 <= v < len(node.table):
                    walk(node.table[v], {**allowed, node.key: frozenset([v])})
            return
        if fixed is not None:
            walk(node.yes if fixed in node.yes_set else node.no, allowed)
            return
        yes, no = allowed[node.key] & node.yes_set, allowed[node.key] - node.yes_set
        if yes:
            walk(node.yes, {**allowed, node.key: yes})
        if no:
            walk(node.no, {**allowed, node.key: no})

    ctx = frozenset(int(v) for v in context)
    walk(tree.to_pdf, {k: ctx for k in range(tree.context_width) if k != P})
    return sorted(found)


def _check_topology(topology: kaldi_io.HmmTopology, what: str) -> None:
    for e in topology.entries:
        for st in e:
            if st.transitions and st.forward_pdf_class != st.self_loop_pdf_class:
                raise ValueError(f"{what}: a topology state with forward pdf-class {st.forward_pdf_class} and self-loop pdf-class "
                                 f"{st.self_loop_pdf_class}: only topologies where the two are equal")


def init_model(topology: kaldi_io.HmmTopology, tree: kaldi_io.ContextDependency, stats: TreeStats, var_floor: float = VAR_FLOOR):
    """gmm-init-model: (RawTransitionModel, RawAmDiagGmm) on a tree.  One Gaussian per leaf from the pooled events that map to
    it (variances floored at ``var_floor``); a leaf without data takes the global mean and variance.  Transition tuples
    (phone, hmm_state, pdf, pdf) for every leaf reachable with that centre phone and pdf-class (``reachable_leaves``; the
    context is every phone of the topology and 0, the utterance's edge), sorted ascending; log-probabilities from the
    topology."""
    _check_topology(topology, "init_model")
    topo = copy.deepcopy(topology)
    dim = stats.dim
    leaf = event_leaves(tree, stats)
    n_pdfs = max(tree.to_pdf.leaves()) + 1
    n, s, q = np.zeros(n_pdfs), np.zeros((n_pdfs, dim)), np.zeros((n_pdfs, dim))
    ok = leaf >= 0
    np.add.at(n, leaf[ok], stats.count[ok].astype(np.float64))
    np.add.at(s, leaf[ok], stats.sum[ok])
    np.add.at(q, leaf[ok], stats.sumsq[ok])
    N = float(stats.count.sum())
    if not N > 0:
        raise ValueError("init_model: the statistics hold no frame")
    gmean = stats.sum.sum(axis=0) / N
    gvar = np.maximum(stats.sumsq.sum(axis=0) / N - gmean * gmean, var_floor)
    one = np.ones(1, np.float32)
    am = kaldi_io.RawAmDiagGmm(dim, [], [], [], [])
    for p in range(n_pdfs):
        mean, var = gmean, gvar
        if n[p] > 0:
            mean = s[p] / n[p]
            var = np.maximum(q[p] / n[p] - mean * mean, var_floor)
        iv = (1.0 / var).astype(np.float32)[None]
        mi = mean.astype(np.float32)[None] * iv
        am.gconsts.append(gconsts(one, mi, iv)); am.weights.append(one.copy())
        am.means_invvars.append(mi); am.inv_vars.append(iv)
    phones = sorted(int(p) for p in topo.phones)
    context = [0] + phones
    tuples = []
    for ph in phones:
        for hs, st in enumerate(topo.entry_for_phone(ph)):
            if not st.transitions:
                continue
            for pdf in reachable_leaves(tree, ph, st.forward_pdf_class, context):
                tuples.append((ph, hs, pdf, pdf))
    tuples.sort()
    log_probs = [np.float32(0.0)]
    for ph, hs, _f, _s in tuples:
        for _dst, prob in topo.entry_for_phone(ph)[hs].transitions:
            log_probs.append(np.log(np.float32(prob)))
    raw_tm = kaldi_io.RawTransitionModel(topo, np.asarray(tuples, dtype=np.int32).reshape(-1, 4), np.asarray(log_probs, dtype=np.float32))
    return raw_tm, am


# ---- alignment conversion ------------------------------------------------------------------------------------------------------
def _same_topology(a: kaldi_io.HmmTopology, b: kaldi_io.HmmTopology) -> bool:
    return (np.array_equal(a.phones, b.phones) and np.array_equal(a.phone2idx, b.phone2idx) and len(a.entries) == len(b.entries)
            and all(len(x) == len(y) and all((s.forward_pdf_class, s.self_loop_pdf_class, [d for d, _p in s.transitions])
                                             == (t.forward_pdf_class, t.self_loop_pdf_class, [d for d, _p in t.transitions])
                                             for s, t in zip(x, y)) for x, y in zip(a.entries, b.entries)))


def local_transitions(topology: kaldi_io.HmmTopology, phone: int) -> List[Tuple[int, int]]:
    """The arcs of a phone's topology entry as (hmm state, index among the state's transitions), in order: the position in
    this list is the arc's local transition index."""
    return [(hs, k) for hs, st in enumerate(topology.entry_for_phone(phone)) for k in range(len(st.transitions))]


def local_of_tid(tm) -> np.ndarray:
    """[transition-ids + 1] int32: every transition-id's local transition index inside its phone's topology entry (0 at 0)."""
    out = np.zeros(tm.num_transition_ids + 1, dtype=np.int32)
    index = {}
    for tid in range(1, tm.num_transition_ids + 1):
        ts = int(tm.id2state[tid])
        ph, hs = int(tm.tuples[ts - 1, 0]), int(tm.tuples[ts - 1, 1])
        if ph not in index:
            index[ph] = {arc: i for i, arc in enumerate(local_transitions(tm.topo, ph))}
        out[tid] = index[ph][(hs, tid - int(tm.state2id[ts]))]
    return out


def convert_table(old_tm, new_tm, tree: kaldi_io.ContextDependency, batch_stats: TreeStats) -> np.ndarray:
    """[E_b, L] int32: for every event of a batch and every local transition index of its centre phone's topology entry, the
    transition-id of the new model whose pdf is the event's own leaf (0 where the arc's pdf-class is not the event's, or the
    entry has fewer arcs).  With ``frame_event`` of the batch, ``new_ali = table[frame_event, local_of_tid(old_tm)[ali]]``;
    frames of skipped utterances (event −1) become 0.  ``old_tm`` / ``new_tm``: ``model.TransitionModel`` on one topology."""
    if not _same_topology(old_tm.topo, new_tm.topo):
        raise ValueError("convert_table: the old and the new model differ in their topology")
    _check_topology(new_tm.topo, "convert_table")
    state_of = {tuple(int(v) for v in row): ts + 1 for ts, row in enumerate(new_tm.tuples)}
    L = max(len(local_transitions(new_tm.topo, int(p))) for p in new_tm.topo.phones)
    W, pc = batch_stats.windows(), batch_stats.pdf_classes()
    leaf = event_leaves(tree, batch_stats)
    table = np.zeros((batch_stats.num_events, L), dtype=np.int32)
    # one row per distinct (centre phone, pdf-class, leaf) — some thousands —, then a gather over the events
    combos, inverse = np.unique(np.stack([W[:, 1], pc, leaf], axis=1), axis=0, return_inverse=True)
    rows = np.zeros((combos.shape[0], L), dtype=np.int32)
    for r, (ph, c, pdf) in enumerate(combos.tolist()):
        entry = new_tm.topo.entry_for_phone(ph)
        for i, (hs, k) in enumerate(local_transitions(new_tm.topo, ph)):
            if entry[hs].forward_pdf_class != c:
                continue
            ts = state_of.get((ph, hs, pdf, pdf))
            if ts is None:
                raise ValueError(f"convert_table: the new model has no state for phone {ph}, hmm state {hs}, pdf {pdf}")
            rows[r, i] = int(new_tm.state2id[ts]) + k
    if batch_stats.num_events:
        table = rows[inverse.reshape(-1)]
    return table


def convert_alignments(table: np.ndarray, local: np.ndarray, frame_event, ali):
    """The gather of ``convert_table`` on numpy arrays or on torch tensors of one device (no kernel of ours): frames without
    an event become 0."""
    if isinstance(frame_event, np.ndarray):
        ev = np.asarray(frame_event, dtype=np.int64)
        a = np.asarray(ali, dtype=np.int64)
        ok = (ev >= 0) & (a > 0) & (a < local.shape[0])
        if table.shape[0] == 0:
            return np.zeros(a.shape[0], dtype=np.int32)
        out = table[np.where(ok, ev, 0), local[np.where(ok, a, 0)]]
        return np.where(ok, out, 0).astype(np.int32)
    import torch

    dev = frame_event.device
    ev, a = frame_event.long(), ali.long()
    ok = (ev >= 0) & (a > 0) & (a < int(local.shape[0]))
    if table.shape[0] == 0:
        return torch.zeros_like(ali, dtype=torch.int32)
    t, l = torch.from_numpy(np.ascontiguousarray(table)).to(dev), torch.from_numpy(np.ascontiguousarray(local)).to(dev).long()
    zero = torch.zeros_like(ev)
    out = t[torch.where(ok, ev, zero), l[torch.where(ok, a, zero)]]
    return torch.where(ok, out, torch.zeros_like(out)).to(torch.int32)
