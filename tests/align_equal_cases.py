"""The equal alignment's case set, shared by tests/test_align_equal_cpu.py (the host twin) and tests/test_gpu_align_equal.py
(the device against the twin): 70 utterances of 0 – 300 frames, and the checks that need no reference — the id sequence is
accepted by the graph, and the loops are spread evenly over the path's loopable states, the larger counts first."""
from __future__ import annotations

from functools import lru_cache
from typing import List, NamedTuple, Optional

import numpy as np

import synth_workload as S
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import kaldi_io as K
from tests import helpers

INF = np.float32(np.inf)


class Case(NamedTuple):
    name: str
    fst: K.Fst
    T: int
    status: Optional[int]      # what the contract demands, None where the case leaves it to the walk
    branching: bool


def make_fst(n_states: int, arcs, finals, start: int = 0) -> K.Fst:
    """arcs: (src, ilabel, dst) triples, kept in the order given inside every state."""
    by_state = [[a for a in arcs if a[0] == s] for s in range(n_states)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in by_state])]).astype(np.int64)
    arr = np.zeros(int(offs[-1]), dtype=K.ARC_DTYPE)
    k = 0
    for lst in by_state:
        for _s, il, d in lst:
            arr[k] = (il, 0, 0.0, d)
            k += 1
    final = np.full(n_states, INF, dtype=np.float32)
    final[list(finals)] = 0.0
    return K.Fst(start, offs, arr, final)


def shortest_labels(fst: K.Fst) -> int:
    """Fewest non-zero input labels on a path from the start to a final state (self-loops never help)."""
    dist = np.full(fst.num_states, np.iinfo(np.int64).max, dtype=np.int64)
    dist[fst.start] = 0
    changed = True
    while changed:
        changed = False
        for s in range(fst.num_states):
            if dist[s] == np.iinfo(np.int64).max:
                continue
            for a in range(int(fst.arc_offsets[s]), int(fst.arc_offsets[s + 1])):
                d = int(fst.arcs["nextstate"][a])
                c = dist[s] + (1 if fst.arcs["ilabel"][a] != 0 else 0)
                if c < dist[d]:
                    dist[d] = c
                    changed = True
    return int(dist[np.isfinite(fst.final)].min())


@lru_cache(maxsize=1)
def world() -> S.SynthWorld:
    return S.SynthWorld.build(n_words=40)


@lru_cache(maxsize=1)
def compiled_graphs() -> List[K.Fst]:
    """Training graphs of 1 – 3 words of the synthetic lexicon with optional silences (the silence model's cyclic inner
    states among them), plain and with epsilon input arcs."""
    w = world()
    model = S.monophone_from_stats(w.lexicon, {(1, 0): [np.zeros(3), np.ones(3), 10]})
    gc = G.TrainingGraphCompiler(model.tm, model.tree, w.lexicon)
    rng = np.random.default_rng(5)
    out = []
    for n in (1, 2, 3):
        f = gc.compile_fst(" ".join(w.words[3 * n + k] for k in range(n)))
        out += [f, helpers.with_eps(rng, f, 0.4)]
    return out


@lru_cache(maxsize=1)
def cases() -> List[Case]:
    chain = make_fst(6, [(s, 10 + s, s + 1) for s in range(5)], [5])
    # two routes of 2 and 4 labels, loops on some states, an epsilon arc, a loop that carries no label (never a loop)
    fork = make_fst(7, [(0, 1, 1), (0, 2, 3), (1, 11, 1), (1, 3, 6), (3, 0, 4), (4, 14, 4), (4, 4, 5), (5, 0, 5), (5, 5, 2),
                        (2, 12, 2), (2, 6, 6)], [6])
    eps_cycle = make_fst(3, [(0, 0, 1), (1, 0, 0), (1, 7, 1)], [2])             # the final state is never reached
    dead_end = make_fst(3, [(0, 1, 1), (1, 9, 1)], [2])                          # state 1: a loop and nothing else
    start_final = make_fst(1, [(0, 5, 0)], [0])
    out = [
        Case("chain T=len", chain, 5, 0, False), Case("chain T=len+1", chain, 6, 2, False),
        Case("chain T=len-1", chain, 4, 2, False), Case("chain T=0", chain, 0, 2, False),
        Case("fork T=shortest", fork, 2, None, True), Case("fork T=9", fork, 9, 0, True),
        Case("eps cycle", eps_cycle, 12, 2, False), Case("dead end", dead_end, 8, 2, False),
        Case("final start T=0", start_final, 0, 0, False), Case("final start T=7", start_final, 7, 0, False),
    ]
    for k, f in enumerate(compiled_graphs()):
        m = shortest_labels(f)
        for T in (m - 1, m, m + 1, m + 2, m + 13, 64, 100, 129, 177, 300):
            out.append(Case(f"graph {k} T={T}", f, T, 2 if T < m else None, True))
    assert len(out) == 70
    return out


def frame_offsets(cs) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([c.T for c in cs])]).astype(np.int64)


def trace(fst: K.Fst, ali: np.ndarray):
    """A path of the graph that spells ``ali`` and ends in a final state, as a list of [state, loops taken there] in path
    order, or None when the graph does not accept the sequence.  Sets of states per consumed label, epsilon arcs closed,
    with one predecessor kept per (labels consumed, state)."""
    off, arcs = fst.arc_offsets, fst.arcs
    pred = [dict() for _ in range(len(ali) + 1)]

    def close(t):
        stack = list(pred[t])
        while stack:
            s = stack.pop()
            for a in range(int(off[s]), int(off[s + 1])):
                d = int(arcs["nextstate"][a])
                if arcs["ilabel"][a] == 0 and d != s and d not in pred[t]:
                    pred[t][d] = (t, s)
                    stack.append(d)

    pred[0][int(fst.start)] = None
    close(0)
    for t, lab in enumerate(ali):
        for s in list(pred[t]):
            for a in range(int(off[s]), int(off[s + 1])):
                d = int(arcs["nextstate"][a])
                if arcs["ilabel"][a] == lab and d not in pred[t + 1]:
                    pred[t + 1][d] = (t, s)
        close(t + 1)
        if not pred[t + 1]:
            return None
    ends = [s for s in pred[len(ali)] if np.isfinite(fst.final[s])]
    if not ends:
        return None
    steps, t, s = [], len(ali), ends[0]
    while pred[t][s] is not None:
        pt, ps = pred[t][s]
        steps.append((ps, s))
        t, s = pt, ps
    path = [[int(fst.start), 0]]
    for ps, s in reversed(steps):
        if s == ps:
            path[-1][1] += 1
        else:
            path.append([s, 0])
    return path


def loopable(fst: K.Fst, s: int) -> bool:
    a0, a1 = int(fst.arc_offsets[s]), int(fst.arc_offsets[s + 1])
    return bool(np.any((fst.arcs["nextstate"][a0:a1] == s) & (fst.arcs["ilabel"][a0:a1] != 0)))


def check_result(c: Case, ali: np.ndarray, status: int) -> None:
    """What holds for every utterance whatever the random numbers were."""
    assert ali.shape == (c.T,), c.name
    assert status in (0, 2), c.name
    if c.status is not None:
        assert status == c.status, (c.name, status)
    if status == 2:
        assert not ali.any(), c.name
        return
    assert np.all(ali != 0), c.name                          # exactly T_u non-zero ids
    path = trace(c.fst, ali)
    assert path is not None, f"{c.name}: the graph does not accept the alignment"
    counts = [n for s, n in path if loopable(c.fst, s)]
    assert sum(n for _s, n in path) == sum(counts), c.name
    if counts:
        assert max(counts) - min(counts) <= 1, (c.name, counts)
        assert all(a >= b for a, b in zip(counts, counts[1:])), (c.name, counts)     # the larger ones first
