"""The band kernel's column skip, checked by brute force on the host (no GPU).  Inside the index range the band rule selects
(tests/test_score_plan_cpu.py), gmm_band_kernel scores a class-0 column only if the column's OWN last depth — the largest BFS
depth of a state one of its arcs leaves, not the running maximum the range is built on — is at least the band's lower
bound.  Claim: for ANY set of live states and any window length K, every column a token can ask for within the window
passes `own_last >= lo and first <= hi`.  Random graphs (cycles, skips, dead ends, unreachable states) and a training graph,
as in test_score_plan_cpu.py, whose plan call this reuses."""
import numpy as np

from tests.test_gpu_parity import _random_graph  # plain numpy graph generator (module import needs no GPU)
from tests.test_score_plan_cpu import _plan


def own_last_depths(f, col, sd, n_cols):
    """What gmm_col_own_last_kernel computes: per column, the max over its arcs of the source state's BFS depth (0 where no
    arc names the column; unreachable states carry depth 0 in the plan)."""
    src = np.repeat(np.arange(f.num_states), np.diff(f.arc_offsets))
    own = np.zeros(n_cols, np.int64)
    np.maximum.at(own, col, sd[src, 0])
    return own


def _check_graph(rng, f, pdf_of_arc, pdf_class, span, groups, trials=30):
    sd, col, cp, cf, cl, cc, gc = _plan(f, pdf_of_arc, pdf_class, span, groups)
    S = f.num_states
    own = own_last_depths(f, col, sd, len(cp))
    # the running maximum the plan ships is the running maximum of these own values, run by run
    bounds = np.concatenate([[0], np.cumsum(list(gc) + list(cc[1:]))])
    src = np.repeat(np.arange(S), np.diff(f.arc_offsets))
    nxt = f.arcs["nextstate"].astype(np.int64)
    INF = 1 << 30
    d = np.full(S, INF, np.int64)
    d[f.start] = 0
    for _ in range(S + 1):
        nd = d.copy()
        np.minimum.at(nd, nxt, d[src] + 1)
        if np.array_equal(nd, d):
            break
        d = nd
    reach0 = d < INF
    live_col = np.zeros(len(cp), bool)
    live_col[col[reach0[src]]] = True
    for k in range(len(bounds) - 1):
        seg = np.arange(bounds[k], bounds[k + 1])
        seg = seg[live_col[seg]]
        if len(seg):
            assert np.all(own[seg] <= cl[seg])                      # own ≤ running max: the mask only ever removes columns
    m = sd[:, 1].astype(np.int64)
    adj = [nxt[f.arc_offsets[s]: f.arc_offsets[s + 1]] for s in range(S)]
    states = np.nonzero(reach0)[0]
    checked = skipped = 0
    for _ in range(trials):
        K = int(rng.choice([1, 2, 5, 16, 64]))
        live = rng.choice(states, size=min(len(states), int(rng.integers(1, 12))), replace=False)
        lo, hi = int(m[live].min()), int(d[live].max()) + K - 1
        frontier, seen = set(int(x) for x in live), set(int(x) for x in live)
        for _step in range(K - 1):            # states a token can sit on at frames t0 .. t0+K-1
            nf = set()
            for s in frontier:
                for t in adj[s]:
                    if int(t) not in seen:
                        seen.add(int(t)); nf.add(int(t))
            frontier = nf
        need = set()
        for s in seen:
            need.update(int(c) for c in col[f.arc_offsets[s]: f.arc_offsets[s + 1]])
        for c_ in need:
            assert own[c_] >= lo and cf[c_] <= hi, (K, lo, hi, c_, cf[c_], own[c_], cl[c_])
        checked += len(need)
        in_range = (cl >= lo) & (cf <= hi)
        skipped += int((in_range & (own < lo)).sum())
    return checked, skipped


def test_own_interval_rule_is_a_superset_on_random_graphs(fx):
    rng = np.random.default_rng(78)
    tm = fx.mono_tm
    pdf_class = rng.integers(0, 6, size=tm.num_pdfs).astype(np.int32)
    checked = skipped = 0
    for trial in range(25):
        f = _random_graph(rng, tm, int(rng.choice([3, 8, 40, 150])))
        pdf_of_arc = tm.id2pdf[f.arcs["ilabel"]].astype(np.int32)
        c, s = _check_graph(rng, f, pdf_of_arc, pdf_class, span=int(rng.choice([0, 2, 8, 32])), groups=int(rng.choice([1, 2, 8, 16])))
        checked += c; skipped += s
    assert checked > 0 and skipped > 0          # the rule was asked about real columns, and it does remove some


def test_own_interval_rule_on_a_training_graph(fx):
    rng = np.random.default_rng(6)
    tm = fx.mono_tm
    f = fx.mono_graph("this is the acoustic corpus i'm talking pretty fast here this is the acoustic corpus")
    pdf_of_arc = tm.id2pdf[f.arcs["ilabel"]].astype(np.int32)
    for pdf_class, groups in ((np.full(tm.num_pdfs, 5, np.int32), 1), (np.zeros(tm.num_pdfs, np.int32), 8), (np.zeros(tm.num_pdfs, np.int32), 1)):
        checked, skipped = _check_graph(rng, f, pdf_of_arc, pdf_class, span=32, groups=groups, trials=60)
        assert checked > 0
    assert skipped > 0                          # one run, a text that repeats itself: columns the running maximum kept
