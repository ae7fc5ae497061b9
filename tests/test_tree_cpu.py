"""The triphone stage without a GPU: the host twin of the tree statistics (mfa_debug_tree_acc_host) against the dict-of-events
restatement of tests/tree_ref.py, ``TreeStats`` addition, ``tree.automatic_questions`` / ``build_tree`` / ``init_model`` /
``convert_table`` on planted statistics against brute force and exhaustive enumeration, the refusals, and the twin's
translation unit under the host sanitizers as a stand-alone program (nothing is preloaded anywhere)."""
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib, kaldi_io, tree
from montreal_forced_aligner_amd.model import TransitionModel
from montreal_forced_aligner_amd.stats import TreeStats, tree_key, tree_statistics_host
from tests import tree_ref as R

ROOT = Path(__file__).resolve().parents[1]


def host(case):
    return tree_statistics_host(case.feats, case.frame_off, case.ali, case.tm, case.ci)


def assert_equal_to_ref(case, got, exact=True):
    st, fe, skipped = got
    keys, count, s, q, rfe, rskipped, a1, a2 = R.accumulate(case, want_abs=True)
    assert skipped == rskipped
    assert np.array_equal(st.keys, keys) and st.keys.dtype == np.uint64
    assert np.array_equal(fe, rfe)
    assert np.array_equal(st.count, count)
    if exact:
        assert np.array_equal(st.sum, s) and np.array_equal(st.sumsq, q)
    else:
        assert np.all(np.abs(st.sum - s) <= R.bound(count, a1)) and np.all(np.abs(st.sumsq - q) <= R.bound(count, a2))
    return st


# ---- the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 13, 48])
def test_twin_exact_on_integers(dim):
    case = R.make_case(np.random.default_rng(dim), list(R.LENGTHS) + [300], dim)
    st = assert_equal_to_ref(case, host(case))
    # lengths 1 and 2 are whole utterances of one-frame phones; the context-independent centres have no context
    W = st.windows()
    assert st.num_events > 20 and np.all(W[np.isin(W[:, 1], R.CI)][:, [0, 2]] == 0)
    assert (W[~np.isin(W[:, 1], R.CI)][:, [0, 2]] != 0).any()
    assert int(st.count.sum()) == int(case.frame_off[-1])
    assert set(st.pdf_classes()) == {0, 1, 2}


def test_twin_on_real_features_within_the_derived_bound():
    case = R.make_case(np.random.default_rng(3), [400, 1, 129, 64, 700], 13, integer=False)
    assert_equal_to_ref(case, host(case), exact=False)


def test_segment_cases():
    tm = R.mono_tm()
    # a three-state phone across the 64-frame step, one-frame phones at the utterance's edges and next to each other
    ali = np.concatenate([R.phone_path(tm, 3, [1]), R.phone_path(tm, 4, [30, 40, 20]), R.phone_path(tm, 6, [1]),
                          R.phone_path(tm, 9, [1]), R.phone_path(tm, 1, [5, 60, 5]), R.phone_path(tm, 3, [1])]).astype(np.int32)
    x = np.random.default_rng(0).integers(-8, 9, size=(len(ali), 4)).astype(np.float32)
    case = R.Case(tm, x, np.array([0, len(ali)], dtype=np.int64), ali, R.CI)
    st = assert_equal_to_ref(case, host(case))
    W = st.windows().tolist()
    assert [0, 3, 4] in W and [3, 4, 6] in W and [4, 6, 9] in W and [6, 9, 1] in W and [0, 1, 0] in W and [1, 3, 0] in W
    assert st.count[(st.keys == tree_key(3, 4, 6, 1))][0] == 40


def test_skipped_utterances_leave_no_trace():
    rng = np.random.default_rng(9)
    case = R.make_case(rng, [50, 64, 65, 129, 40], 5)
    tm, fo = case.tm, case.frame_off
    case.ali[fo[1] + 7] = 0                                             # a transition-id 0
    case.ali[fo[3] - 1] = R.phone_path(tm, 4, [2, 1, 1])[0]             # an unfinished last phone (a self-loop)
    seg = R.phone_path(tm, 4, [1, 1, 1])
    case.ali[fo[3]: fo[3] + 3] = [seg[0], R.phone_path(tm, 5, [1, 1, 1])[1], seg[2]]   # a phone change inside a segment
    case.ali[fo[3] + 3: fo[4]] = R.utterance(rng, tm, 126)
    st, fe, skipped = host(case)
    assert skipped == 3
    assert np.all(fe[fo[1]: fo[4]] == -1) and np.all(fe[: fo[1]] >= 0) and np.all(fe[fo[4]:] >= 0)
    assert_equal_to_ref(case, (st, fe, skipped))
    # the same events as the two utterances that take part give on their own
    keep = np.r_[0: fo[1], fo[4]: fo[5]]
    alone = R.Case(tm, case.feats[keep], np.array([0, 50, 90], dtype=np.int64), case.ali[keep], case.ci)
    st2, _fe, _s = host(alone)
    assert np.array_equal(st.keys, st2.keys) and np.array_equal(st.sum, st2.sum) and np.array_equal(st.count, st2.count)
    # an id past the table
    case.ali[3] = tm.num_transition_ids + 1
    assert host(case)[2] == 4


def test_tree_stats_addition_and_batch_cuts():
    case = R.make_case(np.random.default_rng(4), [70, 3, 90, 129, 64, 11, 200], 6)
    whole, _fe, _s = host(case)
    fo = case.frame_off

    def part(a, b):
        return tree_statistics_host(case.feats[fo[a]: fo[b]], fo[a: b + 1] - fo[a], case.ali[fo[a]: fo[b]], case.tm, case.ci)[0]

    for cuts in ([0, 3, 7], [0, 1, 2, 6, 7], [0, 7]):
        tot = TreeStats.zeros(6)
        for a, b in zip(cuts, cuts[1:]):
            tot += part(a, b)
        assert np.array_equal(tot.keys, whole.keys) and np.array_equal(tot.count, whole.count)
        assert np.array_equal(tot.sum, whole.sum) and np.array_equal(tot.sumsq, whole.sumsq)
    a = part(0, 3)
    b = a.copy()
    b += a
    assert np.array_equal(b.keys, a.keys) and np.array_equal(b.sum, 2 * a.sum) and np.array_equal(b.count, 2 * a.count)
    with pytest.raises(ValueError, match="dimensions"):
        b += TreeStats.zeros(5)


def test_twin_refusals():
    case = R.make_case(np.random.default_rng(2), [5], 49)
    with pytest.raises(_lib.MfaHipError, match="48"):
        host(case)
    lib = _lib.lib()
    assert lib.mfa_tree_acc_max_dim() == 48 == lib.mfa_gmm_acc_max_dim() and lib.mfa_tree_acc_chunk_frames() >= 64
    ok = R.make_case(np.random.default_rng(2), [5], 4)
    with pytest.raises(_lib.MfaHipError, match="only 3 and 1"):
        tree_statistics_host(ok.feats, ok.frame_off, ok.ali, ok.tm, ok.ci, context_width=5, central_position=2)
    with pytest.raises(_lib.MfaHipError, match="not a phone"):
        tree_statistics_host(ok.feats, ok.frame_off, ok.ali, ok.tm, [R.N_PHONES + 1])
    with pytest.raises(_lib.MfaHipError, match="frames"):
        tree_statistics_host(ok.feats[:-1], ok.frame_off, ok.ali, ok.tm, ok.ci)


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "tree_acc_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "tree_acc_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "tree_acc_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout


# ---- questions and the tree on planted statistics --------------------------------------------------------------------------------
DIM = 3
A_SET = [3, 4]                                   # the planted dependence: the centre's mean shifts when the left phone is in A
FAMILIES = [[3, 4, 5], [6, 7], [8, 9]]


def planted_stats(shift=4.0, n=20, with_ci=True, family_spread=0.05):
    """Events of every window over phones 3..9 (and the context-independent 1, 2 with no context), all pdf-classes of the
    centre's entry; unit variance, a mean that depends on the centre's family, a little on the phone and the pdf-class, and by
    ``shift`` on whether the left phone is in A."""
    rng = np.random.default_rng(12)
    topo = R.topology()
    fam_mean = {p: 10.0 * (f + 1) * np.ones(DIM) for f, fam in enumerate(FAMILIES) for p in fam}
    rows = []
    for c in range(3, 10):
        classes = sorted({st.forward_pdf_class for st in topo.entry_for_phone(c) if st.transitions})
        for l in [0] + list(range(1, 10)):
            for r in [0] + list(range(1, 10)):
                for pc in classes:
                    m = fam_mean[c] + family_spread * c + 0.5 * pc + (shift if l in A_SET else 0.0) + 0.01 * rng.normal(size=DIM)
                    rows.append((tree_key(l, c, r, pc), n, n * m, n * (1.0 + m * m)))
    if with_ci:
        for c in (1, 2):
            for pc in (0, 1, 2):
                m = -5.0 * c + pc + np.zeros(DIM)
                rows.append((tree_key(0, c, 0, pc), 50, 50 * m, 50 * (1.0 + m * m)))
    rows.sort(key=lambda r: int(r[0]))
    return TreeStats(np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.int64),
                     np.array([r[2] for r in rows]), np.array([r[3] for r in rows]))


def default_roots():
    return [([1], False, False), ([2], False, False)] + [([p], True, True) for p in range(3, 10)]


QUESTIONS = [[5, 6, 7], A_SET, [8, 9], [3, 4, 5, 6], [1, 2]]


def test_loglike_formula():
    x = np.random.default_rng(0).normal(2.0, 3.0, size=(500, 4))
    n, s, q = 500, x.sum(axis=0), (x * x).sum(axis=0)
    var = x.var(axis=0)
    direct = np.sum(-0.5 * np.log(2 * np.pi * var) - 0.5 * (x - x.mean(axis=0)) ** 2 / var)
    assert abs(tree.loglike(n, s, q) - direct) < 1e-9 * abs(direct)
    assert tree.loglike(0, np.zeros(4), np.zeros(4)) == 0.0
    # the floor: a constant column has variance 0.01
    assert np.isclose(tree.loglike(10, np.full(1, 30.0), np.full(1, 90.0)), -5 * (np.log(2 * np.pi) + 1 + np.log(0.01)))


def test_automatic_questions_returns_the_planted_families():
    st = planted_stats(shift=0.0)
    sets = [[p] for p in range(3, 10)] + [[1], [2]]
    qs = tree.automatic_questions(st, sets, pdf_classes=(0,))
    assert qs[: len(sets)] == sets                                 # every input set, in order
    for fam in FAMILIES:
        assert fam in qs, (fam, qs)
    assert [1, 2] in qs and len(qs) == len(sets) + len(sets) - 2   # a binary tree's inner nodes, without the root
    assert all(q == sorted(q) for q in qs) and len({tuple(q) for q in qs}) == len(qs)
    assert sorted(p for s in sets for p in s) not in qs            # the root is no question
    assert tree.automatic_questions(st, sets, pdf_classes=(0,)) == qs
    # the phones of the one-state entry (3, 6, 9) have no pdf-class 1: a pair with a set without data merges first, at loss
    # 0, and of those pairs the one of the lowest indices: 3 with 4, then 6 and 9 onto that cluster
    qs1 = tree.automatic_questions(st, sets, pdf_classes=(1,))
    assert qs1[len(sets): len(sets) + 3] == [[3, 4], [3, 4, 6], [3, 4, 6, 9]]
    assert [1, 2] in qs1


def test_build_tree_picks_the_planted_question_first():
    st = planted_stats()
    topo = R.topology()
    t, rec = tree.build_tree(topo, QUESTIONS, st, default_roots(), max_leaves=1000)
    W = st.windows()
    initial = [np.flatnonzero((W[:, 1] == c) & (st.pdf_classes() == pc)) for c in (1, 2) for pc in (0, 1, 2)]
    initial += [np.flatnonzero(W[:, 1] == c) for c in range(3, 10)]
    class_q = [[0], [0, 1]]
    gain, leaf, key, question = R.best_split(st, initial[6:], {0: QUESTIONS, 1: QUESTIONS, 2: QUESTIONS, -1: class_q})
    first = rec["splits"][0]
    assert (first["key"], first["question"]) == (0, A_SET) == (key, question)
    assert first["root"] == 2 + leaf
    assert abs(first["gain"] - gain) <= 1e-9 * abs(gain)
    gains = [s["gain"] for s in rec["splits"]]
    # The order of the gains.  "Non-increasing" outright is no theorem of greedy splitting — a child's best gain may exceed its
    # parent's, and among the splits of the 0.01 noise on the planted means it does.  What greedy splitting guarantees, and what
    # is asserted for every split: a leaf that was open while other splits were made was passed over for them, so none of
    # those gained less than it did when its turn came.  Over the initial leaves that is "non-increasing".
    born = {c: i for i, sp in enumerate(rec["splits"]) for c in sp["children"]}
    for j, sp in enumerate(rec["splits"]):
        assert all(rec["splits"][i]["gain"] >= sp["gain"] for i in range(born.get(sp["node"], -1) + 1, j)), j
    assert rec["initial_leaves"] == 6 + 7 and all(sp["node"] >= 6 for sp in rec["splits"])
    of_initial = [sp["gain"] for sp in rec["splits"] if sp["node"] < rec["initial_leaves"]]
    assert len(of_initial) == 7 and all(x >= y for x, y in zip(of_initial, of_initial[1:]))
    assert all(g > 0 for g in gains)
    assert np.isclose(rec["total_gain"], sum(gains), rtol=1e-12)
    # every event maps to a leaf, and the pdfs are 0..n-1 in order of first appearance
    leaves = tree.event_leaves(t, st)
    assert leaves.min() == 0 and leaves.max() == rec["leaves"] - 1
    walk = t.to_pdf.leaves()
    firsts = list(dict.fromkeys(walk))
    assert firsts == list(range(rec["leaves"]))
    # the not-split roots stay whole: one leaf per pdf-class, pdfs 0..5
    for c, base in ((1, 0), (2, 3)):
        assert [t.compute([0, c, 0], pc) for pc in (0, 1, 2)] == [base, base + 1, base + 2]
    # the shared roots split on the pdf-class too
    assert any(s["key"] == -1 for s in rec["splits"])
    # the planted shift is resolved: windows that differ only in "left in A" get different pdfs
    assert t.compute([3, 5, 6], 1) != t.compute([5, 5, 6], 1)
    assert t.compute([3, 5, 6], 1) == t.compute([4, 5, 6], 1)


def test_greedy_order_and_max_leaves():
    st = planted_stats()
    topo = R.topology()
    roots = default_roots()
    initial_leaves = 6 + 7
    for cap in (initial_leaves, initial_leaves + 1, initial_leaves + 5, 40):
        t, rec = tree.build_tree(topo, QUESTIONS, st, roots, max_leaves=cap, cluster_thresh=0.0)
        assert len(rec["splits"]) == cap - initial_leaves            # (the planted statistics have hundreds of positive gains)
        assert rec["leaves"] == initial_leaves + len(rec["splits"]) - len(rec["merges"]) <= cap
        assert rec["leaves"] == len(set(t.to_pdf.leaves()))
    # the greedy order: every split is the best of the leaves at hand, so the prefix of a longer run is the shorter run
    _t, a = tree.build_tree(topo, QUESTIONS, st, roots, max_leaves=initial_leaves + 5, cluster_thresh=0.0)
    _t, b = tree.build_tree(topo, QUESTIONS, st, roots, max_leaves=40, cluster_thresh=0.0)
    assert b["splits"][:5] == a["splits"]
    # gains do not increase as long as the split leaves are the initial ones (a child's gain is not bounded by its parent's)
    top = [s["gain"] for s in b["splits"][:7]]
    assert all(x >= y for x, y in zip(top, top[1:]))


def test_cluster_threshold_collapses_every_root():
    st = planted_stats()
    topo = R.topology()
    t, rec = tree.build_tree(topo, QUESTIONS, st, default_roots(), max_leaves=60, cluster_thresh=1e30)
    assert len(rec["splits"]) > 0 and rec["leaves"] == 6 + 7
    assert len(rec["merges"]) == len(rec["splits"])
    for c in range(3, 10):
        pdfs = {t.compute([l, c, r], pc) for l in range(10) for r in range(10) for pc in ((0,) if c in R.ONE_STATE else (0, 1, 2))}
        assert len(pdfs) == 1
    # the default threshold, the smallest gain of a split made, merges nothing that a split of that gain separated
    _t, rec2 = tree.build_tree(topo, QUESTIONS, st, default_roots(), max_leaves=60)
    assert rec2["leaves"] > 6 + 7 and all(m["loss"] < min(s["gain"] for s in rec2["splits"]) for m in rec2["merges"])


def test_tree_round_trip_and_init_model():
    st = planted_stats()
    topo = R.topology()
    t, rec = tree.build_tree(topo, QUESTIONS, st, default_roots(), max_leaves=45)
    buf = io.BytesIO()
    kaldi_io.write_tree(buf, t)
    back = kaldi_io.read_tree(buf.getvalue())
    assert back == t and (back.context_width, back.central_position) == (3, 1)
    raw_tm, raw_am = tree.init_model(topo, t, st)
    assert raw_am.num_pdfs == rec["leaves"] and raw_am.dim == DIM
    assert [tuple(int(v) for v in r) for r in raw_tm.tuples] == R.transition_tuples(topo, t)
    tm = TransitionModel(raw_tm)                                    # as many log-probabilities as transition-ids
    assert tm.num_pdfs == rec["leaves"]
    assert np.allclose(np.exp(tm.log_probs[1:3]), [0.75, 0.25])
    # a leaf's Gaussian is its pooled events' mean and variance
    leaves = tree.event_leaves(t, st)
    p = int(leaves[5])
    m = leaves == p
    mean = st.sum[m].sum(axis=0) / st.count[m].sum()
    var = np.maximum(st.sumsq[m].sum(axis=0) / st.count[m].sum() - mean * mean, 0.01)
    assert np.allclose(raw_am.means_invvars[p][0] / raw_am.inv_vars[p][0], mean, rtol=1e-5)
    assert np.allclose(1.0 / raw_am.inv_vars[p][0], var, rtol=1e-5)
    # a leaf without data takes the global mean and variance
    no_ci = planted_stats(with_ci=False)
    _tm2, am2 = tree.init_model(topo, t, no_ci)
    g = no_ci.sum.sum(axis=0) / no_ci.count.sum()
    assert np.allclose(am2.means_invvars[0][0] / am2.inv_vars[0][0], g, rtol=1e-5)


def test_conversion_of_alignments():
    rng = np.random.default_rng(21)
    case = R.make_case(rng, [120, 64, 65, 200, 31], DIM, integer=False)
    case.ali[case.frame_off[2] + 3] = 0                             # one utterance is skipped
    st, fe, skipped = host(case)
    assert skipped == 1
    topo = case.tm.topo
    qs = tree.automatic_questions(st, [[p] for p in range(1, 10)], pdf_classes=(0,))
    t, rec = tree.build_tree(topo, qs, st, default_roots(), max_leaves=40)
    raw_tm, _am = tree.init_model(topo, t, st)
    new_tm = TransitionModel(raw_tm)
    table = tree.convert_table(case.tm, new_tm, t, st)
    local = tree.local_of_tid(case.tm)
    new_ali = tree.convert_alignments(table, local, fe, case.ali)
    a, b = case.frame_off[2], case.frame_off[3]
    assert np.all(new_ali[a:b] == 0) and np.all(np.delete(new_ali, np.r_[a:b]) > 0)
    ok = new_ali > 0
    old, new = case.ali[ok], new_ali[ok]
    assert np.array_equal(case.tm.id2phone[old], new_tm.id2phone[new])
    assert np.array_equal(case.tm.tuples[case.tm.id2state[old] - 1, 1], new_tm.tuples[new_tm.id2state[new] - 1, 1])
    assert np.array_equal(case.tm.is_self_loop[old], new_tm.is_self_loop[new])
    assert np.array_equal(case.tm.is_final[old], new_tm.is_final[new])
    assert np.array_equal(local[old], tree.local_of_tid(new_tm)[new])
    assert np.array_equal(new_tm.id2pdf[new], tree.event_leaves(t, st)[fe[ok]])
    # the pdfs are the tree's for the windows the restatement finds
    keys, *_rest, rfe, _sk = R.accumulate(case)
    W = st.windows()
    for tt in np.flatnonzero(ok)[::17]:
        e = fe[tt]
        assert new_tm.id2pdf[new_ali[tt]] == t.compute([int(v) for v in W[e]], int(st.pdf_classes()[e]))


def test_tree_refusals():
    st = planted_stats()
    topo = R.topology()
    uneven = R.topology()
    uneven.entries[0][1] = kaldi_io.HmmState(1, 2, uneven.entries[0][1].transitions)
    t, _rec = tree.build_tree(topo, QUESTIONS, st, default_roots(), max_leaves=20)
    with pytest.raises(ValueError, match="forward pdf-class 1 and self-loop pdf-class 2"):
        tree.init_model(uneven, t, st)
    with pytest.raises(ValueError, match="repeats a phone"):
        tree.build_tree(topo, QUESTIONS, st, [([3], True, True), ([3, 4], True, True)])
    with pytest.raises(ValueError, match="empty phone set"):
        tree.automatic_questions(st, [[3], []])
    other = TransitionModel(tree.init_model(R.topology(one_state=(3,)), t, st)[0])
    mine = TransitionModel(tree.init_model(topo, t, st)[0])
    with pytest.raises(ValueError, match="differ in their topology"):
        tree.convert_table(other, mine, t, st)
    mono = kaldi_io.ContextDependency(1, 0, t.to_pdf)
    with pytest.raises(ValueError, match="only 3, 1"):
        tree.event_leaves(mono, st)


# ---- the trainer on the host backend -------------------------------------------------------------------------------------------
def fst_accepts(fst, tids) -> bool:
    """The input labels of some path from the start state to a final one spell ``tids`` (epsilon input arcs are free)."""
    off, arcs = fst.arc_offsets, fst.arcs

    def closure(states):
        todo, seen = list(states), set(states)
        while todo:
            s = todo.pop()
            for a in arcs[off[s]: off[s + 1]]:
                if a["ilabel"] == 0 and int(a["nextstate"]) not in seen:
                    seen.add(int(a["nextstate"]))
                    todo.append(int(a["nextstate"]))
        return seen

    cur = closure({int(fst.start)})
    for t in tids:
        nxt = {int(a["nextstate"]) for s in cur for a in arcs[off[s]: off[s + 1]] if a["ilabel"] == int(t)}
        if not nxt:
            return False
        cur = closure(nxt)
    return any(np.isfinite(fst.final[s]) for s in cur)


def tree_host_backend(corpus):
    from montreal_forced_aligner_amd.model import TransitionModel as TM
    from tests import train_mono_case as TC

    class TreeHostBackend(TC.HostBackend):
        """``TriphoneTrainer``'s five calls on the host twins."""

        def tree_accumulate(self, raw_tm, ci_phones):
            st, fe, skipped = tree_statistics_host(self.all_feats, self.frame_off, np.concatenate(self.ali), TM(raw_tm), ci_phones)
            self.tree_batch = (st, fe)
            return st, skipped

        def convert_alignments(self, old_raw_tm, raw_tm, raw_am, new_tree):
            st, fe = self.tree_batch
            old_tm, new_tm = TM(old_raw_tm), TM(raw_tm)
            self.old_ali = list(self.ali)
            new = tree.convert_alignments(tree.convert_table(old_tm, new_tm, new_tree, st), tree.local_of_tid(old_tm), fe,
                                          np.concatenate(self.ali))
            self.ali = [new[self.frame_off[k]: self.frame_off[k + 1]] for k in range(len(self.ali))]
            self.converted = list(self.ali)

    return TreeHostBackend(corpus)


NUM_LEAVES = 300


@pytest.fixture(scope="module")
def tri_run():
    from montreal_forced_aligner_amd.train import MonophoneTrainer, TriphoneTrainer
    from tests import train_mono_case as TC

    corpus = TC.train_corpus()
    mono_backend = TC.HostBackend(corpus)
    mono = MonophoneTrainer(lexicon=corpus.world.lexicon, topology=TC.topology(), backend=mono_backend,
                            silence_phones=TC.silence_ids(), num_iterations=6, max_gaussians=208)
    mono_backend.equal_align(mono.raw_tm, mono.raw_am, mono.tree, mono.seed)
    equal_share = TC.phone_share(corpus, mono.raw_tm, mono_backend.alignments())
    mono.train()
    mono_share = TC.phone_share(corpus, mono.raw_tm, TC.host_align(corpus, mono.raw_tm, mono.raw_am, mono.tree, mono.opt))
    backend = tree_host_backend(corpus)
    tr = TriphoneTrainer(lexicon=corpus.world.lexicon, previous=mono, backend=backend, silence_phones=TC.silence_ids(),
                         num_iterations=11, num_leaves=NUM_LEAVES, max_gaussians=NUM_LEAVES + 60).train()
    return corpus, mono, tr, backend, equal_share, mono_share


def check_triphone_training(corpus, mono, tr, final_alignments, equal_share, mono_share):
    """What the host and the device runs of the 11-iteration stage are both held to."""
    from tests import train_mono_case as TC

    h = tr.history
    assert [e["iteration"] for e in h] == list(range(12))
    assert tr.realignment_iterations == [10] and tr.final_gaussian_iteration == 1
    assert [e["realigned"] for e in h] == [i in (0, 10) for i in range(12)]
    checked, bad = TC.em_violations(h)
    print("checked", checked, [(e["iteration"], round(e["loglike"], 4)) for e in h])
    assert len(checked) >= 6 and bad == []
    first = h[0]
    assert set(first) >= {"events", "leaves", "tree_gain_per_frame", "skipped", "questions"}
    print({k: first[k] for k in ("events", "leaves", "tree_gain_per_frame", "skipped", "questions")})
    assert first["skipped"] == first["failed"] <= 2            # an utterance the previous model could not align is all zeros
    assert mono.raw_am.num_pdfs == 208 < first["leaves"] <= NUM_LEAVES
    assert tr.raw_am.num_pdfs == first["leaves"] == tr.initial_gaussians == len(set(tr.tree.to_pdf.leaves()))
    assert first["tree_gain_per_frame"] > 0 and tr.tree_record["total_gain"] > 0
    assert first["events"] == tr.tree_stats.num_events > first["leaves"]
    assert (tr.tree.context_width, tr.tree.central_position) == (3, 1)
    assert tr.num_gaussians <= tr.max_gaussians
    share = TC.phone_share(corpus, tr.raw_tm, final_alignments)
    print(f"frames on the generator's phone: equal alignments {equal_share:.4f}, monophone (6 iterations) {mono_share:.4f}, "
          f"triphone stage (11 iterations, {first['leaves']} leaves) {share:.4f}")
    return share


def test_triphone_trainer_on_the_host_backend(tri_run):
    """Measured here (48 utterances, 14 400 frames, one of them not aligned by the 6-iteration monophone model and so skipped):
    3 404 events, 134 questions, 250 leaves after clustering (``num_leaves`` 300; the monophone has 208 pdfs), tree gain 10.29
    per frame.  Share of frames on the generator's phone: equal alignments 0.1625, monophone (6 iterations) 0.6294, triphone
    stage (11 iterations) 0.7169.

    The margin: tests/test_train_mono_cpu.py allows no spread between runs — it compares one run with the equal alignments —,
    so there is none to borrow and the margin is zero: the triphone's share must not fall below the monophone's."""
    from tests import train_mono_case as TC

    corpus, mono, tr, backend, equal_share, mono_share = tri_run
    final = TC.host_align(corpus, tr.raw_tm, tr.raw_am, tr.tree, tr.opt)
    share = check_triphone_training(corpus, mono, tr, final, equal_share, mono_share)
    assert share >= mono_share > equal_share


def test_triphone_conversion_follows_the_graphs(tri_run):
    from montreal_forced_aligner_amd import graph as G
    from tests import train_mono_case as TC

    corpus, mono, tr, backend, _e, _m = tri_run
    old_tm = TransitionModel(mono.raw_tm)
    new_tm = TransitionModel(tree.init_model(mono.raw_tm.topo, tr.tree, tr.tree_stats)[0])
    gc = G.TrainingGraphCompiler(new_tm, tr.tree, corpus.world.lexicon)
    leaves = tree.event_leaves(tr.tree, tr.tree_stats)
    st, fe = backend.tree_batch
    for k in (0, 7, 23, 47):
        old, new = backend.old_ali[k], backend.converted[k]
        assert np.all(old > 0) and np.all(new > 0)
        assert np.array_equal(old_tm.id2phone[old], new_tm.id2phone[new])
        assert np.array_equal(old_tm.tuples[old_tm.id2state[old] - 1, 1], new_tm.tuples[new_tm.id2state[new] - 1, 1])
        assert np.array_equal(old_tm.is_self_loop[old], new_tm.is_self_loop[new])
        assert np.array_equal(new_tm.id2pdf[new], leaves[fe[backend.frame_off[k]: backend.frame_off[k + 1]]])
        assert fst_accepts(gc.compile_fst(corpus.text[k]), new)
        assert not fst_accepts(gc.compile_fst(corpus.text[k]), new[:-1])


def test_triphone_trainer_options_and_files(tri_run, tmp_path):
    from montreal_forced_aligner_amd.train import LdaTrainer, TriphoneTrainer, default_roots
    from tests import train_mono_case as TC

    corpus, mono, tr, backend, _e, _m = tri_run
    full = TriphoneTrainer(lexicon=corpus.world.lexicon, previous=(mono.raw_tm, mono.raw_am, mono.tree), backend=backend)
    assert (full.num_iterations, full.num_leaves, full.max_gaussians, full.cluster_threshold, full.power) == (35, 1000, 10000, -1.0, 0.25)
    assert full.opt.boost_silence == 1.25 and full.realignment_iterations == [10, 20, 30] and full.final_gaussian_iteration == 25
    roots = default_roots(mono.raw_tm.topo, None, TC.silence_ids())
    sil = set(TC.silence_ids())
    assert all((shared, split) == ((False, False) if set(ph) & sil else (True, True)) for ph, shared, split in roots)
    assert sorted(p for ph, _a, _b in roots for p in ph) == sorted(int(p) for p in mono.raw_tm.topo.phones)
    with pytest.raises(ValueError, match="previous"):
        TriphoneTrainer(lexicon=corpus.world.lexicon, backend=backend)
    with pytest.raises(ValueError, match="only 3 and 1"):
        TriphoneTrainer(lexicon=corpus.world.lexicon, previous=mono, backend=backend, context_width=5, central_position=2)
    paths = tr.write(tmp_path / "tri")
    assert [p.name for p in paths] == ["final.mdl", "tree"]
    assert kaldi_io.read_tree(paths[1].read_bytes()) == tr.tree
    raw_tm, raw_am = kaldi_io.read_model(paths[0].read_bytes())
    assert raw_am.num_pdfs == tr.raw_am.num_pdfs and np.array_equal(raw_tm.tuples, tr.raw_tm.tuples)
    # the default leaves the LDA stage as it is
    assert LdaTrainer(lexicon=corpus.world.lexicon, previous=tr, backend=lda_host_backend(corpus)).num_leaves is None


def lda_host_backend(corpus):
    from tests import lda_case

    return lda_case.LdaHostBackend(corpus)


# ---- the kalpy layer's host half -------------------------------------------------------------------------------------------------
def test_kalpy_names_on_the_host(tmp_path):
    from montreal_forced_aligner_amd import kalpy_api as KA

    case = R.make_case(np.random.default_rng(33), [150, 64, 90, 129], DIM, integer=False)
    st, _fe, _sk = host(case)
    topo = case.tm.topo
    qs = KA.automatically_obtain_questions(st, [[p] for p in range(1, 10)], [0], 1)
    assert qs == tree.automatic_questions(st, [[p] for p in range(1, 10)], (0,), 1)
    roots = tmp_path / "roots.int"
    roots.write_text("not-shared not-split 1\nnot-shared not-split 2\n" + "".join(f"shared split {p}\n" for p in range(3, 10)))
    assert KA.read_roots(roots) == default_roots()
    record = KA.build_tree(topo, qs, st, str(roots), str(tmp_path / "tree"), max_leaves=30, cluster_thresh=-1)
    t = KA.read_tree(tmp_path / "tree")
    want, _rec = tree.build_tree(topo, qs, st, default_roots(), max_leaves=30)
    assert t == want and record["leaves"] == len(set(t.to_pdf.leaves())) <= 30
    KA.gmm_init_model(topo, t, st, str(tmp_path / "1.mdl"))
    new_tm, new_am = KA.read_gmm_model(tmp_path / "1.mdl")
    assert new_am.num_pdfs == record["leaves"] == new_am.num_gauss
    KA.gmm_init_model(topo, t, st, str(tmp_path / "2.mdl"), mixup=record["leaves"] + 5)
    assert record["leaves"] < KA.read_gmm_model(tmp_path / "2.mdl")[1].num_gauss <= record["leaves"] + 5   # (small leaves are not split)
    with pytest.raises(NotImplementedError):
        KA.gmm_init_model(topo, t, st, str(tmp_path / "3.mdl"), mixdown=10)
    with pytest.raises(NotImplementedError):
        KA.gmm_init_model_from_previous(topo, t, st)
    fo = case.frame_off
    old = case.ali[fo[1]: fo[2]]
    new = np.asarray(KA.convert_alignments(case.tm, new_tm, t, old.tolist()))
    assert np.array_equal(case.tm.id2phone[old], new_tm.id2phone[new]) and np.array_equal(case.tm.is_self_loop[old], new_tm.is_self_loop[new])
    _k, _c, _s, _q, rfe, _sk2 = R.accumulate(R.Case(case.tm, case.feats[fo[1]: fo[2]], np.array([0, len(old)]), old, ()))
    keys = R.accumulate(R.Case(case.tm, case.feats[fo[1]: fo[2]], np.array([0, len(old)]), old, ()))[0]
    for tt in range(0, len(old), 7):                               # the pdfs of the windows the alignment spells
        k = int(keys[rfe[tt]])
        assert new_tm.id2pdf[new[tt]] == t.compute([k >> 48, (k >> 28) & 0xFFFFF, (k >> 8) & 0xFFFFF], k & 0xFF)
    with pytest.raises(ValueError, match="does not split into phones"):
        KA.convert_alignments(case.tm, new_tm, t, old[:-1].tolist() + [int(R.phone_path(case.tm, 4, [1, 1, 1])[0])])
    with pytest.raises(ValueError, match="only 3 and 1"):
        KA.TreeStatsAccumulator.__init__(object.__new__(KA.TreeStatsAccumulator), "x", context_width=2, central_position=1)
