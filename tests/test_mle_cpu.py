"""The host half of training (montreal_forced_aligner_amd/mle.py and kaldi_io.write_tree): the Gaussian update against a
brute-force float64 restatement written here, the split targets, mixing up, the flat-start model and the tree writer.

Tolerances.  A re-estimated mean is one float64 division rounded to float32: the restatement rounds the same way, so means
and inverse variances are compared bit for bit; means_invvars is one float32 product of the two, bit for bit as well.  Weights:
occ_i / Σocc in float64, renormalised and rounded to float32 — the restatement sums in another order, so 1 float32 ulp; a
pdf's float32 weights sum to 1 within n·2⁻²⁴ (n roundings of at most half an ulp of a value at most 1) plus the float64
summation of the check itself."""
import io

import numpy as np
import pytest

import synth_workload as SW
from montreal_forced_aligner_amd import adapt as A
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.engine import GmmStats
from tests import helpers
from tests.test_map_adapt_cpu import _raw

SIZES = [1, 2, 32, 128, 3, 4, 2, 1]
# pdf 4 (3 Gaussians): occupancies just below / above min_gaussian_occupancy; pdf 5 (4 Gaussians): shares just below / above
# min_gaussian_weight; pdf 6 (2 Gaussians): both below the occupancy threshold (one survives); pdf 7: no statistics


def _case(dim, seed=0):
    rng = np.random.default_rng(100 + dim + seed)
    raw, _par = _raw(rng, dim, SIZES)
    # gconsts as adapt.gconsts makes them, so that a model kept "as it is" and one recomputed agree to the bit
    raw.gconsts = [A.gconsts(w, mi, iv) for w, mi, iv in zip(raw.weights, raw.means_invvars, raw.inv_vars)]
    offs = A.pdf_offsets(raw)
    G = int(offs[-1])
    st = GmmStats.zeros(G, dim, 1)
    st.occ[:] = rng.uniform(15.0, 400.0, size=G)
    a = int(offs[4]); st.occ[a: a + 3] = [10.0, np.nextafter(10.0, 11.0), 200.0]
    a = int(offs[5]); big = 4.0e6
    st.occ[a: a + 4] = [big, big * 1.0e-5 * 0.999, big * 1.0e-5 * 1.5, 50.0]
    a = int(offs[6]); st.occ[a: a + 2] = [2.0, 9.5]
    a = int(offs[7]); st.occ[a] = 0.0
    mean = rng.normal(0, 3, size=(G, dim))
    var = rng.uniform(0.3, 3.0, size=(G, dim))
    var[int(offs[2]) + 5, 3] = 1.0e-5                       # must be floored
    var[int(offs[3]) + 100, 0] = 0.0
    st.mean_acc[:] = st.occ[:, None] * mean
    st.var_acc[:] = st.occ[:, None] * (var + mean * mean)
    return raw, st, offs


def brute_force(raw, st, flags, min_occ, min_w, min_var, remove):
    """MleDiagGmmUpdate one Gaussian at a time, in float64 Python."""
    out, g, floored = [], 0, 0
    for p in range(raw.num_pdfs):
        n = raw.weights[p].shape[0]
        occ_sum = sum(float(st.occ[g + i]) for i in range(n))
        if not occ_sum > 0:
            out.append(None)
            g += n
            continue
        rows, marked = [], 0
        for i in range(n):
            occ = float(st.occ[g + i])
            iv, mi, w = raw.inv_vars[p][i].copy(), raw.means_invvars[p][i].copy(), float(raw.weights[p][i])
            if occ > min_occ and occ / occ_sum > min_w:
                mu_old = mi / iv
                m = st.mean_acc[g + i] / occ
                mu = m.astype(np.float32) if "m" in flags else mu_old
                if "v" in flags:
                    if "m" in flags:
                        v = st.var_acc[g + i] / occ - m * m
                    else:
                        v = st.var_acc[g + i] / occ - 2.0 * mu_old.astype(np.float64) * m + mu_old.astype(np.float64) ** 2
                    floored += int((v < min_var).sum())
                    iv = (1.0 / np.maximum(v, min_var)).astype(np.float32)
                if "w" in flags:
                    w = occ / occ_sum
                rows.append((w, mu * iv, iv, True))
            elif remove and marked < n - 1:
                marked += 1
            else:
                rows.append((w, mi, iv, False))
        total = sum(r[0] for r in rows)
        renorm = "w" in flags or len(rows) < n
        out.append([(r[0] / total if renorm else r[0], r[1], r[2], r[3]) for r in rows])
        g += n
    return out, floored


@pytest.mark.parametrize("dim", (13, 40, 48))
@pytest.mark.parametrize("flags,remove", (("mvw", True), ("mvw", False), ("mv", True), ("vw", True), ("w", False)))
def test_mle_update_against_brute_force(dim, flags, remove):
    raw, st, offs = _case(dim)
    new, updated, removed, floored = mle.mle_update(raw, st, flags=flags, remove_low_count_gaussians=remove)
    want, want_floored = brute_force(raw, st, flags, 10.0, 1.0e-5, 1.0e-3, remove)
    assert new.num_pdfs == raw.num_pdfs and new.dim == dim
    n_up = n_rm = 0
    for p in range(raw.num_pdfs):
        if want[p] is None:                                  # no statistics: unchanged bits
            for a, b in ((new.gconsts, raw.gconsts), (new.weights, raw.weights), (new.means_invvars, raw.means_invvars),
                         (new.inv_vars, raw.inv_vars)):
                assert a[p].tobytes() == b[p].tobytes()
            continue
        rows = want[p]
        assert new.weights[p].shape[0] == len(rows), p
        n_rm += SIZES[p] - len(rows)
        n_up += sum(r[3] for r in rows)
        w = np.array([r[0] for r in rows])
        assert np.all(np.abs(new.weights[p].astype(np.float64) - w) <= np.spacing(w.astype(np.float32))), p
        assert np.array_equal(new.inv_vars[p], np.stack([r[2] for r in rows])), p
        assert np.array_equal(new.means_invvars[p], np.stack([r[1] for r in rows])), p
        assert np.array_equal(new.gconsts[p], A.gconsts(new.weights[p], new.means_invvars[p], new.inv_vars[p]))
        assert abs(float(new.weights[p].astype(np.float64).sum()) - 1.0) <= (len(rows) + 2) * 2.0 ** -24, p
        assert new.weights[p].dtype == new.inv_vars[p].dtype == new.means_invvars[p].dtype == new.gconsts[p].dtype == np.float32
    assert (updated, removed) == (n_up, n_rm)
    assert floored == want_floored
    if "v" not in flags:
        assert floored == 0
    elif "m" in flags:                                       # the two elements the case plants below the floor
        assert floored == 2
    if remove:                                               # the thresholds from both sides, and the survivor
        assert new.weights[4].shape[0] == 2 and new.weights[5].shape[0] == 3 and new.weights[6].shape[0] == 1
        # of two Gaussians below the threshold the first is removed, the last stays as it was
        assert new.inv_vars[6].tobytes() == raw.inv_vars[6][1:].tobytes() and new.weights[6][0] == 1.0
    else:
        assert [w.shape[0] for w in new.weights] == SIZES


def test_floored_variance_is_the_floor():
    raw, st, offs = _case(13)
    new, _u, _r, floored = mle.mle_update(raw, st, min_variance=0.5)
    assert floored > 2
    for p in range(raw.num_pdfs - 1):
        assert float(new.inv_vars[p].max()) <= 2.0 or p in (4, 5, 6)       # (kept Gaussians keep their own variances)
    assert new.inv_vars[2][5, 3] == np.float32(2.0) and new.inv_vars[3][100, 0] == np.float32(2.0)


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_means_only_is_map_update_bit_for_bit(dim):
    raw, st, _offs = _case(dim, seed=1)
    new, updated, removed, floored = mle.mle_update(raw, st, flags="m", remove_low_count_gaussians=False)
    ref, ref_updated, ref_kept = A.map_update(raw, st)
    assert (updated, removed, floored) == (ref_updated, 0, 0) and ref_kept == sum(SIZES) - updated
    for p in range(raw.num_pdfs):
        for a, b in ((new.gconsts, ref.gconsts), (new.weights, ref.weights), (new.means_invvars, ref.means_invvars),
                     (new.inv_vars, ref.inv_vars)):
            assert a[p].tobytes() == b[p].tobytes(), p


def test_bad_statistics_and_flags_are_refused():
    raw, st, offs = _case(13)
    st.mean_acc[int(offs[1])] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        mle.mle_update(raw, st)
    with pytest.raises(ValueError, match="flags"):
        mle.mle_update(raw, st, flags="mx")
    with pytest.raises(ValueError, match="statistics of shape"):
        mle.mle_update(raw, GmmStats.zeros(3, 13, 1))


# ---- split targets -----------------------------------------------------------------------------------------------------------
def test_split_targets_reach_the_total_or_retire_everything():
    rng = np.random.default_rng(7)
    occ = np.concatenate([rng.uniform(0, 5000, size=40), [0.0, 19.0, 41.0]])
    n0 = np.ones(len(occ), dtype=np.int64)
    prev = n0
    for target in (len(occ), len(occ) + 1, 100, 400, 2000, 100000):
        n = mle.split_targets(occ, n0, target, power=0.25, min_count=20.0)
        assert np.all(n >= prev)                              # monotone in the total
        retired = (n + 1) * 20.0 >= occ
        assert int(n.sum()) == max(target, len(occ)) or retired.all()
        grown = n > 1
        assert np.all(n[grown] * 20.0 < occ[grown])           # no pdf beyond occ / min_count
        prev = n
    assert int(mle.split_targets(occ, n0, 100000).sum()) < 100000
    assert mle.split_targets(occ, n0, 10).tolist() == n0.tolist()     # a total already passed: nothing is taken away
    # equal priorities: the lower index first
    assert mle.split_targets([100.0, 100.0, 100.0], [1, 1, 1], 5).tolist() == [2, 2, 1]
    # the queue is on occ^power / components
    assert mle.split_targets([1.0e4, 1.0e2], [1, 1], 4, power=1.0).tolist() == [3, 1]
    assert mle.split_targets([1.0e4, 1.0e2], [1, 1], 5, power=0.0).tolist() == [3, 2]


# ---- mixing up ----------------------------------------------------------------------------------------------------------------
def test_mix_up_counts_weights_symmetry_and_seed():
    raw, _par = _raw(np.random.default_rng(11), 13, [1, 1, 3, 1])
    occ = np.array([1000.0, 30.0, 500.0, 90.0])
    new, targets = mle.mix_up(raw, occ, 9, rng=np.random.default_rng(5))
    want = mle.split_targets(occ, [1, 1, 3, 1], 9)
    assert targets.tolist() == want.tolist() == [w.shape[0] for w in new.weights] and int(targets.sum()) == 9
    assert targets[1] == 1 and new.means_invvars[1].tobytes() == raw.means_invvars[1].tobytes()
    for p in range(4):
        assert abs(float(new.weights[p].astype(np.float64).sum()) - float(raw.weights[p].astype(np.float64).sum())) <= 2.0 ** -22
        assert np.array_equal(new.gconsts[p], A.gconsts(new.weights[p], new.means_invvars[p], new.inv_vars[p])) or targets[p] == 1
    # pdf 3: one Gaussian split once — the pair sits symmetrically about the parent's mean, at perturb_factor deviations scale
    if targets[3] == 2:
        mu0 = raw.means_invvars[3][0].astype(np.float64) / raw.inv_vars[3][0]
        mu = new.means_invvars[3].astype(np.float64) / new.inv_vars[3]
        sd = np.sqrt(1.0 / raw.inv_vars[3][0].astype(np.float64))
        assert np.all(np.abs(0.5 * (mu[0] + mu[1]) - mu0) <= 4 * 2.0 ** -24 * (np.abs(mu0) + sd))
        z = (mu[1] - mu[0]) / (2 * 0.01 * sd)
        assert 0.3 < float(np.abs(z).mean()) < 2.0
        assert new.inv_vars[3][0].tobytes() == new.inv_vars[3][1].tobytes() == raw.inv_vars[3][0].tobytes()
        assert new.weights[3].tolist() == [0.5, 0.5]
    # pdf 0: split repeatedly, always the component of largest weight, the first on ties
    k = int(targets[0])
    assert k >= 3 and np.all(new.weights[0] > 0) and float(new.weights[0].max()) <= 0.5
    again, _t = mle.mix_up(raw, occ, 9, rng=np.random.default_rng(5))
    other, _t = mle.mix_up(raw, occ, 9, rng=np.random.default_rng(6))
    for p in range(4):
        assert again.means_invvars[p].tobytes() == new.means_invvars[p].tobytes()
    assert other.means_invvars[0].tobytes() != new.means_invvars[0].tobytes()


def test_mix_up_beyond_the_accumulators_limit_is_refused():
    raw, _par = _raw(np.random.default_rng(12), 5, [1, 1])
    with pytest.raises(ValueError, match="128"):
        mle.mix_up(raw, [1.0e7, 30.0], 140, rng=np.random.default_rng(0))
    new, targets = mle.mix_up(raw, [1.0e7, 30.0], 129, rng=np.random.default_rng(0))
    assert targets.tolist() == [128, 1]


# ---- the flat-start model and the tree writer -------------------------------------------------------------------------------
def test_init_mono_and_tree_round_trip():
    topo = SW._topology(7, [6, 7])
    raw_tm, raw_am, tree = mle.init_mono(topo, 39)
    assert raw_am.num_pdfs == 5 * 3 + 2 * 5 and raw_am.dim == 39
    tm = M.TransitionModel(raw_tm)
    assert tm.num_pdfs == raw_am.num_pdfs
    seen = set()
    for ph in range(1, 8):
        for st in topo.entry_for_phone(ph):
            if st.forward_pdf_class >= 0:
                seen.add(tree.compute([ph], st.forward_pdf_class))
    assert seen == set(range(raw_am.num_pdfs))               # the tree answers every (phone, class), one pdf each
    for p in range(raw_am.num_pdfs):
        assert raw_am.weights[p].tolist() == [1.0] and not raw_am.means_invvars[p].any() and np.all(raw_am.inv_vars[p] == 1.0)
        assert raw_am.gconsts[p][0] == np.float32(-0.5 * 39 * np.log(2 * np.pi))
    # initial transition log-probabilities are the topology's
    assert np.allclose(np.exp(raw_tm.log_probs[1:3]), [0.75, 0.25]) and raw_tm.log_probs[0] == 0
    # shared phones share their pdfs
    _tm2, am2, tree2 = mle.init_mono(topo, 13, shared_phones=[[2, 3], [6, 7]])
    assert am2.num_pdfs == 4 * 3 + 5
    assert tree2.compute([2], 1) == tree2.compute([3], 1) != tree2.compute([1], 1)
    assert tree2.compute([6], 4) == tree2.compute([7], 4)
    with pytest.raises(ValueError, match="pdf-classes"):
        mle.init_mono(topo, 13, shared_phones=[[1, 6]])
    with pytest.raises(ValueError, match="48"):
        mle.init_mono(topo, 49)
    # the model file and the tree file read back
    f = io.BytesIO()
    K.write_model(f, raw_tm, raw_am)
    tm_back, am_back = M.load_model_bytes(f.getvalue())
    assert tm_back.num_transition_ids == tm.num_transition_ids and am_back.num_pdfs == raw_am.num_pdfs
    for t in (tree, tree2):
        f = io.BytesIO()
        K.write_tree(f, t)
        assert K.read_tree(f.getvalue()) == t


def test_init_mono_is_the_yardsticks_tree():
    world_lex = SW.SynthWorld.build(n_words=5).lexicon
    ref = SW.monophone_from_stats(world_lex, {(1, 0): [np.zeros(3), np.ones(3), 10]})
    raw_tm, _am, tree = mle.init_mono(ref.tm.topo, 3)
    assert tree == ref.tree and np.array_equal(raw_tm.tuples, ref.tm.tuples)
    assert np.array_equal(raw_tm.log_probs, ref.tm.log_probs)


def test_write_tree_round_trips_a_shipped_tree_and_split_nodes():
    fx = helpers.Fixtures()
    for data in (K.load_acoustic_model_archive(helpers.REF / "mono_model.zip")["tree"], fx.g2p_archive["tree"]):
        t = K.read_tree(data)
        f = io.BytesIO()
        K.write_tree(f, t)
        assert K.read_tree(f.getvalue()) == t
        assert f.getvalue() == data                           # and the bytes are the file's
    se = K.EventMap("SE", key=1, yes_set=frozenset({3, 1, 9}), yes=K.EventMap("CE", answer=4),
                    no=K.EventMap("TE", key=-1, table=[None, K.EventMap("CE", answer=2)]))
    t = K.ContextDependency(3, 1, se)
    f = io.BytesIO()
    K.write_tree(f, t)
    assert K.read_tree(f.getvalue()) == t
