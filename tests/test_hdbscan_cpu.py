"""The HDBSCAN stage without a GPU: the host twins of the pair form, the core scores and the spanning tree against the numpy
restatement (tests/hdbscan_ref.py) bit for bit on integer vectors, the symmetry of the scores, the pair form against the sweep's
existing scores under the restatement's bound, the tree's properties against scipy, ``hdbscan.py`` against scikit-learn on the
twin's distances, the refusals and names of ``cluster.py``, and the twins under the host sanitizers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import hdbscan as H
from montreal_forced_aligner_amd import stats
from tests import hdbscan_ref as R

ROOT = Path(__file__).resolve().parents[1]
EXACT = {"grid": R.grid(), "grid5d": R.grid(5, 5), "all_equal": R.all_equal(), "path": R.path()[0], "integers": R.integer_points(130, 3, 7)}


def found(t):
    return t["lo"][: t["found"]], t["hi"][: t["found"]], t["score"][: t["found"]]


@pytest.mark.parametrize("name", sorted(EXACT))
@pytest.mark.parametrize("metric", ["euclidean", "dot"])
def test_twin_equals_the_restatement_bit_for_bit_on_integer_vectors(name, metric):
    x = EXACT[name]
    y, q, w = R.pair_form(metric, x)
    v = R.scores(y, q, w)
    assert np.array_equal(v, np.rint(v))                                   # integers: every sum was exact
    for k in (0, 1, 4, 64):
        got = stats.core_scores_host(metric, x, k, want_v=True)
        assert np.array_equal(got["y"], y) and np.array_equal(got["q"], q) and np.array_equal(got["v"], v)
        core = R.core(v, k)
        assert np.array_equal(got["core"], core), k
        lo, hi, m = R.kruskal(v, core)
        tree = stats.mreach_mst_host(metric, got["y"], got["q"], got["core"])
        for a, b in zip(found(tree), (lo, hi, m)):
            assert np.array_equal(a, b), k
        assert tree["found"] == x.shape[0] - 1 and R.is_spanning_tree(x.shape[0], tree["lo"], tree["hi"])
        on_v = stats.mreach_mst_host(metric, got["y"], got["q"], got["core"], v=v)      # the same tree from a given matrix
        assert all(np.array_equal(a, b) for a, b in zip(found(on_v), found(tree)))


def test_the_path_is_its_own_tree_and_equal_points_chain_from_the_first():
    x, _ = R.path()
    pf = stats.core_scores_host("euclidean", x, 0)
    t = stats.mreach_mst_host("euclidean", pf["y"], pf["q"], pf["core"])
    assert sorted(zip(t["lo"].tolist(), t["hi"].tolist())) == [(i, i + 1) for i in range(299)]
    pf = stats.core_scores_host("euclidean", R.all_equal(), 4)
    t = stats.mreach_mst_host("euclidean", pf["y"], pf["q"], pf["core"])
    assert list(zip(t["lo"].tolist(), t["hi"].tolist())) == [(0, j) for j in range(1, 20)] and not t["score"].any()


@pytest.mark.parametrize("metric", ["plda", "euclidean", "dot", "cosine"])
def test_scores_are_bit_symmetric_on_random_data(metric):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((97, 13)) * np.exp(rng.uniform(-3, 3, (97, 1)))
    got = stats.core_scores_host(metric, x, 3, R.model(13), want_v=True)
    assert np.isfinite(got["v"]).all() and np.array_equal(got["v"], got["v"].T)


@pytest.mark.parametrize("metric", ["plda", "euclidean", "dot"])
def test_pair_form_against_the_sweeps_scores(metric):
    rng = np.random.default_rng(17)
    for D in (1, 5, 50):
        x = rng.standard_normal((60, D)) * 3.0
        model = R.model(D, D)
        got = stats.core_scores_host(metric, x, 0, model, want_v=True)["v"]
        ref = stats.metric_sweep_host(metric, x, x, model=model, want_scores=True, want_bits=False)[0]
        bound = R.pair_bound(metric, x, model.psi)
        err = np.abs(got - ref)
        print(f"{metric} D={D}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
        assert (err <= bound).all()
        y, q, w = R.pair_form(metric, x, model.psi)                         # and against the definition, the same bound
        assert (np.abs(got - R.scores(y, q, w)) <= bound).all()


@pytest.mark.parametrize("metric,k", [("euclidean", 4), ("cosine", 9), ("plda", 2), ("dot", 0)])
def test_tree_properties_on_random_data(metric, k):
    sparse = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(29)
    n = 150
    x = rng.standard_normal((n, 6)) + rng.integers(0, 3, (n, 1)) * 4.0
    model = R.model(6, 3)
    _, _, dm = stats.pair_metric(metric)
    pf = stats.core_scores_host(metric, x, k, model, want_v=True)
    t = stats.mreach_mst_host(dm, pf["y"], pf["q"], pf["core"])
    assert t["found"] == n - 1 and R.is_spanning_tree(n, t["lo"], t["hi"])
    order = list(zip((-t["score"]).tolist(), t["lo"].tolist(), t["hi"].tolist()))
    assert order == sorted(order)                                          # sorted by the edge order
    m = np.minimum(pf["v"], np.minimum(pf["core"][:, None], pf["core"][None, :]))
    shift = float(m.max()) + 1.0                                           # weights shift − m > 0: scipy reads 0 as "no edge"
    weight = shift - m
    np.fill_diagonal(weight, 0.0)
    ref = float(sparse.minimum_spanning_tree(weight).sum())
    mine = float((shift - t["score"]).sum())
    assert abs(mine - ref) <= 1e-9 * abs(ref)


# (blob sizes, D, seed, strays, metric, min_cluster_size, cluster_selection_epsilon)
SKLEARN_CASES = [
    ((40, 40, 40, 40), 16, 1, 10, "euclidean", 15, 0.0),
    ((40, 40, 40, 40), 16, 1, 10, "euclidean", 5, 0.0),
    ((40, 40, 40, 40), 16, 1, 10, "cosine", 15, 0.0),
    ((40, 40, 40, 40), 16, 1, 10, "cosine", 5, 0.5),
    ((30, 50, 20), 8, 2, 0, "euclidean", 5, 0.0),
    ((30, 50, 20), 8, 2, 0, "euclidean", 15, 30.0),
    ((30, 50, 20), 8, 2, 0, "cosine", 5, 0.5),
    ((30, 50, 20), 8, 2, 0, "cosine", 15, 0.0),
    ((25, 25, 25, 25, 25), 4, 3, 15, "cosine", 5, 0.5),
    ((25, 25, 25, 25, 25), 4, 3, 15, "cosine", 15, 0.0),
    ((60, 15, 35), 3, 4, 5, "euclidean", 5, 0.0),
    ((60, 15, 35), 3, 4, 5, "euclidean", 15, 12.0),
    ((20, 20), 2, 5, 8, "euclidean", 5, 0.0),
]
_SEEN = {}


@pytest.mark.parametrize("case", SKLEARN_CASES, ids=lambda c: f"{len(c[0])}x{c[1]}-{c[4]}-mcs{c[5]}-eps{c[6]}")
def test_cluster_tree_against_scikit_learn(case):
    """``hdbscan.py`` on the twin's tree against ``sklearn.cluster.HDBSCAN(metric="precomputed")`` on the twin's distance matrix:
    the same partition and the same noise.  The pairwise distances are distinct; mutual-reachability distances still tie (a core
    distance is shared by every edge it caps), and where such a tie decides a point, scikit-learn's answer is that of its own
    sort order ("HDBSCAN"): the cases here are free of that."""
    sk = pytest.importorskip("sklearn.cluster")
    sizes, D, seed, strays, metric, mcs, eps = case
    x, truth = R.blobs(sizes, D, seed, strays=strays)
    ms = max(5, mcs // 4)
    _, unit, dm = stats.pair_metric(metric)
    pf = stats.core_scores_host(metric, x, 0, want_v=True)
    d = stats.score_to_distance(dm, pf["v"])
    assert np.array_equal(d, d.T)
    np.fill_diagonal(d, 0.0)
    iu = np.triu_indices(d.shape[0], 1)
    assert np.unique(d[iu]).shape[0] == iu[0].shape[0]                     # distinct pairwise distances
    ref = sk.HDBSCAN(metric="precomputed", min_cluster_size=mcs, min_samples=ms, cluster_selection_epsilon=float(eps)).fit(d.copy()).labels_
    got = CL.hdbscan_matrix(x, metric, distance_threshold=eps, min_cluster_size=mcs, min_samples=ms, strict=False, backend="host")
    _SEEN[case] = (int(ref.max()) + 1, int((ref < 0).sum()))
    assert R.same_partition(got, ref), (got.tolist(), ref.tolist())
    first = [int(np.flatnonzero(got == c)[0]) for c in range(int(got.max()) + 1)]
    assert first == sorted(first)                                          # numbered by smallest member


def test_the_scikit_learn_cases_cover_noise_and_a_merging_epsilon():
    sk = pytest.importorskip("sklearn.cluster")
    for case in SKLEARN_CASES:
        if case not in _SEEN:
            test_cluster_tree_against_scikit_learn(case)
    assert _SEEN[SKLEARN_CASES[0]] == (4, 10)                              # 4 blobs of 40 and 10 strays: 4 × 40 and 10 noise
    by_data = {}
    for case, (clusters, _) in _SEEN.items():
        by_data.setdefault(case[:5], {})[case[6] != 0.0] = clusters
    merged = [k for k, v in by_data.items() if True in v and False in v and v[True] < v[False]]
    assert {k[4] for k in merged} == {"euclidean", "cosine"}               # an ε that merges clusters, for both metrics
    assert any(n > 0 for _, n in _SEEN.values()) and len(SKLEARN_CASES) >= 8


def test_cluster_tree_pieces_on_a_hand_built_tree():
    # two tight groups of 3 joined by a long edge, and a far point
    lo, hi, d = [0, 1, 3, 4, 2, 0], [1, 2, 4, 5, 3, 6], [1.0, 1.5, 1.0, 1.2, 10.0, 50.0]
    labels = H.cluster_tree_labels(7, lo, hi, d, 3)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, -1]
    assert H.cluster_tree_labels(7, lo, hi, d, 3, 20.0).tolist() == [0, 0, 0, 1, 1, 1, -1]      # the root is never selected
    tree = H.condense_tree(7, H.single_linkage(7, lo, hi, d), 3)
    assert sorted(tree["child"][tree["child"] >= 7].tolist()) == [8, 9]
    assert H.cluster_tree_labels(1, [], [], [], 2).tolist() == [-1] and H.cluster_tree_labels(0, [], [], [], 2).shape == (0,)
    with pytest.raises(ValueError, match="spanning tree"):
        H.cluster_tree_labels(4, [0, 1, 0], [1, 2, 2], [1.0, 1.0, 1.0], 2)
    with pytest.raises(ValueError, match="min_cluster_size"):
        H.cluster_tree_labels(4, [0, 1, 2], [1, 2, 3], [1.0, 1.0, 1.0], 1)
    zero = H.cluster_tree_labels(6, [0, 1, 3, 4, 2], [1, 2, 4, 5, 3], [0.0, 0.0, 0.0, 0.0, 3.0], 3)  # λ = +inf where d <= 0
    assert zero.tolist() == [0, 0, 0, 1, 1, 1]


def test_a_point_without_finite_scores_is_noise_and_far_groups_join_once():
    x, _ = R.blobs((12, 12), 3, 8, spread=30.0)
    x = np.concatenate([x, [[np.nan, 0.0, 0.0]]])
    pf = stats.core_scores_host("euclidean", x, 3, want_v=True)
    assert pf["core"][24] == -np.inf and np.isfinite(pf["core"][:24]).all()
    t = stats.mreach_mst_host("euclidean", pf["y"], pf["q"], pf["core"])
    assert t["found"] == 23 and t["lo"].shape[0] == 24 and t["score"][-1] == -np.inf and (t["lo"][-1], t["hi"][-1]) == (0, 24)
    clean = stats.core_scores_host("euclidean", x[:24], 3)
    tc = stats.mreach_mst_host("euclidean", clean["y"], clean["q"], clean["core"])
    assert all(np.array_equal(a[:23], b) for a, b in zip((t["lo"], t["hi"], t["score"]), (tc["lo"], tc["hi"], tc["score"])))
    labels = CL.hdbscan_matrix(x, "euclidean", distance_threshold=0.0, min_cluster_size=5, backend="host")
    assert labels[24] == -1 and np.array_equal(labels[:24], CL.hdbscan_matrix(x[:24], "euclidean", distance_threshold=0.0, min_cluster_size=5,
                                                                             backend="host"))
    truth = R.blobs((12, 12), 3, 8, spread=30.0)[1]
    crossing = [(a, b) for a, b in zip(tc["lo"].tolist(), tc["hi"].tolist()) if truth[a] != truth[b]]
    assert len(crossing) == 1 and (tc["lo"][-1], tc["hi"][-1]) == crossing[0]


def test_refusals_and_names():
    x = np.concatenate([np.zeros((6, 2)), np.ones((6, 2)) * 10.0]) + np.arange(12)[:, None] * 0.01
    with pytest.raises(_lib.MfaHipError, match="neighbours"):
        stats.core_scores_host("euclidean", x, 65)
    with pytest.raises(_lib.MfaHipError, match="neighbours"):
        stats.core_scores_host("euclidean", x, -1)
    with pytest.raises(_lib.MfaHipError, match="metric"):
        stats.core_scores_host("manhattan", x, 1)
    with pytest.raises(_lib.MfaHipError, match="dimension"):
        stats.core_scores_host("euclidean", np.zeros((3, 1025)), 1)
    bad = R.model(2)
    bad.psi = np.array([1.0, 0.0])
    with pytest.raises(_lib.MfaHipError, match="psi"):
        stats.core_scores_host("plda", x, 1, bad)
    lib = _lib.lib()
    assert lib.mfa_debug_hdbscan_core_host(None, 3, 2, 1, None, 1, None, None, None, None, None) == -1
    assert lib.mfa_debug_hdbscan_core_host(None, 1 << 31, 2, 1, None, 1, None, None, None, None, None) == -5
    assert lib.mfa_debug_hdbscan_core_host(None, 0, 2, 1, None, 1, None, None, None, None, None) == 0
    with pytest.raises(ValueError, match="min_samples"):
        CL.hdbscan_matrix(x, "euclidean", distance_threshold=1.0, min_cluster_size=4, min_samples=66, backend="host")
    with pytest.raises(ValueError, match="min_cluster_size"):
        CL.hdbscan_matrix(x, "euclidean", distance_threshold=1.0, min_cluster_size=1, backend="host")
    with pytest.raises(ValueError, match="plda"):
        CL.hdbscan_matrix(x, "plda", distance_threshold=1.0, backend="host")
    with pytest.raises(ValueError, match="backend"):
        CL.hdbscan_matrix(x, "euclidean", distance_threshold=1.0, backend="cpu")
    with pytest.raises(ValueError, match="one cluster"):
        CL.hdbscan_matrix(x[:3], "euclidean", distance_threshold=0.0, min_cluster_size=4, min_samples=2, backend="host")   # all noise
    with pytest.raises(NotImplementedError, match="hdbscan"):               # routing it through cluster_matrix is a later change
        CL.cluster_matrix(x, CL.ClusterType.hdbscan, "euclidean", distance_threshold=1.0, backend="host")
    ids = [f"u{i}" for i in range(13)]
    far = np.concatenate([x, [[500.0, -300.0]]])
    names = CL.hdbscan_utterances(ids, far, metric="euclidean", distance_threshold=0.0, min_cluster_size=4, min_samples=2, backend="host")
    assert names == {**{f"u{i}": "Cluster 0" for i in range(6)}, **{f"u{i}": "Cluster 1" for i in range(6, 12)}, "u12": "MFA_UNKNOWN"}
    with pytest.raises(ValueError, match="utterances"):
        CL.hdbscan_utterances(ids[:3], far, metric="euclidean", distance_threshold=0.0, backend="host")


def test_min_samples_default_and_the_automatic_threshold():
    x, truth = R.blobs((30, 30, 30), 4, 12, spread=10.0)
    auto = CL.hdbscan_matrix(x, "euclidean", min_cluster_size=8, backend="host")
    eps = CL.distance_threshold(x, "euclidean", 8, backend="host")
    assert np.array_equal(auto, CL.hdbscan_matrix(x, "euclidean", distance_threshold=eps, min_cluster_size=8, min_samples=5, backend="host"))
    assert R.same_partition(auto, truth)


# ---- sanitizers --------------------------------------------------------------------------------------------------------------------
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "hdbscan_check"
    csrc = ROOT / "montreal_forced_aligner_amd" / "csrc"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "hdbscan_check.cpp"), str(csrc / "hdbscan_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
