"""The clustering stage without a GPU: the host twin of DBSCAN on a bit matrix against the numpy restatement (tests/dbscan_ref.py)
and against scikit-learn, the hand-built graphs, the knee, the threshold estimate against a brute-force k-th neighbour, the
refusals and the speaker names of ``cluster.py``, the generated corpus of the GPU flow test on the host reference alone, and
the twins under the host sanitizers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import stats
from tests import cluster_case as CC
from tests import dbscan_ref as R

ROOT = Path(__file__).resolve().parents[1]


def check_against_ref(adj, min_samples):
    ref = R.dbscan(adj, min_samples)
    got = stats.dbscan_from_bits_host(R.pack(adj), min_samples)
    n = adj.shape[0]
    assert np.array_equal(R.unpack(got["bits"], n), ref["adj"]) and not R.padding_bits(got["bits"], n).any()
    for key in ("labels", "core", "count"):
        assert np.array_equal(got[key], ref[key]), key
    assert got["n_clusters"] == ref["n_clusters"]
    return got


@pytest.mark.parametrize("n", R.SIZES)
def test_twin_equals_the_restatement_on_random_graphs(n):
    kinds = set()
    for seed in range(4):
        for ms in (1, 3, 5):
            got = check_against_ref(R.random_graph(n, 100 * n + seed), ms)
            kinds |= {("core", bool(c)) for c in got["core"]} | {("noise", bool(l < 0)) for l in got["labels"]}
    if n >= 63:
        assert {("core", True), ("core", False), ("noise", True), ("noise", False)} <= kinds


@pytest.mark.parametrize("name", sorted(R.hand_built()))
def test_hand_built_graphs(name):
    adj, ms, want = R.hand_built()[name]
    got = check_against_ref(adj, ms)
    assert got["labels"].tolist() == want


def test_the_or_rule_on_an_asymmetric_matrix():
    adj, ms, _ = R.hand_built()["asymmetric"]
    assert not (adj & adj.T).any() and not adj.diagonal().any()          # no pair in both directions, no diagonal
    got = stats.dbscan_from_bits_host(R.pack(adj), ms)
    assert np.array_equal(R.unpack(got["bits"], 6), adj | adj.T | np.eye(6, dtype=bool))
    assert got["count"].tolist() == [3] * 6


def test_twin_equals_scikit_learn_on_integer_points():
    """Integer coordinates and ε² = m + ½: every form of the squared distance is an exact integer, so no pair ties with ε."""
    sk = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(5)
    for case in range(40):
        n, d = int(rng.integers(5, 131)), int(rng.integers(1, 5))
        x = rng.integers(-6, 7, size=(n, d)).astype(np.float64)
        if case % 4 == 0:
            x[n // 2:] = x[: n - n // 2]                                   # duplicates
        m, ms = int(rng.integers(0, 9)), int(rng.integers(1, 8))
        eps = float(np.sqrt(m + 0.5))
        dist = R.euclidean(x, x)
        d2 = np.rint(dist * dist)
        assert np.array_equal(d2, ((x[:, None] - x[None]) ** 2).sum(axis=2)) and not (d2 == m + 0.5).any()
        assert (np.abs(dist - eps) > 1e-9).all()                          # on the reference's own distances: no tie with ε
        ref = sk.DBSCAN(eps=eps, min_samples=ms, metric="precomputed").fit(dist)
        bits = stats.neighbor_bits_host("euclidean", x, x, eps)
        assert np.array_equal(R.unpack(bits, n), dist <= eps)
        got = stats.dbscan_from_bits_host(bits, ms)
        assert np.array_equal(got["labels"], ref.labels_), case
        assert sorted(np.flatnonzero(got["core"]).tolist()) == sorted(ref.core_sample_indices_.tolist())


def test_neighbor_bits_host_metrics_against_the_direct_forms():
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((37, 6)), rng.standard_normal((70, 6))
    for metric, dist in (("euclidean", R.euclidean(x, y)), ("cosine", R.cosine(x, y))):
        eps = float(np.median(dist))
        bits = stats.neighbor_bits_host(metric, x, y, eps)
        away = np.abs(dist - eps) > 1e-9                                   # pairs within rounding of ε may go either way
        assert np.array_equal(R.unpack(bits, 70)[away], (dist <= eps)[away]) and not R.padding_bits(bits, 70).any()
    model = CC.corpus()["model"]
    v = CC.corpus()["vectors"]["plda"]
    dist = R.plda(model, v[:20], v)
    eps = float(np.median(dist))
    away = np.abs(dist - eps) > 1e-8
    assert np.array_equal(R.unpack(stats.neighbor_bits_host("plda", v[:20], v, eps, model), v.shape[0])[away], (dist <= eps)[away])
    assert not R.unpack(stats.neighbor_bits_host("euclidean", x, y, -1.0), 70).any()      # ε < 0: nothing
    with pytest.raises(_lib.MfaHipError, match="bytes"):
        stats.neighbor_bits_host("euclidean", x, y, 1.0, max_bytes=100)
    with pytest.raises(_lib.MfaHipError, match="metric"):
        stats.neighbor_bits_host("manhattan", x, y, 1.0)


# ---- the knee ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner,n,steep,flat", [(29, 100, 10.0, 1.0), (10, 60, 5.0, 0.25), (150, 400, 3.0, 0.5)])
def test_knee_of_a_piecewise_linear_curve_is_its_corner(corner, n, steep, flat):
    i = np.arange(n, dtype=np.float64)
    y = np.where(i <= corner, steep * i, steep * corner + flat * (i - corner))
    assert CL.knee_index(y) == corner
    for scale in (0.001, 3.7, 1e6):
        assert CL.knee_index(scale * y) == corner
    assert CL.knee_index(y + 12.5) == corner


def test_a_straight_line_has_no_knee():
    assert CL.knee_index(3.0 * np.arange(80) + 1.0) is None
    assert CL.knee_index(np.full(20, 2.0)) is None and CL.knee_index([1.0, 2.0]) is None
    x = np.arange(80, dtype=np.float64)[:, None] * np.ones((1, 3))        # points on a line: every 1st-neighbour distance equal
    with pytest.raises(CL.NoKneeError, match="distance_threshold"):
        CL.distance_threshold(x, "euclidean", 2, backend="host")


def test_distance_threshold_against_a_brute_force_kth_neighbour():
    rng = np.random.default_rng(3)
    # a jittered lattice (every neighbour distance near 1) and a tight group: the sorted curve rises fast, then lies flat
    lattice = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0)), axis=-1).reshape(-1, 2) + rng.uniform(-0.03, 0.03, (144, 2)) + 3.0
    x = np.concatenate([lattice, rng.standard_normal((20, 2)) * 0.02 + 40.0])
    for metric, dist in (("euclidean", R.euclidean(x, x)), ("cosine", R.cosine(x, x))):
        for ms in (2, 5):
            np.fill_diagonal(dist, np.inf)
            kth = np.sort(np.sort(dist, axis=1)[:, ms - 2])
            got = np.sort(CL.kth_neighbor_distances(x, metric, ms - 1, backend="host"))
            np.testing.assert_allclose(got, kth, rtol=1e-9, atol=1e-9)
            knee = CL.knee_index(kth)
            assert metric != "euclidean" or knee is not None
            if knee is None:
                with pytest.raises(CL.NoKneeError):
                    CL.distance_threshold(x, metric, ms, backend="host")
            else:
                assert CL.distance_threshold(x, metric, ms, backend="host") == pytest.approx(kth[knee], rel=1e-9, abs=1e-9)
    with pytest.raises(ValueError, match="distance_threshold"):
        CL.distance_threshold(x, "euclidean", 66, backend="host")
    with pytest.raises(ValueError, match="distance_threshold"):
        CL.distance_threshold(x, "euclidean", 1, backend="host")


# ---- cluster.py --------------------------------------------------------------------------------------------------------------------
def test_cluster_matrix_refusals_and_strict():
    x = np.concatenate([np.zeros((5, 2)), np.ones((5, 2)) * 10.0])
    for ctype in CL.ClusterType:
        if ctype is CL.ClusterType.dbscan:
            continue
        with pytest.raises(NotImplementedError, match=ctype.name):
            CL.cluster_matrix(x, ctype, "euclidean", distance_threshold=1.0, backend="host")
    with pytest.raises(ValueError, match="plda"):
        CL.cluster_matrix(x, "dbscan", "plda", distance_threshold=1.0, backend="host")
    with pytest.raises(ValueError):
        CL.cluster_matrix(x, "dbscan", "manhattan", distance_threshold=1.0, backend="host")
    with pytest.raises(ValueError, match="backend"):
        CL.cluster_matrix(x, "dbscan", "euclidean", distance_threshold=1.0, backend="cpu")
    two = CL.cluster_matrix(x, CL.ClusterType.dbscan, CL.DistanceMetric.euclidean, distance_threshold=1.0, min_cluster_size=3, backend="host")
    assert two.tolist() == [0] * 5 + [1] * 5
    with pytest.raises(ValueError, match="one cluster"):                  # one cluster, strict
        CL.cluster_matrix(x, "dbscan", "euclidean", distance_threshold=100.0, min_cluster_size=3, backend="host")
    with pytest.raises(ValueError, match="one cluster"):                  # all noise is one label too
        CL.cluster_matrix(x, "dbscan", "euclidean", distance_threshold=1.0, min_cluster_size=8, backend="host")
    one = CL.cluster_matrix(x, "dbscan", "euclidean", distance_threshold=100.0, min_cluster_size=3, strict=False, backend="host")
    assert one.tolist() == [0] * 10


def test_speaker_names():
    x = np.concatenate([np.zeros((4, 2)), np.ones((4, 2)) * 10.0, [[50.0, 50.0]]])
    ids = [f"u{i}" for i in range(9)]
    names = CL.cluster_utterances(ids, x, metric="euclidean", distance_threshold=1.0, min_cluster_size=3, backend="host")
    assert names == {**{f"u{i}": "Cluster 0" for i in range(4)}, **{f"u{i}": "Cluster 1" for i in range(4, 8)}, "u8": "MFA_UNKNOWN"}
    with pytest.raises(ValueError, match="utterances"):
        CL.cluster_utterances(ids[:3], x, metric="euclidean", distance_threshold=1.0, backend="host")


@pytest.mark.parametrize("metric", ["plda", "cosine", "euclidean"])
def test_host_reference_separates_the_generated_speakers(metric):
    """The corpus and thresholds of tests/test_gpu_cluster_flow.py: the host reference alone finds exactly the speakers."""
    c = CC.corpus()
    lo, hi = c["gap"][metric]
    assert hi - lo > 1e-3 * max(abs(lo), abs(hi))
    assert (np.abs(c["dist"][metric] - c["eps"][metric]) > 1e-6).all()     # no pair, in either direction, within rounding of ε
    labels = CL.cluster_matrix(c["vectors"][metric], "dbscan", metric, plda=c["model"], distance_threshold=c["eps"][metric],
                               min_cluster_size=CC.MIN_CLUSTER_SIZE, backend="host")
    assert CC.same_partition(labels, c["speakers"])


# ---- sanitizers --------------------------------------------------------------------------------------------------------------------
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "cluster_check"
    csrc = ROOT / "montreal_forced_aligner_amd" / "csrc"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "cluster_check.cpp"), str(csrc / "plda_host.cpp"), str(csrc / "cluster_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
