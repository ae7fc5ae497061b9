"""The silhouette stage without a GPU: the known answer, the longdouble restatement against scikit-learn, the host twin against
the restatement (bit for bit on integer vectors with the dot metric, under the derived bound otherwise, and the bound itself is
small), the tie rule of b, the noise modes, the refusals, relabelling and permuting, ``cluster_vectors`` on the host backend, and
the twin under the host sanitizers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import stats
from tests import hdbscan_ref as H
from tests import silhouette_ref as R

ROOT = Path(__file__).resolve().parents[1]


def blob_case(metric, n=300, D=50, seed=61):
    """Random blobs ordered by cluster: (x, offsets, model).  Cosine: unit rows for the dot metric."""
    sizes = [n // 2, n // 4, n // 8, n - n // 2 - n // 4 - n // 8 - 1, 1]
    x, truth = H.blobs(sizes, D, seed, spread=2.0)
    order, offsets = R.sort_by_label(truth)
    x = np.ascontiguousarray(x[order])
    model = H.model(D, 5)
    if metric == "cosine":
        return np.ascontiguousarray(stats._unit_rows(x)), offsets, model, "dot"
    return x, offsets, model, metric


# ---- the known answer ----------------------------------------------------------------------------------------------------------------
def test_known_answer():
    x = np.array([[0.0], [1.0], [5.0], [9.0]])
    want = [0.8, 0.75, 0.0, 0.0]
    assert CL.silhouette_samples(x, [0, 0, 1, 2], "euclidean", backend="host").tolist() == want
    assert CL.silhouette_samples(x[[3, 1, 2, 0]], [7, -5, 3, -5], "euclidean", backend="host").tolist() == [0.0, 0.75, 0.0, 0.8]
    r = stats.silhouette_host("euclidean", x, [0, 2, 3, 4], want_parts=True)
    assert r["a"].tolist() == [1.0, 1.0, 0.0, 0.0] and r["b"].tolist() == [5.0, 4.0, 4.0, 4.0] and r["bj"].tolist() == [1, 1, 2, 1]
    assert CL.silhouette_score(x, [0, 0, 1, 2], "euclidean", backend="host") == np.mean(want)
    assert np.asarray(R.samples(R.distances("euclidean", x), [0, 2, 3, 4])["s"], dtype=np.float64).tolist() == want


# ---- the restatement against scikit-learn --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_restatement_against_scikit_learn(metric):
    from sklearn.metrics import silhouette_samples
    x, _ = H.blobs((100, 80, 70, 50), 50, 67, spread=2.0)
    labels = R.random_labels(300, 5, 68, noise=20, singleton=True)
    assert (labels == -1).sum() == 20 and (labels == 1000).sum() == 1
    order, offsets = R.sort_by_label(labels)
    xs = x[order] if metric == "euclidean" else stats._unit_rows(x[order])
    s = np.empty(300)
    s[order] = np.asarray(R.samples(R.distances("euclidean" if metric == "euclidean" else "dot", xs), offsets)["s"], dtype=np.float64)
    np.testing.assert_allclose(s, silhouette_samples(x, labels, metric=metric), rtol=0, atol=1e-12)
    # and the wrapper's sort, offsets and scatter on the twin
    np.testing.assert_allclose(CL.silhouette_samples(x, labels, metric, backend="host"), silhouette_samples(x, labels, metric=metric),
                               rtol=0, atol=1e-12)


# ---- the twin against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130, 300])
def test_twin_is_bit_exact_on_integer_vectors(n):
    for D in (1, 3, 50):
        x = H.integer_points(n, D, 2000 * n + D)
        for name, offsets in R.layouts(n).items():
            r = stats.silhouette_host("dot", x, offsets, want_parts=True)
            ref = R.samples(R.distances("dot", x), offsets)
            for key in ("a", "b", "bj"):
                assert np.array_equal(r[key], np.asarray(ref[key]).astype(r[key].dtype)), (D, name, key)
            a, b = r["a"], r["b"]
            den = np.where(a < b, b, a)
            with np.errstate(invalid="ignore", divide="ignore"):
                want = np.where((ref["sizes"][ref["own"]] == 1) | (den == 0), 0.0, (b - a) / den)   # one IEEE division of exact operands
            assert np.array_equal(r["sil"], want), (D, name)


@pytest.mark.parametrize("metric", ["euclidean", "plda", "cosine"])
def test_twin_under_the_derived_bound(metric):
    x, offsets, model, name = blob_case(metric)
    bound, ref = R.bound(name, x, offsets, model.psi)
    assert bound.max() <= 1e-9, bound.max()                           # the bound cannot hide a failure
    r = stats.silhouette_host(name, x, offsets, model, want_parts=True, want_v=True)
    err = np.abs(r["sil"] - np.asarray(ref["s"], dtype=np.float64))
    print(f"{metric}: largest bound {bound.max():.3e}, largest error {err.max():.3e}")
    assert (err <= bound).all()
    assert np.array_equal(r["bj"], ref["bj"])
    again = stats.silhouette_host(name, x, offsets, model, want_parts=True, v=r["v"])   # from the stored matrix: the same bits
    assert all(np.array_equal(r[k], again[k]) for k in ("sil", "a", "b", "bj"))
    assert r["sil"][-1] == 0.0 and bound[-1] == 0.0                   # the singleton


def test_plda_distances_are_measured_from_the_smallest_one():
    """The cluster layer's plda rule: the restatement on d − d0 (d0 the smallest −LLR between two points) under the derived bound;
    every value in [−1, 1]; and on the generated speaker corpus, whose −LLR means are negative, the true speakers score higher than a
    shuffled labelling — with the signed distance taken as it is they scored lower (−0.935 against +1.022)."""
    from tests import cluster_case as CC
    x, offsets, model, _ = blob_case("plda", n=120, D=16, seed=83)
    labels = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    bound, ref = R.bound("plda", x, offsets, model.psi, from_smallest=True)
    got = CL.silhouette_samples(x, labels, "plda", plda=model, backend="host")
    assert bound.max() <= 1e-9 and (np.abs(got - np.asarray(ref["s"], dtype=np.float64)) <= bound).all()
    assert (np.abs(got) <= 1.0).all() and got[-1] == 0.0
    raw = stats.silhouette_host("plda", x, offsets, model, want_parts=True)
    assert np.array_equal(CL.silhouette_from_means(raw["a"], raw["b"], np.diff(offsets)[labels]), raw["sil"])      # no shift: the twin's finish
    c = CC.corpus()
    v = c["vectors"]["plda"]
    true = CL.silhouette_score(v, c["speakers"], "plda", plda=c["model"], backend="host")
    shuffled = CL.silhouette_score(v, np.random.default_rng(9).permutation(c["speakers"]), "plda", plda=c["model"], backend="host")
    assert -1.0 <= shuffled < true <= 1.0
    order, off = R.sort_by_label(c["speakers"])
    assert stats.silhouette_host("plda", v[order], off, c["model"])["sil"].mean() < 0.0                           # the signed distance as it is


def test_tie_of_b_goes_to_the_lower_cluster():
    x = np.array([[0.0], [0.0], [-3.0], [-3.0], [3.0], [3.0], [5.0]])
    r = stats.silhouette_host("euclidean", x, [0, 2, 4, 6, 7], want_parts=True)
    assert r["b"][:2].tolist() == [3.0, 3.0] and r["bj"][:2].tolist() == [1, 1]
    assert r["bj"][2:].tolist() == [0, 0, 3, 3, 2]
    nan = stats.silhouette_host("dot", np.array([[1.0], [1.0], [np.nan], [2.0]]), [0, 2, 3, 4], want_parts=True)
    assert nan["bj"][:2].tolist() == [2, 2] and nan["b"][:2].tolist() == [-1.0, -1.0]   # a NaN mean is never taken


def test_noise_modes():
    x, truth = H.blobs((20, 20, 15), 4, 71, spread=6.0, strays=5)
    as_cluster = CL.silhouette_samples(x, truth, "euclidean", noise="cluster", backend="host")
    assert np.isfinite(as_cluster).all()
    excluded = CL.silhouette_samples(x, truth, "euclidean", noise="exclude", backend="host")
    assert np.isnan(excluded[truth == -1]).all() and np.isfinite(excluded[truth != -1]).all()
    keep = truth != -1
    assert np.array_equal(excluded[keep], CL.silhouette_samples(x[keep], truth[keep], "euclidean", backend="host"))
    assert CL.silhouette_score(x, truth, "euclidean", noise="exclude", backend="host") == np.mean(excluded[keep])
    assert CL.silhouette_score(x, truth, "euclidean", backend="host") == np.mean(as_cluster)
    assert np.mean(excluded[keep]) > np.mean(as_cluster)              # the strays are no cluster


def test_relabelling_and_permuting_keep_every_points_value():
    x, truth = H.blobs((40, 30, 20, 1), 6, 73, spread=3.0)
    base = CL.silhouette_samples(x, truth, "euclidean", backend="host")
    order, offsets = R.sort_by_label(truth)
    bound = np.empty(x.shape[0])
    bound[order] = R.bound("euclidean", x[order], offsets)[0]
    relabelled = CL.silhouette_samples(x, np.array([50, -1, 7, 8])[truth], "euclidean", backend="host")
    perm = np.random.default_rng(5).permutation(x.shape[0])
    permuted = CL.silhouette_samples(x[perm], truth[perm], "euclidean", backend="host")
    assert (np.abs(relabelled - base) <= 2 * bound).all() and (np.abs(permuted - base[perm]) <= 2 * bound[perm]).all()
    assert bound.max() <= 1e-9


def test_refusals():
    x = np.arange(12.0).reshape(6, 2)
    for labels, word in (([0] * 6, "Number of labels is 1"), (list(range(6)), "Number of labels is 6"), ([0, 1] * 2, "labels for 6"),
                         ([0.5] * 6, "integers")):
        with pytest.raises(ValueError, match=word):
            CL.silhouette_samples(x, labels, "euclidean", backend="host")
    with pytest.raises(ValueError, match="Number of labels is 1"):
        CL.silhouette_samples(x, [0, 0, 0, -1, -1, -1], "euclidean", noise="exclude", backend="host")
    bad = x.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        CL.silhouette_samples(bad, [0, 0, 0, 1, 1, 1], "euclidean", backend="host")
    with pytest.raises(ValueError, match="noise"):
        CL.silhouette_samples(x, [0, 0, 0, 1, 1, 1], "euclidean", noise="drop", backend="host")
    with pytest.raises(ValueError, match="backend"):
        CL.silhouette_samples(x, [0, 0, 0, 1, 1, 1], "euclidean", backend="cpu")
    with pytest.raises(ValueError, match="plda"):
        CL.silhouette_samples(x, [0, 0, 0, 1, 1, 1], "plda", backend="host")
    for offsets, word in (([0, 6], "clusters"), ([0, 3, 3, 6], "offsets"), ([1, 3, 6], "offsets"), ([0, 3, 5], "offsets"),
                          ([0, 4, 2, 6], "offsets"), (list(range(8)), "clusters")):
        with pytest.raises(_lib.MfaHipError, match=word):
            stats.silhouette_host("euclidean", x, offsets)
    with pytest.raises(_lib.MfaHipError, match="metric"):
        stats.silhouette_host("manhattan", x, [0, 3, 6])
    with pytest.raises(_lib.MfaHipError, match="dimension"):
        stats.silhouette_host("euclidean", np.zeros((3, 1025)), [0, 1, 3])
    model = H.model(2)
    model.psi = np.array([1.0, 0.0])
    with pytest.raises(_lib.MfaHipError, match="psi"):
        stats.silhouette_host("plda", x, [0, 3, 6], model)
    lib = _lib.lib()
    assert lib.mfa_debug_silhouette_host(None, 3, 2, 1, None, None, 2, None, None, None, None, None, None) == -1
    assert lib.mfa_debug_silhouette_host(None, 1 << 31, 2, 1, None, None, 2, None, None, None, None, None, None) == -5
    assert lib.mfa_debug_silhouette_host(None, 0, 2, 1, None, None, 0, None, None, None, None, None, None) == 0


# ---- cluster_vectors on the host backend ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctype", ["dbscan", "hdbscan"])
def test_cluster_vectors_on_the_host_backend(ctype):
    from sklearn.metrics import silhouette_score
    x, truth = H.blobs((30, 30, 30), 4, 12, spread=10.0)
    x = x + 20.0                                                      # away from the origin: cosine and euclidean differ
    kw = dict(min_cluster_size=8, backend="host")
    for metric in ("euclidean", "cosine"):
        labels, score = CL.cluster_vectors(x, CL.ClusterType(ctype), metric, **kw)
        single = (CL.cluster_matrix(x, CL.ClusterType.dbscan, metric, **kw) if ctype == "dbscan" else CL.hdbscan_matrix(x, metric, **kw))
        assert np.array_equal(labels, single)
        to_fit, score_metric = x, metric
        if ctype == "hdbscan" and metric == "cosine":                 # the reference's score_metric rule
            to_fit, score_metric = stats._unit_rows(x), "euclidean"
        assert abs(score - silhouette_score(to_fit, labels, metric=score_metric)) <= 1e-12
    model = H.model(4, 3)
    labels, score = CL.cluster_vectors(x, ctype, "plda", plda=model, **kw)
    assert score == CL.silhouette_score(x, labels, "plda", plda=model, backend="host")
    names, score2 = CL.cluster_vectors_utterances([f"u{i}" for i in range(90)], x, ctype, metric="euclidean", **kw)
    assert score2 == CL.cluster_vectors(x, ctype, "euclidean", **kw)[1] and set(names.values()) <= {f"Cluster {c}" for c in range(3)} | {"MFA_UNKNOWN"}
    with pytest.raises(ValueError, match="utterances"):
        CL.cluster_vectors_utterances(["u0"], x, ctype, metric="euclidean", **kw)


def test_cluster_vectors_strict_and_refused_types():
    x = np.concatenate([np.zeros((6, 2)), np.ones((6, 2)) * 10.0]) + np.arange(12)[:, None] * 0.01
    one = dict(metric="euclidean", distance_threshold=100.0, min_cluster_size=3, backend="host")          # every point one cluster
    with pytest.raises(ValueError, match="Only found one cluster"):
        CL.cluster_vectors(x, "dbscan", **one)
    labels, score = CL.cluster_vectors(x, "dbscan", strict=False, **one)
    assert score is None and np.array_equal(labels, np.zeros(12, dtype=np.int64))
    with pytest.raises(ValueError, match="Only found one cluster"):
        CL.cluster_vectors(x[:3], "hdbscan", metric="euclidean", distance_threshold=0.0, min_cluster_size=4, min_samples=2, backend="host")
    labels, score = CL.cluster_vectors(x[:3], "hdbscan", metric="euclidean", distance_threshold=0.0, min_cluster_size=4, min_samples=2,
                                       strict=False, backend="host")
    assert score is None and (labels == -1).all()
    for ctype in CL.ClusterType:
        if ctype not in (CL.ClusterType.dbscan, CL.ClusterType.hdbscan):
            with pytest.raises(NotImplementedError, match=ctype.name):
                CL.cluster_vectors(x, ctype, "euclidean", backend="host")
    labels, score = CL.cluster_vectors(x, "dbscan", metric="euclidean", distance_threshold=1.0, min_cluster_size=3, backend="host")
    assert labels.tolist() == [0] * 6 + [1] * 6 and score > 0.9


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------------
def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "silhouette_check"
    csrc = ROOT / "montreal_forced_aligner_amd" / "csrc"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "silhouette_check.cpp"), str(csrc / "silhouette_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
