"""``cluster_vectors`` end to end on the generated corpus of tests/cluster_case.py (12 speakers × 8 utterances, D = 16, in random
order): train PLDA → transform on the device → cluster and score on the device, for dbscan and hdbscan and the three metrics,
against ``backend="host"``: the same labels, scores within the derived bound; the true speakers score higher than a shuffled
labelling; the kalpy-layer calls."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import kalpy_api as K
from montreal_forced_aligner_amd import stats
from tests import cluster_case as CC
from tests import silhouette_ref as R

pytestmark = pytest.mark.gpu

METRICS = ("plda", "cosine", "euclidean")


def threshold(c, ctype, metric):
    """The corpus's ε in the distance the type clusters on: hdbscan's cosine is euclidean on unit rows, |u − v|² = 2 (1 − cos)."""
    return float(np.sqrt(2.0 * c["eps"]["cosine"])) if (ctype, metric) == ("hdbscan", "cosine") else c["eps"][metric]


def vectors(engine, c, metric):
    return stats.plda_transform(engine, c["model"], c["raw"]).cpu().numpy() if metric == "plda" else c["vectors"][metric]


def score_bound(c, ctype, metric, x, labels):
    """The bound on the mean's difference between two runs of the contract: the mean of twice the per-row bound (each run is within it
    of the restatement), the device's root allowed 1 ulp."""
    name, fit = metric, x
    if metric == "cosine":
        name, fit = ("euclidean" if ctype == "hdbscan" else "dot"), stats._unit_rows(x)
    order, offsets = R.sort_by_label(labels)
    return float(np.mean(2 * R.bound(name, np.ascontiguousarray(fit[order]), offsets, c["model"].psi, ulp_root=2,
                                     from_smallest=metric == "plda")[0]))


@pytest.mark.parametrize("ctype", ["dbscan", "hdbscan"])
@pytest.mark.parametrize("metric", METRICS)
def test_device_and_host_give_the_same_labels_and_scores(engine, ctype, metric):
    c = CC.corpus()
    x = vectors(engine, c, metric)
    kw = dict(plda=c["model"], distance_threshold=threshold(c, ctype, metric), min_cluster_size=CC.MIN_CLUSTER_SIZE)
    labels, score = CL.cluster_vectors(x, ctype, metric, engine=engine, **kw)
    h_labels, h_score = CL.cluster_vectors(x, ctype, metric, backend="host", **kw)
    assert np.array_equal(labels, h_labels) and CC.same_partition(labels, c["speakers"])
    bound = score_bound(c, ctype, metric, x, labels)
    print(f"{ctype} {metric}: score {score:.6f}, host {h_score:.6f}, bound {bound:.3e}")
    assert bound <= 1e-9 and abs(score - h_score) <= bound
    assert -1.0 <= score <= 1.0                                        # every distance is measured so that none is negative


@pytest.mark.parametrize("ctype", ["dbscan", "hdbscan"])
@pytest.mark.parametrize("metric", METRICS)
def test_true_speakers_score_higher_than_a_shuffled_labelling(engine, ctype, metric):
    """For plda this is what the zero point of ``cluster.silhouette_samples`` is for: with the signed −LLR taken as it is, a ≈ −21.5 and
    b ≈ −9 for the true speakers of this corpus and (b − a) / max(a, b) gave −0.935 against +1.022 for the shuffled labelling."""
    c = CC.corpus()
    x = vectors(engine, c, metric)
    kw = dict(plda=c["model"], distance_threshold=threshold(c, ctype, metric), min_cluster_size=CC.MIN_CLUSTER_SIZE)
    labels, score = CL.cluster_vectors(x, ctype, metric, engine=engine, **kw)
    assert CC.same_partition(labels, c["speakers"])
    shuffled = np.random.default_rng(9).permutation(c["speakers"])
    fit, fit_metric = (stats._unit_rows(x), "euclidean") if (ctype, metric) == ("hdbscan", "cosine") else (x, metric)
    other = CL.silhouette_score(fit, shuffled, fit_metric, plda=c["model"], engine=engine)
    print(f"{ctype} {metric}: true speakers {score:.6f}, shuffled {other:.6f}")
    assert score > other


def test_kalpy_layer(engine, monkeypatch):
    monkeypatch.setattr(K, "_ENGINE", engine)
    c = CC.corpus()
    x = vectors(engine, c, "plda")
    plda = K.Plda(c["model"])
    labels, score = K.cluster_vectors(x, K.ClusterType.hdbscan, K.DistanceMetric.plda, plda=plda, distance_threshold=c["eps"]["plda"],
                                      min_cluster_size=CC.MIN_CLUSTER_SIZE)
    assert CC.same_partition(labels, c["speakers"])
    assert score == K.silhouette_score(x, labels, "plda", plda=plda)
    s = K.silhouette_samples(x, labels, "plda", plda=plda)
    assert s.shape == (x.shape[0],) and score == float(np.mean(s))
    d_labels, d_score = K.cluster_vectors(c["vectors"]["cosine"], K.ClusterType.dbscan, K.DistanceMetric.cosine,
                                          distance_threshold=c["eps"]["cosine"], min_cluster_size=CC.MIN_CLUSTER_SIZE)
    assert CC.same_partition(d_labels, c["speakers"]) and d_score == K.silhouette_score(c["vectors"]["cosine"], d_labels, "cosine")
    with pytest.raises(NotImplementedError, match="kmeans"):
        K.cluster_vectors(x, K.ClusterType.kmeans, K.DistanceMetric.plda, plda=plda)
    with pytest.raises(TypeError, match="n_clusters"):
        K.cluster_vectors(x, K.ClusterType.dbscan, K.DistanceMetric.cosine, n_clusters=3)
    with pytest.raises(ValueError, match="Only found one cluster"):
        K.cluster_vectors(c["vectors"]["euclidean"], K.ClusterType.dbscan, K.DistanceMetric.euclidean, distance_threshold=1e6,
                          min_cluster_size=CC.MIN_CLUSTER_SIZE)
    assert K.cluster_vectors(c["vectors"]["euclidean"], K.ClusterType.dbscan, K.DistanceMetric.euclidean, strict=False, distance_threshold=1e6,
                             min_cluster_size=CC.MIN_CLUSTER_SIZE)[1] is None
