"""Speaker clustering end to end on the generated corpus of tests/cluster_case.py (12 speakers × 8 utterances, D = 16, in random
order): train PLDA → transform on the device → ``cluster_matrix(dbscan)`` on the device, against ``backend="host"`` given the
device's own bits, for plda, cosine and euclidean; the clusters are the speakers (tests/test_cluster_cpu.py shows that the host
reference alone achieves that at these thresholds); the automatic threshold; the kalpy-layer call; the speaker names."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import kalpy_api as K
from montreal_forced_aligner_amd import stats
from tests import cluster_case as CC
from tests import dbscan_ref as R

pytestmark = pytest.mark.gpu

METRICS = ("plda", "cosine", "euclidean")


def device_vectors(engine, c, metric):
    """The corpus in the metric's space; for plda through the device's transform."""
    if metric != "plda":
        return c["vectors"][metric]
    v = stats.plda_transform(engine, c["model"], c["raw"]).cpu().numpy()
    np.testing.assert_allclose(v, c["vectors"]["plda"], rtol=1e-11, atol=1e-12)
    return v


@pytest.mark.parametrize("metric", METRICS)
def test_device_clusters_equal_the_host_on_the_same_bits_and_the_speakers(engine, metric):
    c = CC.corpus()
    x = device_vectors(engine, c, metric)
    kw = dict(plda=c["model"], distance_threshold=c["eps"][metric], min_cluster_size=CC.MIN_CLUSTER_SIZE)
    dev = CL.cluster_matrix(x, CL.ClusterType.dbscan, metric, engine=engine, **kw)
    bits = stats.neighbor_bits(engine, metric, x, x, c["eps"][metric], c["model"])
    host = CL.cluster_matrix(x, CL.ClusterType.dbscan, metric, backend="host", bits=bits.cpu().numpy(), **kw)
    assert np.array_equal(dev, host)
    assert CC.same_partition(dev, c["speakers"])
    # no distance of the direct form is within 1e-6 of ε (tests/test_cluster_cpu.py), so the device's bits are its, pair for pair
    direct = {"plda": lambda: R.plda(c["model"], x, x), "cosine": lambda: R.cosine(x, x), "euclidean": lambda: R.euclidean(x, x)}[metric]()
    assert np.array_equal(R.unpack(bits.cpu().numpy(), x.shape[0]), direct <= c["eps"][metric])
    assert np.array_equal(dev, CL.cluster_matrix(x, "dbscan", metric, backend="host", **kw))


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_automatic_threshold(engine, metric):
    c = CC.corpus()
    x = c["vectors"][metric]
    eps = CL.distance_threshold(x, metric, CC.MIN_CLUSTER_SIZE, engine=engine)
    assert eps == pytest.approx(CL.distance_threshold(x, metric, CC.MIN_CLUSTER_SIZE, backend="host"), rel=1e-9)
    d = {"cosine": R.cosine, "euclidean": R.euclidean}[metric](x, x)
    np.fill_diagonal(d, np.inf)
    kth = np.sort(np.sort(d, axis=1)[:, CC.MIN_CLUSTER_SIZE - 2])
    assert eps == pytest.approx(kth[CL.knee_index(kth)], rel=1e-9)
    auto = CL.cluster_matrix(x, "dbscan", metric, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, engine=engine)
    given = CL.cluster_matrix(x, "dbscan", metric, distance_threshold=eps, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, engine=engine)
    assert np.array_equal(auto, given)
    bits = stats.neighbor_bits(engine, metric, x, x, eps)
    host = CL.cluster_matrix(x, "dbscan", metric, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, backend="host", bits=bits.cpu().numpy())
    assert np.array_equal(auto, host)


def test_plda_threshold_estimate_device_equals_host(engine):
    c = CC.corpus()
    x = c["vectors"]["plda"]
    k = CC.MIN_CLUSTER_SIZE - 1
    dev = np.sort(CL.kth_neighbor_distances(x, "plda", k, plda=c["model"], engine=engine))
    host = np.sort(CL.kth_neighbor_distances(x, "plda", k, plda=c["model"], backend="host"))
    np.testing.assert_allclose(dev, host, rtol=1e-10, atol=1e-10)
    d = R.plda(c["model"], x, x)
    np.fill_diagonal(d, np.inf)
    np.testing.assert_allclose(dev, np.sort(np.sort(d, axis=1)[:, k - 1]), rtol=1e-9, atol=1e-9)


def test_kalpy_layer_and_speaker_names(engine, monkeypatch):
    monkeypatch.setattr(K, "_ENGINE", engine)
    c = CC.corpus()
    x = device_vectors(engine, c, "plda")
    labels = K.cluster_matrix(x, K.ClusterType.dbscan, K.DistanceMetric.plda, plda=K.Plda(c["model"]), distance_threshold=c["eps"]["plda"],
                              min_cluster_size=CC.MIN_CLUSTER_SIZE)
    assert CC.same_partition(labels, c["speakers"])
    with pytest.raises(NotImplementedError, match="hdbscan"):
        K.cluster_matrix(x, K.ClusterType.hdbscan, K.DistanceMetric.plda, plda=K.Plda(c["model"]))
    with pytest.raises(TypeError, match="n_clusters"):
        K.cluster_matrix(x, K.ClusterType.dbscan, K.DistanceMetric.cosine, n_clusters=3)
    names = CL.cluster_utterances(c["ids"], c["vectors"]["euclidean"], metric="euclidean", distance_threshold=c["eps"]["euclidean"],
                                  min_cluster_size=CC.MIN_CLUSTER_SIZE, engine=engine)
    assert [names[u] for u in c["ids"]] == [f"Cluster {l}" for l in labels]       # the same partition, numbered the same way
    out = np.concatenate([c["vectors"]["euclidean"], c["vectors"]["euclidean"].mean(axis=0, keepdims=True) + 500.0])
    names = CL.cluster_utterances(c["ids"] + ["stray"], out, metric="euclidean", distance_threshold=c["eps"]["euclidean"],
                                  min_cluster_size=CC.MIN_CLUSTER_SIZE, engine=engine)
    assert names["stray"] == "MFA_UNKNOWN" and sorted(set(names.values()))[-1] == "MFA_UNKNOWN"
