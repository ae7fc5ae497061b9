"""HDBSCAN end to end on the generated corpus of tests/cluster_case.py (12 speakers × 8 utterances, D = 16, in random order): train
PLDA → transform on the device → ``hdbscan_matrix`` on the device, against ``backend="host"`` given the device's own edges, for
plda, cosine and euclidean; the clusters are the speakers; the automatic threshold; the kalpy-layer call; the speaker names."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import kalpy_api as K
from montreal_forced_aligner_amd import stats
from tests import cluster_case as CC

pytestmark = pytest.mark.gpu

METRICS = ("plda", "cosine", "euclidean")


def threshold(c, metric):
    """The corpus's ε in the distance HDBSCAN clusters on: cosine is euclidean on unit rows, |u − v|² = 2 (1 − cos)."""
    return float(np.sqrt(2.0 * c["eps"]["cosine"])) if metric == "cosine" else c["eps"][metric]


def device_edges(engine, c, metric, x, min_samples):
    _, unit, dm = stats.pair_metric(metric)
    pf = stats.core_scores(engine, metric, x, min_samples - 1, c["model"])
    return stats.mreach_mst(engine, dm, pf["y"], pf["q"], pf["core"])


@pytest.mark.parametrize("metric", METRICS)
def test_device_clusters_equal_the_host_on_the_same_edges_and_the_speakers(engine, metric):
    c = CC.corpus()
    x = stats.plda_transform(engine, c["model"], c["raw"]).cpu().numpy() if metric == "plda" else c["vectors"][metric]
    kw = dict(plda=c["model"], distance_threshold=threshold(c, metric), min_cluster_size=CC.MIN_CLUSTER_SIZE)
    dev = CL.hdbscan_matrix(x, metric, engine=engine, **kw)
    edges = device_edges(engine, c, metric, x, 5)                            # min_samples = max(5, 4 // 4)
    assert edges["found"] == x.shape[0] - 1
    host = CL.hdbscan_matrix(x, metric, backend="host", edges=edges, **kw)
    assert np.array_equal(dev, host)
    assert CC.same_partition(dev, c["speakers"])
    assert CC.same_partition(CL.hdbscan_matrix(x, metric, backend="host", **kw), c["speakers"])     # the host twins end to end


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_automatic_threshold(engine, metric):
    c = CC.corpus()
    x = c["vectors"][metric]
    fit = stats._unit_rows(x) if metric == "cosine" else x
    eps = CL.distance_threshold(fit, "euclidean", CC.MIN_CLUSTER_SIZE, engine=engine)
    auto = CL.hdbscan_matrix(x, metric, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, engine=engine)
    given = CL.hdbscan_matrix(x, metric, distance_threshold=eps, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, engine=engine)
    assert np.array_equal(auto, given)
    host = CL.hdbscan_matrix(x, metric, distance_threshold=eps, min_cluster_size=CC.MIN_CLUSTER_SIZE, strict=False, backend="host",
                             edges=device_edges(engine, c, metric, x, 5))
    assert np.array_equal(auto, host)


def test_kalpy_layer_and_speaker_names(engine, monkeypatch):
    monkeypatch.setattr(K, "_ENGINE", engine)
    c = CC.corpus()
    x = stats.plda_transform(engine, c["model"], c["raw"]).cpu().numpy()
    labels = K.hdbscan_matrix(x, K.DistanceMetric.plda, plda=K.Plda(c["model"]), distance_threshold=c["eps"]["plda"],
                              min_cluster_size=CC.MIN_CLUSTER_SIZE)
    assert CC.same_partition(labels, c["speakers"])
    with pytest.raises(NotImplementedError, match="hdbscan"):               # cluster_matrix does not route here yet
        K.cluster_matrix(x, K.ClusterType.hdbscan, K.DistanceMetric.plda, plda=K.Plda(c["model"]))
    with pytest.raises(TypeError, match="n_clusters"):
        K.hdbscan_matrix(x, K.DistanceMetric.cosine, n_clusters=3)
    kw = dict(metric="euclidean", distance_threshold=c["eps"]["euclidean"], min_cluster_size=CC.MIN_CLUSTER_SIZE, engine=engine)
    names = CL.hdbscan_utterances(c["ids"], c["vectors"]["euclidean"], **kw)
    assert [names[u] for u in c["ids"]] == [f"Cluster {l}" for l in labels]       # the same partition, numbered the same way
    out = np.concatenate([c["vectors"]["euclidean"], c["vectors"]["euclidean"].mean(axis=0, keepdims=True) + 500.0])
    names = CL.hdbscan_utterances(c["ids"] + ["stray"], out, **kw)
    assert names["stray"] == "MFA_UNKNOWN" and sorted(set(names.values()))[-1] == "MFA_UNKNOWN"
