"""Speaker clustering: the reference's ``cluster_matrix`` and ``calculate_distance_threshold`` (MFA/diarization/multiprocessing.py)
and the naming of ``SpeakerDiarizer.cluster_utterances`` (MFA/diarization/speaker_diarizer.py), for ``ClusterType.dbscan``.

The device path never stores a distance matrix: the sweep writes the ε-neighbourhoods as a bit matrix (``stats.neighbor_bits``)
and DBSCAN runs on the bits (``stats.dbscan_from_bits``); the threshold estimate takes its k-th neighbour distances from the
sweep's k-nearest consumer.  ``backend="host"`` runs the host twins of the same calls.  What is restated and unpinned:
DESIGN.md, "Clustering".
"""
from __future__ import annotations

import enum
from typing import Dict, Optional, Sequence

import numpy as np

from . import stats


class DistanceMetric(enum.Enum):
    cosine = "cosine"
    plda = "plda"
    euclidean = "euclidean"


class ClusterType(enum.Enum):
    mfa = "mfa"
    affinity = "affinity"
    agglomerative = "agglomerative"
    spectral = "spectral"
    dbscan = "dbscan"
    hdbscan = "hdbscan"
    optics = "optics"
    kmeans = "kmeans"
    meanshift = "meanshift"


UNKNOWN_SPEAKER = "MFA_UNKNOWN"
MAX_NEIGHBOURS = 64          # the k-nearest consumer keeps a row's list in one wavefront register pair


class NoKneeError(ValueError):
    pass


def knee_index(y, S: float = 5.0) -> Optional[int]:
    """Kneedle (Satopää, Albrecht, Irwin, Raghavan 2011) for a concave increasing curve over x = 0, 1, …: the index of the knee,
    or None.  x and y are scaled to [0, 1]; the knee is the first local maximum of the difference curve y − x after which the
    difference falls below (the maximum − S · the mean step of x) before the next local maximum."""
    y = np.asarray(y, dtype=np.float64)
    n = int(y.shape[0])
    if n < 3 or not np.all(np.isfinite(y)):
        return None
    lo, hi = float(y.min()), float(y.max())
    if hi == lo:
        return None
    idx = np.arange(n, dtype=np.float64)
    diff = (y - lo) / (hi - lo) - idx / (n - 1)
    step = 1.0 / (n - 1)
    cand, thr = None, 0.0
    for i in range(1, n - 1):
        if diff[i - 1] < diff[i] >= diff[i + 1]:
            cand, thr = i, diff[i] - S * step
        if cand is not None and diff[i + 1] < thr:
            return cand
    return None


def _model(plda):
    return getattr(plda, "model", plda)


def _metric(metric) -> DistanceMetric:
    return metric if isinstance(metric, DistanceMetric) else DistanceMetric(getattr(metric, "value", metric))


def _engine(engine):
    if engine is not None:
        return engine
    from .kalpy_api import get_engine
    return get_engine()


def _check_backend(backend: str) -> None:
    if backend not in ("device", "host"):
        raise ValueError(f"backend {backend!r}: 'device' or 'host'")


def _vectors(vectors, metric: DistanceMetric, plda) -> np.ndarray:
    x = np.ascontiguousarray(np.atleast_2d(vectors), dtype=np.float64)
    if metric is DistanceMetric.plda:
        if plda is None:
            raise ValueError("the plda metric needs plda=<the model>")
        if x.shape[1] != _model(plda).dim:
            raise ValueError(f"vectors of dimension {x.shape[1]} for a PLDA model of dimension {_model(plda).dim}")
    return x


def kth_neighbor_distances(vectors, metric, k: int, plda=None, backend: str = "device", engine=None) -> np.ndarray:
    """Every point's distance to its ``k``-th nearest other point (1 ≤ k ≤ 64), unsorted."""
    metric = _metric(metric)
    x = _vectors(vectors, metric, plda)
    _check_backend(backend)
    if backend == "host":
        _, score = stats.knn_host(metric.value, x, x, k, _model(plda), exclude_diagonal=True)
    else:
        score = stats.knn(_engine(engine), metric.value, x, x, k, _model(plda), exclude_diagonal=True)[1].cpu().numpy()
    return stats.score_to_distance(metric.value, score[:, k - 1])


def distance_threshold(vectors, metric, min_samples: int, plda=None, backend: str = "device", engine=None, S: float = 5.0) -> float:
    """The reference's ``calculate_distance_threshold``: the knee of the sorted distances to each point's (min_samples − 1)-th other
    neighbour (scikit-learn's ``kneighbors`` on the fitted data counts the point itself first)."""
    k = int(min_samples) - 1
    if k < 1:
        raise ValueError(f"min_samples {min_samples}: the estimate needs a neighbour other than the point itself; pass distance_threshold")
    if k > MAX_NEIGHBOURS:
        raise ValueError(f"min_samples {min_samples}: the estimate keeps at most {MAX_NEIGHBOURS} neighbours a point "
                         f"(min_samples up to {MAX_NEIGHBOURS + 1}); pass distance_threshold")
    d = np.sort(kth_neighbor_distances(vectors, metric, k, plda, backend, engine))
    if d.shape[0] and not np.all(np.isfinite(d)):
        raise NoKneeError(f"a point has fewer than {k} neighbours at a finite distance; pass distance_threshold")
    i = knee_index(d, S)
    if i is None:
        raise NoKneeError("the sorted neighbour distances have no knee; pass distance_threshold")
    return float(d[i])


_estimate_threshold = distance_threshold     # cluster_matrix takes the reference's keyword of the same name


def cluster_matrix(ivectors, cluster_type, metric="cosine", plda=None, distance_threshold=None, min_cluster_size: int = 15,
                   strict: bool = True, backend: str = "device", engine=None, bits=None) -> np.ndarray:
    """The reference's ``cluster_matrix`` for ``ClusterType.dbscan``: the label of every row of ``ivectors`` (−1: noise), clusters
    numbered as scikit-learn numbers them.  ε is ``distance_threshold`` or its estimate; ``min_samples = min_cluster_size``.  For the
    plda metric the vectors are already in the model's space (``stats.plda_transform``) and the distance is −LLR.  ``bits``: a
    neighbour matrix to use in place of the sweep's (tests: the host twin on the device's own bits)."""
    ctype = cluster_type if isinstance(cluster_type, ClusterType) else ClusterType(getattr(cluster_type, "value", cluster_type))
    if ctype is not ClusterType.dbscan:
        raise NotImplementedError(f"The cluster type '{ctype}' is not supported: only {ClusterType.dbscan} is built")
    metric = _metric(metric)
    _check_backend(backend)
    x = _vectors(ivectors, metric, plda)
    if int(min_cluster_size) < 1:
        raise ValueError(f"min_cluster_size {min_cluster_size}: 1 or more")
    if bits is None:
        eps = distance_threshold if distance_threshold is not None else _estimate_threshold(x, metric, min_cluster_size, plda, backend, engine)
        if backend == "host":
            bits = stats.neighbor_bits_host(metric.value, x, x, eps, _model(plda))
        else:
            bits = stats.neighbor_bits(_engine(engine), metric.value, x, x, eps, _model(plda))
    if backend == "host":
        labels = stats.dbscan_from_bits_host(bits, int(min_cluster_size), x.shape[0])["labels"]
    else:
        labels = stats.dbscan_from_bits(_engine(engine), bits, int(min_cluster_size), x.shape[0])["labels"].cpu().numpy()
    if strict and np.unique(labels).shape[0] == 1:
        raise ValueError("Only found one cluster, please adjust cluster parameters to generate more clusters.")
    return labels.astype(np.int64)


def speaker_names(labels) -> list:
    """``Cluster <n>`` for a label ≥ 0, ``MFA_UNKNOWN`` for noise (SpeakerDiarizer.cluster_utterances)."""
    return [f"Cluster {int(c)}" if c >= 0 else UNKNOWN_SPEAKER for c in labels]


def cluster_utterances(utterance_ids: Sequence, ivectors, cluster_type=ClusterType.dbscan, **kwargs) -> Dict:
    """{utterance: speaker name} for the utterances' vectors; ``kwargs`` go to ``cluster_matrix``."""
    utterance_ids = list(utterance_ids)
    x = np.atleast_2d(ivectors)
    if len(utterance_ids) != x.shape[0]:
        raise ValueError(f"{len(utterance_ids)} utterances for {x.shape[0]} vectors")
    return dict(zip(utterance_ids, speaker_names(cluster_matrix(x, cluster_type, **kwargs))))


def hdbscan_matrix(ivectors, metric="cosine", plda=None, distance_threshold=None, min_cluster_size: int = 15, min_samples=None,
                   strict: bool = True, backend: str = "device", engine=None, edges=None) -> np.ndarray:
    """What the reference's ``cluster_matrix`` asks of HDBSCAN for ``ClusterType.hdbscan``: the label of every row of ``ivectors`` (−1:
    noise), clusters numbered by their smallest member.  ``min_samples`` defaults to ``max(5, min_cluster_size // 4)`` and
    ``cluster_selection_epsilon`` is ``distance_threshold`` or its estimate at ``min_cluster_size``, the reference's rules; cosine is
    euclidean on unit rows, as there, and so is its threshold.  The device computes the core scores and the minimum spanning tree
    of the mutual-reachability graph (``stats.core_scores``, ``stats.mreach_mst``) with no N × N array; the cluster tree on the
    N − 1 edges is host work (``hdbscan.cluster_tree_labels``).  For the plda metric the vectors are already in the model's space and
    the distance is −LLR, measured in the cluster tree from the spanning tree's smallest edge (ε is on the −LLR scale).  ``edges``: a spanning tree (lo, hi, score) to use in place of the sweep's (tests: the host path on the
    device's own edges).  ``cluster_matrix(…, ClusterType.hdbscan)`` does not route here yet."""
    from . import hdbscan as _hdbscan
    metric = _metric(metric)
    _check_backend(backend)
    x = _vectors(ivectors, metric, plda)
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size {min_cluster_size}: 2 or more")
    if min_samples is None:
        min_samples = max(5, int(min_cluster_size) // 4)
    k = int(min_samples) - 1
    if k < 0 or k > MAX_NEIGHBOURS:
        raise ValueError(f"min_samples {min_samples}: 1 to {MAX_NEIGHBOURS + 1} (the core distance keeps at most {MAX_NEIGHBOURS} "
                         "neighbours a point)")
    _, unit, dist_metric = stats.pair_metric(metric.value)
    if unit:
        x = np.ascontiguousarray(stats._unit_rows(x))
    fit_metric = DistanceMetric(dist_metric)
    eps = distance_threshold if distance_threshold is not None else _estimate_threshold(x, fit_metric, min_cluster_size, plda, backend, engine)
    n = x.shape[0]
    if edges is None:
        if backend == "host":
            pf = stats.core_scores_host(dist_metric, x, k, _model(plda))
            edges = stats.mreach_mst_host(dist_metric, pf["y"], pf["q"], pf["core"])
        else:
            pf = stats.core_scores(_engine(engine), dist_metric, x, k, _model(plda))
            edges = stats.mreach_mst(_engine(engine), dist_metric, pf["y"], pf["q"], pf["core"])
    lo, hi, score = (edges["lo"], edges["hi"], edges["score"]) if isinstance(edges, dict) else edges
    dist, eps = stats.score_to_distance(dist_metric, score), float(eps)
    if metric is DistanceMetric.plda and np.isfinite(dist).any():
        # −LLR is a signed distance (on a corpus whose speakers the model knows every pair's can be negative), and λ = 1 / d needs
        # one that is not: the tree's distances, and ε with them, are measured from its smallest edge.  The hierarchy does not
        # depend on the zero point; the λ do, and this choice makes the labels a function of LLR differences alone.
        d0 = float(dist[np.isfinite(dist)].min())
        dist, eps = dist - d0, eps - d0
    labels = _hdbscan.cluster_tree_labels(n, lo, hi, dist, int(min_cluster_size), eps)
    if strict and np.unique(labels).shape[0] == 1:
        raise ValueError("Only found one cluster, please adjust cluster parameters to generate more clusters.")
    return labels.astype(np.int64)


def hdbscan_utterances(utterance_ids: Sequence, ivectors, **kwargs) -> Dict:
    """{utterance: speaker name} from ``hdbscan_matrix``; ``kwargs`` go to it."""
    utterance_ids = list(utterance_ids)
    x = np.atleast_2d(ivectors)
    if len(utterance_ids) != x.shape[0]:
        raise ValueError(f"{len(utterance_ids)} utterances for {x.shape[0]} vectors")
    return dict(zip(utterance_ids, speaker_names(hdbscan_matrix(x, **kwargs))))


__all__ = ["ClusterType", "DistanceMetric", "NoKneeError", "cluster_matrix", "cluster_utterances", "distance_threshold", "hdbscan_matrix",
           "hdbscan_utterances", "knee_index", "kth_neighbor_distances", "speaker_names"]
