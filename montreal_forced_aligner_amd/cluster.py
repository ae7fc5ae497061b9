"""Speaker clustering: the reference's ``cluster_matrix`` and ``calculate_distance_threshold`` (MFA/diarization/multiprocessing.py)
and the naming of ``SpeakerDiarizer.cluster_utterances`` (MFA/diarization/speaker_diarizer.py), for ``ClusterType.dbscan``.

The device path never stores a distance matrix: the sweep writes the ε-neighbourhoods as a bit matrix (``stats.neighbor_bits``)
and DBSCAN runs on the bits (``stats.dbscan_from_bits``); the threshold estimate takes its k-th neighbour distances from the
sweep's k-nearest consumer.  ``hdbscan_matrix`` is the ``ClusterType.hdbscan`` branch; ``cluster_vectors`` runs either type and then,
as the reference does after every clustering, the silhouette score (``silhouette_samples``: the cluster sums come out of one more
sweep over the points ordered by label).  ``backend="host"`` runs the host twins of the same calls.  What is restated and
unpinned: DESIGN.md, "Clustering", "HDBSCAN", "Silhouette".
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


ONE_CLUSTER = "Only found one cluster, please adjust cluster parameters to generate more clusters."


def silhouette_from_means(a, b, n_own, shift: float = 0.0) -> np.ndarray:
    """The coefficients from every point's a and b (``stats.silhouette(…, want_parts=True)``) with every distance moved by
    ``shift``: a singleton scores 0; den = max(a, b) + shift, den == 0 scores 0, any other den (b − a) / den."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.where(a < b, b, a) + float(shift)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((np.asarray(n_own) == 1) | (den == 0.0), 0.0, (b - a) / den)


def _silhouette(vectors, labels, metric, plda, noise: str, backend: str, engine):
    """(the coefficients [n] in the caller's order, NaN for a row that was left out; the rows that took part)."""
    metric = _metric(metric)
    _check_backend(backend)
    if noise not in ("cluster", "exclude"):
        raise ValueError(f"noise {noise!r}: 'cluster' (label -1 is one more cluster) or 'exclude'")
    x = _vectors(vectors, metric, plda)
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != x.shape[0]:
        raise ValueError(f"{labels.shape} labels for {x.shape[0]} vectors")
    if labels.shape[0] and not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"labels of type {labels.dtype}: integers")
    if not np.isfinite(x).all():
        raise ValueError("vectors that are not finite")
    keep = np.flatnonzero(labels != -1) if noise == "exclude" else np.arange(labels.shape[0])
    n = int(keep.shape[0])
    counts = np.unique(labels[keep], return_counts=True)[1]
    if not 2 <= counts.shape[0] <= n - 1:
        raise ValueError(f"Number of labels is {counts.shape[0]}. Valid values are 2 to n_samples - 1 (inclusive): {n} samples")
    order = keep[np.argsort(labels[keep], kind="stable")]          # the points by label: every cluster one range of rows
    offsets = np.concatenate([[0], np.cumsum(counts)])
    xs, name = x[order], metric.value
    if metric is DistanceMetric.cosine:                            # the cosine distance: 1 − dot on unit rows
        xs, name = np.ascontiguousarray(stats._unit_rows(xs)), "dot"
    parts = metric is DistanceMetric.plda
    if backend == "host":
        r = stats.silhouette_host(name, xs, offsets, _model(plda), want_parts=parts)
        best = stats.core_scores_host(name, xs, 1, _model(plda))["core"] if parts else None
    else:
        r = {k: (v.cpu().numpy() if k in ("sil", "a", "b") and v is not None else v)
             for k, v in stats.silhouette(_engine(engine), name, xs, offsets, _model(plda), want_parts=parts).items()}
        best = stats.core_scores(_engine(engine), name, xs, 1, _model(plda))["core"].cpu().numpy() if parts else None
    sil = r["sil"]
    if parts:
        # −LLR is a signed distance, and (b − a) / max(a, b) ranks clusterings only for one that is never negative (with a and b both
        # negative the quotient changes sign exactly where the clustering is right).  As in hdbscan_matrix, the plda distances are
        # measured from the smallest one between two points: a mean of d − d0 is the mean of d less d0, so a and b move by −d0, the
        # cluster that gives b stays, and only the denominator changes.
        d0 = -float(np.max(best))
        sil = silhouette_from_means(r["a"], r["b"], np.repeat(counts, counts), -d0)
    out = np.full(labels.shape[0], np.nan)
    out[order] = sil
    return out, keep


def silhouette_samples(vectors, labels, metric="cosine", plda=None, noise: str = "cluster", backend: str = "device", engine=None) -> np.ndarray:
    """scikit-learn's ``silhouette_samples(vectors, labels, metric=metric)``: every point's (b − a) / max(a, b), a the mean distance
    to the other points of its cluster and b the least mean distance to another cluster; a cluster of one scores 0.  ``labels`` are
    arbitrary integers.  ``noise="cluster"`` is scikit-learn's and the reference's rule: label −1 is one more cluster;
    ``noise="exclude"`` leaves those rows out and returns NaN for them.  ``cosine`` is 1 − dot on unit rows; for the plda metric
    the vectors are already in the model's space and the distance is −LLR measured from the smallest one between two of the points
    (−LLR is signed, and the quotient ranks clusterings only for a distance that is never negative; one more sweep finds that
    pair, and a and b move by the same amount: ``silhouette_from_means``).  The device
    sums every cluster's distances inside the pair sweep (``stats.silhouette``): no N × N array.  Fewer than 2 labels, more than
    N − 1, vectors that are not finite and a length mismatch raise ``ValueError``."""
    return _silhouette(vectors, labels, metric, plda, noise, backend, engine)[0]


def silhouette_score(vectors, labels, metric="cosine", plda=None, noise: str = "cluster", backend: str = "device", engine=None) -> float:
    """The mean of ``silhouette_samples`` over the rows that took part (the reference's ``metrics.silhouette_score``), on the host."""
    s, keep = _silhouette(vectors, labels, metric, plda, noise, backend, engine)
    return float(np.mean(s[keep]))


def cluster_vectors(ivectors, cluster_type, metric="cosine", plda=None, strict: bool = True, backend: str = "device", engine=None, **kwargs):
    """The reference's ``cluster_matrix`` to its end for the two cluster types that are built: (labels, silhouette score).
    ``ClusterType.dbscan`` goes to ``cluster_matrix`` and ``ClusterType.hdbscan`` to ``hdbscan_matrix`` with ``kwargs``; the score
    then follows the reference's ``score_metric``: hdbscan with cosine scores euclidean distances on unit rows, dbscan with cosine
    cosine distances, plda −LLR (from its smallest value: ``silhouette_samples``), label −1 one more cluster.  One label raises the reference's ``ValueError`` under ``strict`` and
    gives ``score = None`` without; as many labels as points give ``score = None``."""
    ctype = cluster_type if isinstance(cluster_type, ClusterType) else ClusterType(getattr(cluster_type, "value", cluster_type))
    metric = _metric(metric)
    if ctype is ClusterType.dbscan:
        labels = cluster_matrix(ivectors, ctype, metric, plda=plda, strict=False, backend=backend, engine=engine, **kwargs)
    elif ctype is ClusterType.hdbscan:
        labels = hdbscan_matrix(ivectors, metric, plda=plda, strict=False, backend=backend, engine=engine, **kwargs)
    else:
        raise NotImplementedError(f"The cluster type '{ctype}' is not supported: {ClusterType.dbscan} and {ClusterType.hdbscan} are built")
    found = np.unique(labels).shape[0]
    if found == 1 and strict:
        raise ValueError(ONE_CLUSTER)
    if not 2 <= found <= labels.shape[0] - 1:
        return labels, None
    to_fit, score_metric = _vectors(ivectors, metric, plda), metric
    if ctype is ClusterType.hdbscan and metric is DistanceMetric.cosine:
        to_fit, score_metric = np.ascontiguousarray(stats._unit_rows(to_fit)), DistanceMetric.euclidean
    return labels, silhouette_score(to_fit, labels, score_metric, plda, "cluster", backend, engine)


def cluster_vectors_utterances(utterance_ids: Sequence, ivectors, cluster_type=ClusterType.dbscan, **kwargs):
    """({utterance: speaker name}, silhouette score) from ``cluster_vectors``; ``kwargs`` go to it."""
    utterance_ids = list(utterance_ids)
    x = np.atleast_2d(ivectors)
    if len(utterance_ids) != x.shape[0]:
        raise ValueError(f"{len(utterance_ids)} utterances for {x.shape[0]} vectors")
    labels, score = cluster_vectors(x, cluster_type, **kwargs)
    return dict(zip(utterance_ids, speaker_names(labels))), score


__all__ = ["ClusterType", "DistanceMetric", "NoKneeError", "cluster_matrix", "cluster_utterances", "cluster_vectors",
           "cluster_vectors_utterances", "distance_threshold", "hdbscan_matrix", "hdbscan_utterances", "knee_index", "kth_neighbor_distances",
           "silhouette_from_means", "silhouette_samples", "silhouette_score", "speaker_names"]
