"""The generated speaker corpus of the clustering tests (the recipe of tests/test_gpu_plda_flow.py at a smaller size and a wider
separation), shared by tests/test_cluster_cpu.py — which shows on the CPU that the host reference alone separates the speakers
at the thresholds chosen here — and tests/test_gpu_cluster_flow.py."""
import numpy as np

from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd import stats
from tests import dbscan_ref as R

SPEAKERS, UTTS, D = 12, 8, 16
MIN_CLUSTER_SIZE = 4
_CASE = None


def corpus():
    """dict(model, raw [N, D], vectors {metric: [N, D]}, speakers [N], eps {metric}, dist {metric: direct form [N, N]}): built once.  ε is the middle of the gap
    between the largest within-speaker and the smallest between-speaker distance of the direct form (tests/dbscan_ref.py);
    ``gap`` keeps both ends so that the tests can assert the gap is there."""
    global _CASE
    if _CASE is not None:
        return _CASE
    rng = np.random.default_rng(23)
    frame = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    means = rng.standard_normal((SPEAKERS, D)) * 8.0
    vecs = (means[:, None, :] + rng.standard_normal((SPEAKERS, UTTS, D))) @ frame.T + 5.0
    ivectors = {f"s{s:02d}-u{u}": vecs[s, u] for s in range(SPEAKERS) for u in range(UTTS)}
    utt2spk = {k: k.split("-")[0] for k in ivectors}
    model = P.train_plda({k: v for k, v in ivectors.items() if int(k[-1]) < 4}, utt2spk)
    order = rng.permutation(SPEAKERS * UTTS)              # speakers interleaved: cluster numbers are not speaker numbers
    raw = vecs.reshape(-1, D)[order]
    speakers = np.repeat(np.arange(SPEAKERS), UTTS)[order]
    centred = raw - raw.mean(axis=0)
    vectors = {"plda": stats.plda_transform_host(model, raw), "cosine": centred, "euclidean": raw}
    dist = {"plda": R.plda(model, vectors["plda"], vectors["plda"]), "cosine": R.cosine(centred, centred), "euclidean": R.euclidean(raw, raw)}
    same = speakers[:, None] == speakers[None, :]
    off = ~np.eye(raw.shape[0], dtype=bool)
    gap, eps = {}, {}
    for m, d in dist.items():
        d = np.minimum(d, d.T) if m == "plda" else d        # an edge is a pair that passes in either direction
        gap[m] = (float(d[same & off].max()), float(d[~same].min()))
        eps[m] = 0.5 * (gap[m][0] + gap[m][1])
    _CASE = dict(model=model, raw=raw, vectors=vectors, speakers=speakers, eps=eps, gap=gap, dist=dist, ids=[f"utt{i:03d}" for i in range(raw.shape[0])])
    return _CASE


def same_partition(labels, speakers) -> bool:
    """The clusters are the speakers: no noise, and label ↔ speaker is one to one."""
    labels, speakers = np.asarray(labels), np.asarray(speakers)
    if (labels < 0).any():
        return False
    pairs = set(zip(labels.tolist(), speakers.tolist()))
    return len(pairs) == len(set(labels.tolist())) == len(set(speakers.tolist()))
