"""A longdouble restatement of the silhouette stage's contract (include/mfa_hip.h "Silhouette"), for tests/test_silhouette_cpu.py
and tests/test_gpu_silhouette*.py: the distances computed directly from the vectors (‖x_i − x_j‖, not the expanded form the
sweep sums), the cluster means, the coefficient, and a per-row bound on |s − s_ref| that is derived, not measured.

The bound, for a row i, from the inside out.  Nothing here is taken from what the code returns.
  score     |v − v_real| ≤ δv = hdbscan_ref.pair_bound (each form is within that of the real number).
  distance  plda d = −v and dot d = 1 − v: δd = δv + u |d| (the subtraction's rounding).  euclidean d = √m, m = max(−v, 0), with
            |m − d_ref²| ≤ δv:  where d_ref² > δv,  |√m − d_ref| = |m − d_ref²| / (√m + d_ref) ≤ δv / (d_ref + √(d_ref² − δv)), which is
            δv / (2 d) to first order;  where d_ref² ≤ δv,  m lies in [0, 2 δv] and |√m − d_ref| ≤ √δv.  The root adds ULP_ROOT u d
            (1: correctly rounded; the tests that allow the device's root 1 ulp pass 2).
  sums      S = Σ d over n terms in some order: δS = Σ δd + γ_n Σ (|d| + δd)  (Higham §4.2: any order of a recursive sum).
  means     a = S / (n − 1), m_c = S_c / n_c: δ = δS / count + u (|mean| + δS / count).  b is a minimum: |min_c m_c − min_c m_ref,c| ≤
            max_c δm_c over the other clusters.
  quotient  s = (b − a) / den, den = max(a, b):  with e = δa + δb, |num − num_ref| ≤ e and |den − den_ref| ≤ e, so
            |s − s_ref| ≤ e (1 + |s_ref|) / (|den_ref| − e) + 3 u (1 + |s_ref|)   (the subtraction, the division; inf where |den_ref| ≤ e).
  A singleton scores 0 on both sides: bound 0.
"""
import numpy as np

from tests import hdbscan_ref as H

U = H.U
LD = np.longdouble


def sort_by_label(labels):
    """(order, offsets): a stable sort of the points by label and the clusters' ranges in it."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    counts = np.unique(labels, return_counts=True)[1]
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def distances(metric, x, psi=None):
    """d [n, n] in longdouble from the definition: euclidean ‖x_i − x_j‖ computed directly, dot 1 − x_i·x_j, plda −LLR of the pair
    form with its coefficients in longdouble."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    if metric == "euclidean":
        diff = x[:, None, :] - x[None, :, :]
        return np.sqrt((diff * diff).sum(axis=2))
    if metric == "dot":
        return LD(1) - x @ x.T
    psi = np.asarray(psi, dtype=np.float64).astype(LD)
    a, b = psi * psi / ((psi + 1) * (2 * psi + 1)), psi / (2 * psi + 1)
    c = (np.log((1 + psi) ** 2 / (2 * psi + 1))).sum() / 2
    q = c / 2 - ((x * x) * a[None, :]).sum(axis=1) / 2
    return -((q[:, None] + q[None, :]) + (x * b[None, :]) @ x.T)


def samples(d, offsets):
    """dict(s, a, b, bj, den: longdouble / int [n]; S, n: the cluster sums [n, C] and sizes [C]) for rows ordered by cluster."""
    d = np.array(d, dtype=LD)
    n, C = d.shape[0], len(offsets) - 1
    np.fill_diagonal(d, 0)                                            # the diagonal never enters a sum
    sizes = np.diff(np.asarray(offsets, dtype=np.int64))
    own = np.repeat(np.arange(C), sizes)
    S = np.stack([d[:, offsets[c]: offsets[c + 1]].sum(axis=1) for c in range(C)], axis=1)
    rows = np.arange(n)
    n_own = sizes[own]
    a = np.where(n_own > 1, S[rows, own] / np.maximum(n_own - 1, 1).astype(LD), LD(0))
    means = S / sizes[None, :].astype(LD)
    means[rows, own] = np.inf
    bj = np.argmin(means, axis=1)                                     # the first of equal ones: the lower cluster
    b = means[rows, bj]
    den = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(n_own == 1, LD(0), np.where(den == 0, LD(0), (b - a) / den))
    return dict(s=s, a=a, b=b, bj=bj.astype(np.int32), den=den, S=S, sizes=sizes, own=own)


def distance_bound(metric, x, psi, d_ref, ulp_root: int = 1):
    """δd [n, n] (float64) from δv = hdbscan_ref.pair_bound."""
    dv = H.pair_bound(metric, x, psi)
    d = np.abs(np.asarray(d_ref, dtype=np.float64))
    if metric != "euclidean":
        return dv + U * (d + dv)
    far = d * d > dv
    with np.errstate(invalid="ignore", divide="ignore"):
        through = np.where(far, dv / (d + np.sqrt(np.maximum(d * d - dv, 0.0))), np.sqrt(dv))
    return through + ulp_root * U * (d + through)


def bound(metric, x, offsets, psi=None, ulp_root: int = 1, from_smallest: bool = False):
    """The per-row bound on |s − s_ref| for rows ordered by cluster, and the restatement it belongs to: (bound [n] float64, ref).
    ``from_smallest``: the cluster layer's plda rule — the distances measured from the smallest one between two points, d0.  The
    restatement is then the plain one on d − d0.  The code sums the unshifted d and moves a and b by −d0 afterwards, so its sums
    round at the unshifted magnitudes (|d| + |d − d0| covers both), d0 itself is off by at most the largest δd, which every
    shifted distance inherits, and the moved denominator is one more rounding."""
    d_ref = distances(metric, x, psi)
    dd = distance_bound(metric, x, psi, d_ref, ulp_root)
    if not from_smallest:
        return propagate(dd, d_ref, samples(d_ref, offsets), offsets), samples(d_ref, offsets)
    off = ~np.eye(d_ref.shape[0], dtype=bool)
    shifted = d_ref - d_ref[off].min()
    ref = samples(shifted, offsets)
    return propagate(dd + dd[off].max(), np.abs(d_ref) + np.abs(shifted), ref, offsets, roundings=4), ref


def root_bound(d, offsets, ulps: int = 1):
    """The bound between two runs of the contract on the same stored scores whose roots differ by at most ``ulps`` units in the last
    place (2 u relative each): δd = ulps · 2 u · d, and both sides round their own sums (``sums=2``).  ``d``: the distances of one side."""
    d = np.asarray(d, dtype=np.float64)
    return propagate(ulps * 2 * U * np.abs(d), d, samples(d, offsets), offsets, sums=2)


def propagate(dd, d_ref, ref, offsets, sums: int = 1, roundings: int = 3):
    """δd [n, n] through the sums, the means and the quotient (the module's docstring): the bound on |s − s_ref| per row."""
    dd = np.array(dd, dtype=np.float64)
    np.fill_diagonal(dd, 0.0)
    absd = np.abs(np.asarray(d_ref, dtype=np.float64))
    np.fill_diagonal(absd, 0.0)
    n, C = absd.shape[0], len(offsets) - 1
    sizes, own, rows = ref["sizes"], ref["own"], np.arange(absd.shape[0])
    dS = np.stack([dd[:, offsets[c]: offsets[c + 1]].sum(axis=1) + sums * H.gamma(int(sizes[c])) * (absd + dd)[:, offsets[c]: offsets[c + 1]].sum(axis=1)
                   for c in range(C)], axis=1)
    count = np.tile(sizes[None, :].astype(np.float64), (n, 1))
    count[rows, own] = np.maximum(sizes[own] - 1, 1)
    mean_abs = np.stack([absd[:, offsets[c]: offsets[c + 1]].sum(axis=1) for c in range(C)], axis=1) / count   # >= |mean|
    dm = dS / count + sums * U * (mean_abs + dS / count)
    da = dm[rows, own]
    other = dm.copy()
    other[rows, own] = 0.0
    e = da + other.max(axis=1)
    s_abs, den_abs = np.abs(np.asarray(ref["s"], dtype=np.float64)), np.abs(np.asarray(ref["den"], dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den_abs > e, e * (1 + s_abs) / (den_abs - e) + roundings * sums * U * (1 + s_abs), np.inf)
    return np.where(sizes[own] == 1, 0.0, out)


# ---- the exact tier's cluster layouts: offsets [C + 1] for n points ------------------------------------------------------------------
def layouts(n: int):
    """{name: offsets} of the cluster layouts that fit ``n`` points: the boundaries at which the consumer changes path."""
    out = {}
    if n >= 2:
        out["two"] = [0, n // 2, n]
    if n >= 3:
        out["singletons_but_a_pair"] = [0, 2] + list(range(3, n + 1))
    if n >= 66:
        out["boundary_at_64"] = [0, 64, n]
        out["singletons_at_63_and_64"] = [0, 63, 64, 65, n]
    if n >= 200:
        out["three_steps"] = [0, 20, 190, n]                          # a cluster that begins in step 0 and ends in step 2
    if n >= 40:
        out["many_in_one_step"] = list(range(0, 36, 2)) + [n]         # 17 clusters of 2 inside the first step, the rest one cluster
    return {k: np.asarray(v, dtype=np.int32) for k, v in out.items()}


def random_labels(n: int, clusters: int, seed: int, noise: int = 0, singleton: bool = False):
    """Arbitrary integer labels in a random order: ``clusters`` labels drawn from 3, 13, 23, …, ``noise`` points labelled −1, and one
    point with a label of its own."""
    rng = np.random.default_rng(seed)
    labels = 3 + 10 * rng.integers(0, clusters, n)
    labels[: 2 * clusters] = 3 + 10 * np.repeat(np.arange(clusters), 2)                    # no label stays empty
    labels = rng.permutation(labels)
    if noise:
        labels[rng.choice(n, noise, replace=False)] = -1
    if singleton:
        labels[int(np.flatnonzero(labels != -1)[0])] = 1000
    return labels
