"""The LDA estimate from scatter statistics: what ``est-lda`` makes of ``acc-lda``'s sums (the reference's
``LdaStatsAccumulator.lda.estimate``, MFA/acoustic_modeling/lda.py:352-373), in float64 numpy.  Restated from the algorithm's
description — Kaldi's source is not among this project's references: parity unpinned.

With N = Σ zero and m = Σ_c first[c] / N:

  total   = second / N − m mᵀ
  between = Σ_{c: zero[c] ≠ 0} first[c] first[c]ᵀ / zero[c] / N − m mᵀ
  within  = total − between,  L = Cholesky(within),  P = L⁻¹
  P·between·Pᵀ = Q·diag(s)·Qᵀ with s descending;  full = Qᵀ·P

so that full·within·fullᵀ = I and full·between·fullᵀ = diag(s).  Every row's sign is then fixed (its largest-magnitude entry
is positive: the matrix is a function of the statistics), ``remove_offset`` appends the column −full·m, and the LDA matrix is
the first ``dim`` rows.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .stats import LdaStats


def scatter_matrices(stats: LdaStats) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """(N, mean [S], within [S, S], between [S, S]) of the statistics, float64, both matrices symmetrised."""
    zero = np.asarray(stats.zero, dtype=np.float64)
    first = np.asarray(stats.first, dtype=np.float64)
    second = np.asarray(stats.second, dtype=np.float64)
    N = float(zero.sum())
    if not N > 0:
        raise ValueError(f"estimate_lda: the statistics hold no frames (total weight {N})")
    m = first.sum(axis=0) / N
    mm = np.outer(m, m)
    total = second / N - mm
    live = zero != 0
    scaled = first[live] / zero[live, None]
    between = (first[live].T @ scaled) / N - mm
    between = 0.5 * (between + between.T)
    within = total - between
    within = 0.5 * (within + within.T)
    return N, m, within, between


def estimate_lda(stats: LdaStats, dim: int = 40, allow_large_dim: bool = False, remove_offset: bool = False):
    """(lda_mat float32 [dim, S(+1)], full float32 [S, S(+1)]) from ``LdaStats``.

    ``ValueError``: no frames; ``dim`` outside 1..S; ``dim`` above the between-class rank (classes with frames − 1) unless
    ``allow_large_dim`` — this project's rule; a within-class covariance that is not positive definite."""
    S = int(stats.first.shape[1])
    dim = int(dim)
    N, m, within, between = scatter_matrices(stats)
    if dim < 1 or dim > S:
        raise ValueError(f"estimate_lda: dim {dim} outside 1..{S} (the spliced dimension)")
    live = int(np.count_nonzero(np.asarray(stats.zero) > 0))
    if dim > live - 1 and not allow_large_dim:
        raise ValueError(f"estimate_lda: dim {dim} above the between-class rank {live - 1} ({live} classes with frames); "
                         "pass allow_large_dim to take the extra rows anyway")
    diag = np.diag(within)
    if not np.all(np.isfinite(within)) or np.any(diag <= 0):
        bad = np.flatnonzero(~(diag > 0))
        raise ValueError("estimate_lda: the within-class covariance is not positive definite: spliced columns "
                         f"{bad[:8].tolist()} have no within-class variance (a constant or muted channel?)")
    try:
        L = np.linalg.cholesky(within)
    except np.linalg.LinAlgError:
        raise ValueError(f"estimate_lda: the within-class covariance is not positive definite (Cholesky failed; {N:.0f} frames "
                         f"for {S} spliced dimensions: too few frames, or linearly dependent columns)") from None
    P = np.linalg.inv(L)
    # the pivots of a numerically singular matrix can come out positive: hold the factor to what it claims
    if not np.all(np.isfinite(P)) or np.linalg.cond(within) > 1.0 / (S * np.finfo(np.float64).eps):
        raise ValueError("estimate_lda: the within-class covariance is not positive definite to working precision "
                         "(linearly dependent spliced columns, or too few frames)")
    B = P @ between @ P.T
    s, Q = np.linalg.eigh(0.5 * (B + B.T))
    order = np.argsort(-s, kind="stable")
    s, Q = s[order], Q[:, order]
    full = Q.T @ P
    big = np.abs(full).argmax(axis=1)
    sign = np.where(full[np.arange(S), big] < 0, -1.0, 1.0)
    full = full * sign[:, None]
    if remove_offset:
        full = np.concatenate([full, -(full @ m)[:, None]], axis=1)
    full32 = full.astype(np.float32)
    return np.ascontiguousarray(full32[:dim]), full32
