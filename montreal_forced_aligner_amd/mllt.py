"""The MLLT estimate from per-Gaussian full second moments, and what the LDA+MLLT stage does with it: what ``est-mllt``,
``gmm-transform-means`` and ``compose-transforms`` make of ``gmm-acc-mllt``'s sums (the reference's ``LdaTrainer``,
MFA/acoustic_modeling/lda.py:372-451), in float64 numpy.  Restated from the algorithm's description (Gales, "Semi-tied
covariance matrices for hidden Markov models", 1999) — Kaldi's source is not among this project's references: parity
unpinned; the sweep count of 200 in particular is Kaldi's as remembered, not as checked.

Kaldi's accumulator keeps, for every output dimension j, G_j = Σ_{t,g} γ_tg · inv_var_g[j] · d_tg d_tgᵀ with d = x − μ_g.
The device keeps F_g = Σ_t γ_tg d_tg d_tgᵀ per Gaussian (``stats.MlltStats.full``), and G_j = Σ_g inv_var_g[j] · F_g is one
GEMM here (``mllt_accs``).  With beta = Σ occ the auxiliary function of a square transform M with rows m_j is

    Q(M) = beta · log|det M| − ½ Σ_j m_j G_j m_jᵀ

and a row's maximiser, the others held, is m_i = G_i⁻¹ c · sqrt(beta / cᵀ G_i⁻¹ c) with c = row i of M⁻ᵀ (the cofactors over
the determinant).
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import adapt as _adapt
from . import kaldi_io
from .model import DiagGmmModel
from .stats import MlltStats


def mllt_accs(stats: MlltStats, gmm) -> Tuple[float, np.ndarray]:
    """(beta, G [D, D, D]) of the statistics under the model they were accumulated with (a ``DiagGmmModel`` or a
    ``RawAmDiagGmm``): beta = Σ occ, G_j = Σ_g inv_vars[g][j] · full[g] — one float64 GEMM [D, G] × [G, D·D]."""
    if not hasattr(gmm, "pdf_offsets"):
        gmm = DiagGmmModel.from_raw(gmm)
    iv = np.asarray(gmm.inv_vars, dtype=np.float64)
    full = np.asarray(stats.full, dtype=np.float64)
    Gn, D = iv.shape
    if full.shape != (Gn, D, D):
        raise ValueError(f"mllt_accs: statistics {full.shape} do not fit a model of {Gn} Gaussians of dim {D}")
    G = (iv.T @ full.reshape(Gn, D * D)).reshape(D, D, D)
    return float(np.asarray(stats.occ, dtype=np.float64).sum()), G


def objective(beta: float, G: np.ndarray, M: np.ndarray) -> float:
    """Q(M) = beta·log|det M| − ½ Σ_j m_j G_j m_jᵀ in float64."""
    M = np.asarray(M, dtype=np.float64)
    _sign, logdet = np.linalg.slogdet(M)
    return float(beta * logdet - 0.5 * np.einsum("ja,jab,jb->", M, np.asarray(G, dtype=np.float64), M))


def estimate_mllt(beta: float, G: np.ndarray, num_sweeps: int = 200, dtype=np.float32) -> Tuple[np.ndarray, float, float, List[float]]:
    """The row update of semi-tied covariances from M = I: ``num_sweeps`` sweeps over the rows, each row set to its
    maximiser.  Returns (mat [D, D] as ``dtype``, objf_impr = the sum of the per-row gains of Q, count = beta, trace = the
    running total after every sweep).  ValueError: beta ≤ 0, a G_j that is not symmetric positive definite, and a row update
    that lowers the objective beyond rounding (a bug, not data)."""
    G = np.array(G, dtype=np.float64)      # a copy: symmetrised below
    beta = float(beta)
    if G.ndim != 3 or G.shape[0] != G.shape[1] or G.shape[1] != G.shape[2]:
        raise ValueError(f"estimate_mllt: G of shape {G.shape} is not [D, D, D]")
    if not beta > 0:
        raise ValueError(f"estimate_mllt: beta = {beta}: no frames in the statistics")
    D = G.shape[0]
    Ginv = np.empty_like(G)
    eye = np.eye(D)
    for j in range(D):
        sym = 0.5 * (G[j] + G[j].T)
        try:
            L = np.linalg.cholesky(sym)
        except np.linalg.LinAlgError:
            raise ValueError(f"estimate_mllt: G[{j}] is not positive definite (too few frames for dimension {D}, or a "
                             "Gaussian with a non-positive variance)") from None
        Li = np.linalg.solve(L, eye)
        Ginv[j] = Li.T @ Li
        G[j] = sym
    M = np.eye(D)
    total, trace = 0.0, []
    for _sweep in range(int(num_sweeps)):
        for i in range(D):
            c = np.linalg.inv(M)[:, i]                 # row i of M⁻ᵀ: old m_i · c = 1
            gc = Ginv[i] @ c
            new = gc * np.sqrt(beta / float(c @ gc))   # new G_i newᵀ = beta
            old_quad = float(M[i] @ G[i] @ M[i])
            gain = beta * np.log(abs(float(new @ c))) - 0.5 * (beta - old_quad)
            if gain < -1e-9 * beta:
                raise ValueError(f"estimate_mllt: the update of row {i} lowers the objective by {-gain:g} (beta {beta:g})")
            M[i] = new
            total += gain
        trace.append(total)
    return M.astype(dtype), float(total), beta, trace


def transform_means(raw_am: kaldi_io.RawAmDiagGmm, mat: np.ndarray) -> kaldi_io.RawAmDiagGmm:
    """``gmm-transform-means``: μ' = M μ for every Gaussian (float64, rounded to float32), ``means_invvars`` rebuilt from the
    unchanged ``inv_vars`` in float32, gconsts recomputed with ``adapt.gconsts``.  Weights and variances are untouched."""
    M = np.asarray(mat, dtype=np.float64)
    D = int(raw_am.dim)
    if M.shape != (D, D):
        raise ValueError(f"transform_means: a {M.shape} matrix for a model of dimension {D}")
    out = kaldi_io.RawAmDiagGmm(D, [], [], [], [])
    for w, mi, iv in zip(raw_am.weights, raw_am.means_invvars, raw_am.inv_vars):
        iv = np.asarray(iv, dtype=np.float32)
        mean = np.asarray(mi, dtype=np.float64) / iv.astype(np.float64)
        new_mi = (mean @ M.T).astype(np.float32) * iv
        w = np.asarray(w, dtype=np.float32)
        out.gconsts.append(_adapt.gconsts(w, new_mi, iv)); out.weights.append(w.copy())
        out.means_invvars.append(new_mi); out.inv_vars.append(iv.copy())
    return out


def compose_transforms(a: np.ndarray, b: np.ndarray, b_is_affine: bool = False) -> np.ndarray:
    """``compose-transforms``: a·b for a linear ``a`` [D, D] and a linear ``b`` [D, S], float32.  An affine ``b`` (S + 1
    columns: an LDA matrix estimated with ``remove_offset``) is refused: the reference's stage never makes one."""
    if b_is_affine:
        raise ValueError("compose_transforms: an affine second transform (an LDA matrix with remove_offset) is not supported")
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a64.ndim != 2 or a64.shape[0] != a64.shape[1]:
        raise ValueError(f"compose_transforms: the first transform {a64.shape} is not square")
    if b64.ndim != 2 or b64.shape[0] != a64.shape[1]:
        raise ValueError(f"compose_transforms: a {a64.shape} transform does not apply to the rows of a {b64.shape} one")
    return np.ascontiguousarray((a64 @ b64).astype(np.float32))
