"""The i-vector extractor — the model of the reference's ``IvectorTrainer`` (MFA/ivector/trainer.py:390-632) with
``use_weights = False`` — and the host half of its training: initialisation from a diagonal UBM, the statistics object, the
M-step with the variance and prior updates, and the diagnostic objective.  The E-steps are the device's
(``stats.ivector_utterance_statistics``, ``stats.ivector_estep``); everything here is float64 numpy.  The algorithm is Kaldi's
ivector-extractor, restated from its description (Kaldi's source is not among this project's references: parity unpinned,
DESIGN §2); the ``.ie`` layout is as remembered and equally unpinned — only a round trip is tested.

Notation: G Gaussians, feature dimension D, i-vector dimension R, P = R (R + 1) / 2; a symmetric matrix is stored as its packed
lower triangle, row-major (``kaldi_io.pack_lower``).  The model: x_t | i, w ~ N(M_i w, SigmaInv_i⁻¹), w ~ N(prior_offset·e₀, I).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from . import kaldi_io
from .kaldi_io import pack_lower, unpack_lower

PRIOR_OFFSET = 100.0               # the offset an extractor starts with
MAX_IVECTOR_DIM = 192              # mfa_ivector_estep_batch's limit (config.IVECTOR_DIMENSION)


@dataclass
class IvectorExtractorModel:
    """float64 ``w_vec`` [G] (the UBM's weights: carried, not trained), ``M`` [G, D, R], ``sigma_inv`` [G, D, D] and the scalar
    ``prior_offset``."""

    w_vec: np.ndarray
    M: np.ndarray
    sigma_inv: np.ndarray
    prior_offset: float

    @classmethod
    def from_diag_ubm(cls, ubm, ivector_dim: int, rng: Optional[np.random.Generator] = None) -> "IvectorExtractorModel":
        """SigmaInv_i = diag(inv_vars_i); prior_offset = 100; column 0 of M_i = mean_i / prior_offset; the other columns
        standard-normal draws of ``rng`` (a numpy generator, not Kaldi's: the draws differ)."""
        R = int(ivector_dim)
        if R <= 0 or R > MAX_IVECTOR_DIM:
            raise ValueError(f"from_diag_ubm: i-vector dimension {R} (1 to {MAX_IVECTOR_DIM})")
        rng = np.random.default_rng(0) if rng is None else rng
        G, D = ubm.num_gauss, ubm.dim
        M = rng.standard_normal((G, D, R))
        M[:, :, 0] = ubm.means / PRIOR_OFFSET
        sigma_inv = np.zeros((G, D, D))
        sigma_inv[:, np.arange(D), np.arange(D)] = ubm.inv_vars.astype(np.float64)
        return cls(ubm.weights.astype(np.float64), M, sigma_inv, PRIOR_OFFSET)

    @property
    def num_gauss(self) -> int:
        return int(self.M.shape[0])

    @property
    def dim(self) -> int:
        return int(self.M.shape[1])

    @property
    def ivector_dim(self) -> int:
        return int(self.M.shape[2])

    def derived(self) -> Tuple[np.ndarray, np.ndarray]:
        """(W [G, D, R], U [G, P]): W_i = SigmaInv_i·M_i and U_i = vec(M_iᵀ·SigmaInv_i·M_i), contiguous float64, as the
        library takes the model."""
        W = np.einsum("gde,ger->gdr", self.sigma_inv, self.M)
        U = np.einsum("gdr,gds->grs", self.M, W)
        U = 0.5 * (U + U.transpose(0, 2, 1))
        return np.ascontiguousarray(W), pack_lower(U)

    def copy(self) -> "IvectorExtractorModel":
        return IvectorExtractorModel(self.w_vec.copy(), self.M.copy(), self.sigma_inv.copy(), float(self.prior_offset))

    def write(self, path) -> None:
        """``<i>.ie`` / ``final.ie``: ``<IvectorExtractor> <w> <w_vec> <M> <SigmaInv> <IvectorOffset> </IvectorExtractor>`` with
        double matrices and packed symmetric matrices (the layout as remembered: unpinned)."""
        G, D = self.num_gauss, self.dim
        with open(path, "wb") as f:
            f.write(b"\0B")
            kaldi_io._w_token(f, "<IvectorExtractor>")
            kaldi_io._w_token(f, "<w>")
            kaldi_io.write_matrix(f, np.zeros((0, 0)))                       # no i-vector dependent weights
            kaldi_io._w_token(f, "<w_vec>")
            kaldi_io.write_vector(f, np.asarray(self.w_vec, dtype=np.float64))
            kaldi_io._w_token(f, "<M>")
            kaldi_io._w_int32(f, G)
            for i in range(G):
                kaldi_io.write_matrix(f, np.asarray(self.M[i], dtype=np.float64))
            kaldi_io._w_token(f, "<SigmaInv>")
            for i in range(G):
                kaldi_io.write_sp_matrix(f, pack_lower(np.asarray(self.sigma_inv[i], dtype=np.float64)), D)
            kaldi_io._w_token(f, "<IvectorOffset>")
            kaldi_io.write_double(f, self.prior_offset)
            kaldi_io._w_token(f, "</IvectorExtractor>")

    @classmethod
    def read(cls, path_or_bytes) -> "IvectorExtractorModel":
        data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
        r = kaldi_io.BinaryReader(bytes(data))
        r.expect_binary_header()
        r.expect("<IvectorExtractor>")
        r.expect("<w>")
        if r.matrix().size:
            raise kaldi_io.KaldiFormatError("an extractor with i-vector dependent weights is not supported")
        r.expect("<w_vec>")
        w_vec = r.vector().astype(np.float64)
        r.expect("<M>")
        G = r.int32()
        M = np.stack([r.matrix().astype(np.float64) for _ in range(G)])
        r.expect("<SigmaInv>")
        D = M.shape[1]
        sigma_inv = np.stack([unpack_lower(kaldi_io.read_sp_matrix(r).astype(np.float64), D) for _ in range(G)])
        r.expect("<IvectorOffset>")
        offset = float(r.float32())
        r.expect("</IvectorExtractor>")
        return cls(w_vec, M, sigma_inv, offset)


@dataclass
class IvectorStats:
    """What an E-step pass leaves, float64: ``gamma`` [G] (Γ), ``Y`` [G, D, R], ``Rq`` [G, P], ``isum`` [R], ``iscat`` [P], the
    utterance count ``n``; the global second-order statistics ``S`` [G, D (D + 1) / 2] (they do not depend on the extractor: the
    trainer computes them once); and the two sums of the objective that need the factorisation, ``quad`` = Σ_u lin·μ and
    ``logdet`` = Σ_u log det Q.  Additive: ``a += b``; what a sum over batches, or later over ranks, needs."""

    gamma: np.ndarray
    Y: np.ndarray
    Rq: np.ndarray
    isum: np.ndarray
    iscat: np.ndarray
    n: float
    S: np.ndarray
    quad: float = 0.0
    logdet: float = 0.0

    @classmethod
    def zeros(cls, num_gauss: int, dim: int, ivector_dim: int) -> "IvectorStats":
        P = ivector_dim * (ivector_dim + 1) // 2
        return cls(np.zeros(num_gauss), np.zeros((num_gauss, dim, ivector_dim)), np.zeros((num_gauss, P)), np.zeros(ivector_dim),
                   np.zeros(P), 0.0, np.zeros((num_gauss, dim * (dim + 1) // 2)))

    def copy(self) -> "IvectorStats":
        return IvectorStats(self.gamma.copy(), self.Y.copy(), self.Rq.copy(), self.isum.copy(), self.iscat.copy(), float(self.n),
                            self.S.copy(), float(self.quad), float(self.logdet))

    def __iadd__(self, other: "IvectorStats") -> "IvectorStats":
        if self.Y.shape != other.Y.shape:
            raise ValueError("IvectorStats of different models cannot be added")
        self.gamma += other.gamma
        self.Y += other.Y
        self.Rq += other.Rq
        self.isum += other.isum
        self.iscat += other.iscat
        self.n += other.n
        self.S += other.S
        self.quad += other.quad
        self.logdet += other.logdet
        return self


def objective(model: IvectorExtractorModel, stats: IvectorStats) -> float:
    """The marginal log-likelihood of the statistics under ``model`` — the model the E-step that wrote ``stats`` ran with —
    per frame (divided by ΣΓ).  Per utterance, with w integrated out,
      Σ_i γ_i (½ log det SigmaInv_i − (D/2) log 2π) − ½ Σ_i tr(SigmaInv_i S_u[i]) + ½ linᵀ Q⁻¹ lin − ½ log det Q − ½ prior_offset²:
    the joint is exp(−½ wᵀ Q w + wᵀ lin − ½ prior_offset² + terms without w) / (2π)^(R/2), and the Gaussian integral over w
    gives (2π)^(R/2) |Q|^(−½) exp(½ linᵀ Q⁻¹ lin).  linᵀ Q⁻¹ lin = lin·μ.  Diagnostic: computed on the host."""
    D = model.dim
    logdet_si = np.linalg.slogdet(model.sigma_inv)[1]
    S = unpack_lower(stats.S, D)
    tot = float(np.dot(stats.gamma, 0.5 * logdet_si - 0.5 * D * np.log(2.0 * np.pi)))
    tot -= 0.5 * float(np.einsum("gde,gde->", model.sigma_inv, S))
    tot += 0.5 * stats.quad - 0.5 * stats.logdet - 0.5 * stats.n * model.prior_offset ** 2
    occ = float(stats.gamma.sum())
    return tot / occ if occ > 0 else 0.0


def prior_transform(stats: IvectorStats) -> Tuple[np.ndarray, float]:
    """(V, new prior_offset) of the prior update: m = isum / n, C = iscat / n − m mᵀ; T whitens C (T C Tᵀ = I, from C's
    eigenvectors); A is the orthogonal reflection taking T m / ‖T m‖ to e₀ — the identity when it already is e₀; V = A T, and
    the new offset is ‖T m‖.  V maps the i-vectors' empirical distribution to mean ‖T m‖·e₀ and unit covariance."""
    R = stats.isum.shape[0]
    m = stats.isum / stats.n
    C = unpack_lower(stats.iscat, R) / stats.n - np.outer(m, m)
    lam, Pm = np.linalg.eigh(C)
    if not (lam > 0).all():
        raise ValueError("prior_transform: the i-vectors' covariance is not positive definite")
    T = (Pm / np.sqrt(lam)).T
    v = T @ m
    norm = float(np.linalg.norm(v))
    a = v / norm
    a[0] -= 1.0
    aa = float(a @ a)
    A = np.eye(R) if aa < 1e-28 else np.eye(R) - (2.0 / aa) * np.outer(a, a)
    return A @ T, norm


def update(model: IvectorExtractorModel, stats: IvectorStats, gaussian_min_count: float = 100.0, update_variances: bool = True,
           variance_floor_factor: float = 0.1, update_prior: bool = True):
    """The M-step.  For every i with Γ_i >= ``gaussian_min_count``: M_i = Y_i·Rq_i⁻¹; with ``update_variances``, from the new
    M_i, C_i = (S_i − Y_i M_iᵀ − M_i Y_iᵀ + M_i Rq_i M_iᵀ) / Γ_i, floored in the metric of F = factor·ΣS / ΣΓ (the eigenvalues
    of L⁻¹ C L⁻ᵀ floored at 1, F = L Lᵀ), SigmaInv_i = C_i⁻¹.  Then the prior update (``prior_transform``): M_i ← M_i·V⁻¹,
    prior_offset ← ‖T m‖.  Returns (new model, Gaussians updated, Gaussians skipped for their count, eigenvalues floored)."""
    G, D, R = model.num_gauss, model.dim, model.ivector_dim
    new = model.copy()
    Rq = unpack_lower(stats.Rq, R)
    S = unpack_lower(stats.S, D)
    ok = stats.gamma >= gaussian_min_count
    floored = 0
    Lf = None
    if update_variances and ok.any():
        F = variance_floor_factor * S.sum(axis=0) / stats.gamma.sum()
        Lf = np.linalg.cholesky(F)
    for i in np.flatnonzero(ok):
        Mi = np.linalg.solve(Rq[i], stats.Y[i].T).T                         # Y_i Rq_i⁻¹ (Rq_i symmetric)
        new.M[i] = Mi
        if update_variances:
            YM = stats.Y[i] @ Mi.T
            C = (S[i] - YM - YM.T + Mi @ Rq[i] @ Mi.T) / stats.gamma[i]
            C = 0.5 * (C + C.T)
            Li = np.linalg.inv(Lf)
            lam, Pm = np.linalg.eigh(Li @ C @ Li.T)
            low = lam < 1.0
            if low.any():
                floored += int(low.sum())
                C = Lf @ (Pm * np.maximum(lam, 1.0)) @ Pm.T @ Lf.T
                C = 0.5 * (C + C.T)
            new.sigma_inv[i] = np.linalg.inv(C)
            new.sigma_inv[i] = 0.5 * (new.sigma_inv[i] + new.sigma_inv[i].T)
    if update_prior and stats.n > 0:
        V, offset = prior_transform(stats)
        new.M = new.M @ np.linalg.inv(V)
        new.prior_offset = offset
    return new, int(ok.sum()), int(G - ok.sum()), floored
