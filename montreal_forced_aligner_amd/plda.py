"""PLDA — the model every consumer of an i-vector goes through in the reference (``IvectorCorpusMixin.compute_plda``,
``adapt_plda``, ``transform_ivectors``, ``collect_speaker_ivectors``, MFA/corpus/ivector_corpus.py:123-452;
``PldaClassificationFunction``, MFA/diarization/multiprocessing.py) — and the host half of its life: the statistics, the EM
estimate, the unsupervised adaptation, the file, and the scoring formula in its direct form, which is the specification the
device's expanded form (``stats.plda_scores``; include/mfa_hip.h "PLDA") is held to.  Everything here is float64 numpy.

The algorithm is Kaldi's two-covariance PLDA (ivector-compute-plda, ivector-adapt-plda), restated from its description
(Kaldi's source is not among this project's references: parity unpinned); the ``<Plda>`` layout is as remembered
and equally unpinned — only a round trip is tested.

The model: a class mean y ~ N(mean, between), an example x | y ~ N(y, within).  ``transform`` T takes x − mean into the
space where within = I and between = diag(psi), psi descending.
"""
from __future__ import annotations

import io
import math
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import kaldi_io

LOG_2PI = math.log(2.0 * math.pi)


class PldaTrainingError(RuntimeError):
    """The reference's ``IvectorTrainingError`` of ``compute_plda`` (MFA/corpus/ivector_corpus.py:259-269)."""


# ---- helpers -----------------------------------------------------------------------------------------------------------
def normalize_length(x: np.ndarray) -> np.ndarray:
    """Each row (or the one vector) scaled to norm √D (Kaldi ivector-normalize-length).  A zero row stays zero."""
    x = np.asarray(x, dtype=np.float64)
    norm = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    ratio = norm / math.sqrt(x.shape[-1])
    return x / np.where(ratio == 0.0, 1.0, ratio)


def subtract_mean(X: np.ndarray) -> np.ndarray:
    """The rows with their mean taken off (Kaldi ivector-subtract-global-mean)."""
    X = np.asarray(X, dtype=np.float64)
    return X - X.mean(axis=0, keepdims=True)


def _text_vector(v: np.ndarray) -> str:
    return " [ " + " ".join(repr(float(a)) for a in v) + " ]\n"


def _text_matrix(m: np.ndarray) -> str:
    return " [\n" + "\n".join("  " + " ".join(repr(float(a)) for a in row) for row in m) + " ]\n"


# ---- the model ---------------------------------------------------------------------------------------------------------
@dataclass
class PldaModel:
    """float64 ``mean`` [D], ``transform`` [D, D] and ``psi`` [D]."""

    mean: np.ndarray
    transform: np.ndarray
    psi: np.ndarray

    def __post_init__(self):
        self.mean = np.ascontiguousarray(self.mean, dtype=np.float64)
        self.transform = np.ascontiguousarray(self.transform, dtype=np.float64)
        self.psi = np.ascontiguousarray(self.psi, dtype=np.float64)
        D = self.mean.shape[0]
        if self.mean.ndim != 1 or self.transform.shape != (D, D) or self.psi.shape != (D,):
            raise ValueError(f"PldaModel: mean {self.mean.shape}, transform {self.transform.shape}, psi {self.psi.shape}")

    @property
    def dim(self) -> int:
        return int(self.mean.shape[0])

    @property
    def offset(self) -> np.ndarray:
        """−transform·mean: what the transform adds after the product."""
        return -(self.transform @ self.mean)

    def copy(self) -> "PldaModel":
        return PldaModel(self.mean.copy(), self.transform.copy(), self.psi.copy())

    # -- file
    def write(self, path, binary: bool = True) -> None:
        """``<Plda>`` mean (double vector) transform (double matrix) psi (double vector) ``</Plda>``, Kaldi's binary or text
        object form (the layout as remembered: unpinned)."""
        if binary:
            with open(path, "wb") as f:
                f.write(b"\0B")
                kaldi_io._w_token(f, "<Plda>")
                kaldi_io.write_vector(f, self.mean)
                kaldi_io.write_matrix(f, self.transform)
                kaldi_io.write_vector(f, self.psi)
                kaldi_io._w_token(f, "</Plda>")
        else:
            Path(path).write_text("<Plda> " + _text_vector(self.mean) + _text_matrix(self.transform) + _text_vector(self.psi)
                                  + "</Plda> ", encoding="ascii")

    @classmethod
    def read(cls, path_or_bytes) -> "PldaModel":
        data = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
        if data[:2] == b"\0B":
            r = kaldi_io.BinaryReader(data)
            r.expect_binary_header()
            r.expect("<Plda>")
            mean, transform, psi = r.vector(), r.matrix(), r.vector()
            r.expect("</Plda>")
            return cls(mean.astype(np.float64), transform.astype(np.float64), psi.astype(np.float64))
        text = data.decode("ascii")
        m = re.match(r"\s*<Plda>\s*\[([^\]]*)\]\s*\[([^\]]*)\]\s*\[([^\]]*)\]\s*</Plda>\s*$", text)
        if not m:
            raise kaldi_io.KaldiFormatError("not a <Plda> object")
        mean = np.array(m.group(1).split(), dtype=np.float64)
        rows = [np.array(line.split(), dtype=np.float64) for line in m.group(2).splitlines() if line.strip()]
        psi = np.array(m.group(3).split(), dtype=np.float64)
        transform = np.stack(rows) if rows else np.zeros((0, 0))
        return cls(mean, transform, psi)

    # -- the transform
    def transform_ivector(self, x: np.ndarray, num_examples=1, normalize_length: bool = True,
                          simple_length_norm: bool = False) -> np.ndarray:
        """u = transform·x + offset, then the length normalisation: with ``simple_length_norm`` the factor √D/‖u‖, otherwise
        √(D / Σ_k u_k²/(ψ_k + 1/n)) — the factor under which u has the norm the model expects of a mean of n examples.  ``x``
        a vector or rows; ``num_examples`` a number or one per row."""
        x = np.asarray(x, dtype=np.float64)
        u = x @ self.transform.T + self.offset
        if not normalize_length:
            return u
        D = self.dim
        if simple_length_norm:
            factor = math.sqrt(D) / np.sqrt((u * u).sum(axis=-1, keepdims=True))
        else:
            n = np.asarray(num_examples, dtype=np.float64)
            n = n[..., None] if n.ndim else n
            factor = np.sqrt(D / (u * u / (self.psi + 1.0 / n)).sum(axis=-1, keepdims=True))
        return u * factor

    # -- scoring: the direct form
    def log_likelihood_ratio(self, train: np.ndarray, n, test: np.ndarray):
        """log p(test | the class of ``train``, a mean of ``n`` examples) − log p(test | a class of its own), both vectors in
        the model's space.  Broadcasts: train [..., D], n [...], test [..., D]."""
        train, test = np.asarray(train, dtype=np.float64), np.asarray(test, dtype=np.float64)
        n = np.asarray(n, dtype=np.float64)[..., None]
        psi = self.psi
        mean = n * psi / (n * psi + 1.0) * train
        var = 1.0 + psi / (n * psi + 1.0)
        D = self.dim
        given = -0.5 * (np.log(var).sum(axis=-1) + D * LOG_2PI + ((test - mean) ** 2 / var).sum(axis=-1))
        without = -0.5 * (np.log(1.0 + psi).sum() + D * LOG_2PI + (test ** 2 / (1.0 + psi)).sum(axis=-1))
        return given - without

    def log_likelihood_ratios(self, train: np.ndarray, n, test: np.ndarray) -> np.ndarray:
        """The matrix [test, train] of ``log_likelihood_ratio``, on the host: the specification of ``stats.plda_scores``."""
        train, test = np.atleast_2d(train), np.atleast_2d(test)
        n = np.broadcast_to(np.asarray(n, dtype=np.float64), (train.shape[0],))
        out = np.empty((test.shape[0], train.shape[0]))
        for i in range(test.shape[0]):
            out[i] = self.log_likelihood_ratio(train, n, test[i])
        return out

    def covariances(self) -> Tuple[np.ndarray, np.ndarray]:
        """(within, between) in the original space: T⁻¹ T⁻ᵀ and T⁻¹ diag(psi) T⁻ᵀ."""
        Ti = np.linalg.inv(self.transform)
        return Ti @ Ti.T, (Ti * self.psi) @ Ti.T


# ---- statistics ----------------------------------------------------------------------------------------------------------
@dataclass
class PldaStats:
    """What ``estimate_plda`` needs of the training classes (Kaldi PldaStats)."""

    dim: int = 0
    num_classes: int = 0
    num_examples: int = 0
    class_weight: float = 0.0
    example_weight: float = 0.0
    sum: Optional[np.ndarray] = None
    offset_scatter: Optional[np.ndarray] = None
    records: List[Tuple[float, np.ndarray, int]] = field(default_factory=list)

    def add_samples(self, weight: float, group: np.ndarray) -> None:
        """One class: ``group`` [n, D], its examples."""
        group = np.asarray(group, dtype=np.float64)
        if group.ndim != 2 or group.shape[0] == 0:
            raise ValueError("add_samples: a class is a matrix [examples, D] with at least one row")
        n, D = group.shape
        if self.dim == 0:
            self.dim, self.sum, self.offset_scatter = D, np.zeros(D), np.zeros((D, D))
        elif D != self.dim:
            raise ValueError(f"add_samples: dimension {D} after {self.dim}")
        m = group.mean(axis=0)
        self.num_classes += 1
        self.num_examples += n
        self.class_weight += weight
        self.example_weight += weight * n
        self.sum += weight * m
        self.offset_scatter += weight * (group.T @ group - n * np.outer(m, m))
        self.records.append((float(weight), m, int(n)))

    def sort(self) -> None:
        """The records by their number of examples (stable): the estimate inverts once per distinct count."""
        self.records.sort(key=lambda r: r[2])

    def is_sorted(self) -> bool:
        return all(a[2] <= b[2] for a, b in zip(self.records, self.records[1:]))


def _by_count(stats: PldaStats):
    """(n, weights [c], centred means [c, D]) per distinct n of the sorted records."""
    gmean = stats.sum / stats.class_weight
    out, i, recs = [], 0, stats.records
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j][2] == recs[i][2]:
            j += 1
        out.append((recs[i][2], np.array([r[0] for r in recs[i:j]]), np.stack([r[1] for r in recs[i:j]]) - gmean))
        i = j
    return out


def plda_objective(stats: PldaStats, within: np.ndarray, between: np.ndarray) -> float:
    """The log marginal likelihood of the training examples under (global mean, within, between), per example: a class mean
    of n examples is N(mean, between + within/n), the deviations from it carry within."""
    D = stats.dim
    _, logdet_w = np.linalg.slogdet(within)
    tot = -0.5 * ((stats.example_weight - stats.class_weight) * (D * LOG_2PI + logdet_w)
                  + np.trace(np.linalg.solve(within, stats.offset_scatter)))
    for n, w, m in _by_count(stats):
        cov = between + within / n
        _, logdet = np.linalg.slogdet(cov)
        quad = (m * np.linalg.solve(cov, m.T).T).sum(axis=1)
        tot += -0.5 * (w * (D * LOG_2PI + logdet + D * math.log(n) + quad)).sum()
    return float(tot / stats.example_weight)


def em_plda(stats: PldaStats, num_em_iters: int = 10):
    """``num_em_iters`` EM rounds from within = between = I.  Returns (within, between, objectives): the objective of the
    model every round started from, then the final one's."""
    if not stats.is_sorted():
        stats.sort()
    D = stats.dim
    within, between = np.eye(D), np.eye(D)
    groups = _by_count(stats)
    objectives = []
    for _ in range(int(num_em_iters)):
        objectives.append(plda_objective(stats, within, between))
        within_inv, between_inv = np.linalg.inv(within), np.linalg.inv(between)
        b_stats, w_stats, b_count, w_count = np.zeros((D, D)), np.zeros((D, D)), 0.0, 0.0
        for n, wt, m in groups:                              # one inversion per distinct n
            mixed = np.linalg.inv(between_inv + n * within_inv)
            w = (n * (m @ within_inv.T)) @ mixed.T           # rows: mixed·(n·within⁻¹·m)
            b_stats += wt.sum() * mixed + (w * wt[:, None]).T @ w
            mw = m - w
            w_stats += n * (wt.sum() * mixed + (mw * wt[:, None]).T @ mw)
            b_count += wt.sum()
            w_count += wt.sum()
        w_stats += stats.offset_scatter
        w_count += stats.example_weight - stats.class_weight
        within, between = w_stats / w_count, b_stats / b_count
        within, between = 0.5 * (within + within.T), 0.5 * (between + between.T)
    objectives.append(plda_objective(stats, within, between))
    return within, between, objectives


def diagonalise(mean: np.ndarray, within: np.ndarray, between: np.ndarray) -> PldaModel:
    """T₁ = chol(within)⁻¹; T₁·between·T₁ᵀ = U diag(s) Uᵀ; transform = Uᵀ·T₁, psi = s floored at 0, descending."""
    L = np.linalg.cholesky(within)
    T1 = np.linalg.inv(L)
    M = T1 @ between @ T1.T
    s, U = np.linalg.eigh(0.5 * (M + M.T))
    order = np.argsort(-s, kind="stable")
    s, U = np.maximum(s[order], 0.0), U[:, order]
    return PldaModel(np.array(mean, dtype=np.float64), U.T @ T1, s)


def estimate_plda(stats: PldaStats, num_em_iters: int = 10) -> PldaModel:
    if stats.num_classes == 0:
        raise PldaTrainingError("No stats accumulated, unable to estimate PLDA.")
    within, between, _ = em_plda(stats, num_em_iters)
    return diagonalise(stats.sum / stats.class_weight, within, between)


def group_by_speaker(ivectors: Mapping[str, np.ndarray], utt2spk: Mapping[str, str]) -> Dict[str, np.ndarray]:
    """speaker → [utterances, D], utterances in the mapping's order; an utterance without a speaker is left out."""
    groups: Dict[str, List[np.ndarray]] = {}
    for utt, v in ivectors.items():
        spk = utt2spk.get(utt)
        if spk is not None:
            groups.setdefault(spk, []).append(np.asarray(v, dtype=np.float64))
    return {s: np.stack(v) for s, v in groups.items()}


def train_plda(ivectors: Mapping[str, np.ndarray], utt2spk: Mapping[str, str], minimum_utterance_count: int = 1,
               num_em_iters: int = 10) -> PldaModel:
    """The reference's ``compute_plda``: every vector length-normalised, one class per speaker with at least
    ``minimum_utterance_count`` utterances, its three refusals, then the estimate."""
    stats = PldaStats()
    for spk, mat in group_by_speaker(ivectors, utt2spk).items():
        if mat.shape[0] < max(int(minimum_utterance_count), 1):
            continue
        stats.add_samples(1.0, normalize_length(mat))
    if stats.num_classes == 0:
        raise PldaTrainingError("No stats accumulated, unable to estimate PLDA.")
    if stats.num_examples <= stats.dim:
        raise PldaTrainingError("Number of training iVectors is not greater than their dimension, unable to estimate PLDA.")
    if stats.num_classes == stats.num_examples:
        raise PldaTrainingError("No speakers with multiple utterances, unable to estimate PLDA.")
    stats.sort()
    return estimate_plda(stats, num_em_iters)


# ---- unsupervised adaptation -------------------------------------------------------------------------------------------------
class PldaUnsupervisedAdaptor:
    """Kaldi's ivector-adapt-plda: move a model towards unlabelled in-domain vectors.  The data's total covariance (plus
    ``mean_diff_scale`` times the outer product of the mean shift) is brought into the model's space, each direction scaled by
    1/√(1 + ψ) so that the model's own total covariance is the identity there, and diagonalised as P·diag(s)·Pᵀ; in that basis
    the model's within covariance is Pᵀdiag(1/(1+ψ))P and its between covariance Pᵀdiag(ψ/(1+ψ))P (in the unscaled model space:
    I and diag ψ).  Where an eigenvalue s exceeds 1, the excess s − 1 — variance the model does not account for — is given to
    the within covariance (``within_covar_scale``) and the between covariance (``between_covar_scale``) in that direction; both
    are taken back to the original space and re-diagonalised; the model's mean becomes the data's.  Data drawn from the model
    itself has s ≈ 1 and leaves it as it is, up to the sampling spread of s."""

    def __init__(self, mean_diff_scale: float = 1.0, within_covar_scale: float = 0.3, between_covar_scale: float = 0.7):
        self.mean_diff_scale, self.within_covar_scale = float(mean_diff_scale), float(within_covar_scale)
        self.between_covar_scale = float(between_covar_scale)
        self.tot_weight = 0.0
        self.mean_stats: Optional[np.ndarray] = None
        self.variance_stats: Optional[np.ndarray] = None

    def add_stats(self, weight: float, x: np.ndarray) -> None:
        """``x``: one vector, or rows that each get ``weight``."""
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        if self.mean_stats is None:
            self.mean_stats, self.variance_stats = np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
        self.tot_weight += weight * x.shape[0]
        self.mean_stats += weight * x.sum(axis=0)
        self.variance_stats += weight * (x.T @ x)

    def data_moments(self) -> Tuple[np.ndarray, np.ndarray]:
        mean = self.mean_stats / self.tot_weight
        return mean, self.variance_stats / self.tot_weight - np.outer(mean, mean)

    def update_plda(self, model: PldaModel) -> PldaModel:
        """The adapted model (``model`` is left as it is)."""
        if self.tot_weight <= 0.0:
            raise ValueError("update_plda: no statistics")
        mean, variance = self.data_moments()
        diff = mean - model.mean
        variance = variance + self.mean_diff_scale * np.outer(diff, diff)
        # the model's space with every direction scaled by 1/√(1 + ψ): there the model's total covariance is I, so an
        # eigenvalue above 1 is variance the model does not account for (data drawn from the model itself has none)
        T = model.transform / np.sqrt(1.0 + model.psi)[:, None]
        V = T @ variance @ T.T
        s, P = np.linalg.eigh(0.5 * (V + V.T))
        W = (P.T / (1.0 + model.psi)) @ P                    # Pᵀ·diag(1/(1+ψ))·P: the model's within covariance there
        B = (P.T * (model.psi / (1.0 + model.psi))) @ P      # Pᵀ·diag(ψ/(1+ψ))·P: its between covariance
        excess = np.maximum(s - 1.0, 0.0)
        W[np.diag_indices_from(W)] += self.within_covar_scale * excess
        B[np.diag_indices_from(B)] += self.between_covar_scale * excess
        Qi = np.linalg.inv(P.T @ T)                          # from the eigenbasis back to the original space
        within, between = Qi @ W @ Qi.T, Qi @ B @ Qi.T
        return diagonalise(mean, 0.5 * (within + within.T), 0.5 * (between + between.T))


# ---- the expanded form (what the device computes) ----------------------------------------------------------------------------
def expanded_operands(psi: np.ndarray, train: np.ndarray, n) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(A [Ns, D], B [Ns, D], c [Ns]) with score_ij = c_j + Σ_k p_ik²·A_jk + Σ_k p_ik·B_jk (include/mfa_hip.h "PLDA"), in
    numpy: the device's prepare step restated (``stats.plda_prepare_host`` is the twin)."""
    train = np.atleast_2d(np.asarray(train, dtype=np.float64))
    n = np.broadcast_to(np.asarray(n, dtype=np.float64), (train.shape[0],))[:, None]
    a = n * psi / (n * psi + 1.0)
    v = 1.0 + psi / (n * psi + 1.0)
    A = -0.5 * (psi * a / (v * (1.0 + psi)))                 # = −½(1/v − 1/(1+ψ)) without the difference
    B = a * train / v
    c = 0.5 * (np.log1p(psi * a / v).sum(axis=1) - ((a * train) ** 2 / v).sum(axis=1))   # log((1+ψ)/v) = log1p(ψa/v)
    return A, B, c
