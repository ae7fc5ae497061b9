"""The diagonal UBM — one global diagonal-covariance GMM — and the host half of the reference's ``DubmTrainer``
(MFA/ivector/trainer.py:105-388): initialisation from random frames (Kaldi gmm-global-init-from-feats), growth by splitting
(DiagGmm::Split), re-estimation (MleDiagGmmUpdate) and the schedule of the init phase.  The E-steps are the device's
(``stats.gaussian_selection``, ``stats.ubm_statistics``); everything here is float64 numpy, and the update and the split are
``mle``'s on a one-pdf view of the model, not a second copy of them.  The rules are Kaldi's, restated from their descriptions
(parity unpinned: DESIGN §2).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from . import kaldi_io, mle
from .adapt import gconsts as _gconsts
from .stats import GmmStats

MAX_GAUSSIANS = 2048               # mfa_ubm_gselect_batch's limit
MIN_GAUSSIAN_WEIGHT = 1.0e-4       # train_diag_ubm's --min-gaussian-weight


@dataclass
class DiagUbm:
    """float32 ``weights`` [G], ``means_invvars`` / ``inv_vars`` [G, dim], ``gconsts`` [G]: a ``<DiagGMM>`` object."""

    weights: np.ndarray
    means_invvars: np.ndarray
    inv_vars: np.ndarray
    gconsts: np.ndarray

    @classmethod
    def from_parameters(cls, weights, means, variances) -> "DiagUbm":
        """From float64 weights [G], means and variances [G, dim]: inv_vars and means_invvars rounded to float32, gconsts
        recomputed; one that is not finite raises."""
        w = np.asarray(weights, dtype=np.float64)
        iv = (1.0 / np.asarray(variances, dtype=np.float64)).astype(np.float32)
        mi = np.asarray(means, dtype=np.float64).astype(np.float32) * iv
        w32 = w.astype(np.float32)
        gc = _gconsts(w32, mi, iv)
        if not np.isfinite(gc).all():
            raise ValueError("DiagUbm: a gconst that is not finite (a zero weight or variance)")
        return cls(w32, mi, iv, gc)

    @classmethod
    def from_raw(cls, raw: kaldi_io.RawAmDiagGmm) -> "DiagUbm":
        if raw.num_pdfs != 1:
            raise ValueError(f"DiagUbm: a model of {raw.num_pdfs} pdfs is no global mixture")
        gc = raw.gconsts[0] if raw.gconsts[0] is not None else _gconsts(raw.weights[0], raw.means_invvars[0], raw.inv_vars[0])
        return cls(*(np.ascontiguousarray(a, dtype=np.float32) for a in (raw.weights[0], raw.means_invvars[0], raw.inv_vars[0], gc)))

    def as_raw(self) -> kaldi_io.RawAmDiagGmm:
        """The one-pdf acoustic model ``mle.mle_update`` and ``mle.mix_up`` work on."""
        return kaldi_io.RawAmDiagGmm(self.dim, [self.gconsts], [self.weights], [self.means_invvars], [self.inv_vars])

    @property
    def num_gauss(self) -> int:
        return int(self.weights.shape[0])

    @property
    def dim(self) -> int:
        return int(self.inv_vars.shape[1])

    @property
    def means(self) -> np.ndarray:
        return self.means_invvars.astype(np.float64) / self.inv_vars.astype(np.float64)

    @property
    def variances(self) -> np.ndarray:
        return 1.0 / self.inv_vars.astype(np.float64)

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(gconsts, means_invvars, inv_vars) contiguous float32, as the library takes a model."""
        return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (self.gconsts, self.means_invvars, self.inv_vars))

    def write(self, path) -> None:
        """``<i>.dubm`` / ``final.dubm``: the binary header and one ``<DiagGMM>``."""
        with open(path, "wb") as f:
            f.write(b"\0B")
            kaldi_io.write_diag_gmm(f, self.gconsts, self.weights, self.means_invvars, self.inv_vars)

    @classmethod
    def read(cls, path_or_bytes) -> "DiagUbm":
        data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
        r = kaldi_io.BinaryReader(bytes(data))
        r.expect_binary_header()
        gc, w, mi, iv = kaldi_io.read_diag_gmm(r)
        return cls.from_raw(kaldi_io.RawAmDiagGmm(int(iv.shape[1]), [gc], [w], [mi], [iv]))


def init_from_random_frames(feats: np.ndarray, num_gauss: int, rng: Optional[np.random.Generator] = None) -> DiagUbm:
    """gmm-global-init-from-feats' InitGmmFromRandomFrames: every Gaussian gets the global variance of ``feats`` (float64,
    Σx²/T − mean²), ``num_gauss`` distinct rows drawn by ``rng`` as means, and weight 1 / num_gauss.  (Kaldi draws with its
    own generator: the frames chosen are not Kaldi's.)"""
    x = np.asarray(feats, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < num_gauss or num_gauss <= 0:
        raise ValueError(f"init_from_random_frames: {num_gauss} Gaussians from features of shape {x.shape}")
    if num_gauss > MAX_GAUSSIANS:
        raise ValueError(f"init_from_random_frames: {num_gauss} Gaussians (the selection kernel takes at most {MAX_GAUSSIANS})")
    rng = np.random.default_rng(0) if rng is None else rng
    mean = x.mean(axis=0)
    var = (x * x).mean(axis=0) - mean * mean
    if not (var > 0).all():
        raise ValueError("init_from_random_frames: a feature column without variance")
    rows = np.sort(rng.choice(x.shape[0], size=num_gauss, replace=False))
    return DiagUbm.from_parameters(np.full(num_gauss, 1.0 / num_gauss), x[rows], np.tile(var, (num_gauss, 1)))


def split(ubm: DiagUbm, target: int, perturb_factor: float = 0.1, rng: Optional[np.random.Generator] = None) -> DiagUbm:
    """DiagGmm::Split up to ``target`` Gaussians: ``mle.mix_up``'s split of one pdf (the heaviest component halves its weight
    with a copy, the two means move apart by perturb_factor·σ·z), with the whole target given to the one pdf."""
    if target > MAX_GAUSSIANS:
        raise ValueError(f"split: {target} Gaussians (the selection kernel takes at most {MAX_GAUSSIANS})")
    if target <= ubm.num_gauss:
        return ubm
    raw, _ = mle.mix_up(ubm.as_raw(), [np.inf], int(target), min_count=0.0, perturb_factor=perturb_factor, rng=rng,
                        max_per_pdf=MAX_GAUSSIANS)
    return DiagUbm.from_raw(raw)


def update(ubm: DiagUbm, stats: GmmStats, remove_low_count_gaussians: bool = True,
           min_gaussian_weight: float = MIN_GAUSSIAN_WEIGHT, **mle_options):
    """``DiagGmm.mle_update(accs, remove_low_count_gaussians=)``: ``mle.mle_update`` with flags "mvw" on the one-pdf view.
    Returns (new model, Gaussians updated, removed, variance elements floored)."""
    raw, updated, removed, floored = mle.mle_update(ubm.as_raw(), stats, "mvw", min_gaussian_weight=min_gaussian_weight,
                                                    remove_low_count_gaussians=remove_low_count_gaussians, **mle_options)
    return DiagUbm.from_raw(raw), updated, removed, floored


def init_schedule(num_gaussians: int = 256, initial_gaussian_proportion: float = 0.5, num_iterations_init: int = 20,
                  rule: str = "kaldi") -> Tuple[int, List[int]]:
    """The init phase's growth: (Gaussians to start with, Gaussians to split to after each of the ``num_iterations_init``
    iterations).  The start is int(proportion · num_gaussians), or num_gaussians when that is not in (0, num_gaussians];
    inc = int((num_gaussians − start) / (num_iterations_init / 2)).
      rule "kaldi"      next = min(num_gaussians, cur + inc): gmm-global-init-from-feats.
      rule "reference"  next = min(num_gaussians, cur, inc), as MFA/ivector/trainer.py:301 reads: never above the current
                        count, so the model is never split and stays at its start (DESIGN §4 "Diagonal UBM")."""
    if rule not in ("kaldi", "reference"):
        raise ValueError(f"init_schedule: rule {rule!r} ('kaldi' or 'reference')")
    start = int(initial_gaussian_proportion * int(num_gaussians))
    if start <= 0 or start > num_gaussians:
        start = int(num_gaussians)
    inc = int((num_gaussians - start) / (num_iterations_init / 2)) if num_iterations_init > 0 else 0
    cur, out = start, []
    for _ in range(num_iterations_init):
        nxt = min(num_gaussians, cur + inc) if rule == "kaldi" else min(num_gaussians, cur, inc)
        if nxt > cur:
            cur = nxt
        out.append(cur)
    return start, out
