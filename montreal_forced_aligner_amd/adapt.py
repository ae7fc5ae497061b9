"""MAP adaptation of an acoustic model from GMM statistics: the host half of ``mfa adapt`` (MFA/alignment/adapting.py).

The reference accumulates statistics from alignments (AccStatsFunction → kalpy GmmStatsAccumulator), smooths them towards
the old model (IsmoothStatsAmDiagGmmFromModel, τ = ``mapping_tau``), re-estimates the means (``mle_update`` with update flags
"m", low-count Gaussians kept) and the transition probabilities, and writes ``final.mdl`` / ``final.alimdl``.  The
accumulation is the device's (``engine.gmm_statistics``); everything here is float64 numpy on ``kaldi_io.RawAmDiagGmm`` /
``RawTransitionModel`` — the forms that keep the mixture weights and can be written back with ``kaldi_io.write_model``.
The rules are Kaldi's, restated from their description (parity unpinned: DESIGN §2).
"""
from __future__ import annotations

import copy
from typing import Optional, Tuple

import numpy as np

from . import kaldi_io
from .engine import GmmStats
from .model import DiagGmmModel, TransitionModel, _logf

MIN_GAUSSIAN_OCCUPANCY = 10.0      # MleDiagGmmOptions: min_gaussian_occupancy, min_gaussian_weight
MIN_GAUSSIAN_WEIGHT = 1.0e-5
TRANSITION_MIN_COUNT = 5.0         # MleTransitionUpdateConfig: mincount, floor
TRANSITION_FLOOR = np.float32(0.01)


def pdf_offsets(raw_am: kaldi_io.RawAmDiagGmm) -> np.ndarray:
    offs = np.zeros(raw_am.num_pdfs + 1, dtype=np.int64)
    np.cumsum([w.shape[0] for w in raw_am.weights], out=offs[1:])
    return offs


def raw_from_soa(am: DiagGmmModel) -> kaldi_io.RawAmDiagGmm:
    """The per-pdf form of a ``DiagGmmModel``.  Mixture weights are ``am.weights`` when the model carries them; otherwise they
    are read back out of the gconsts (ln w = gconst + ½·dim·ln 2π − ½ Σ ln inv_var + ½ Σ means_invvars²/inv_var)."""
    iv = am.inv_vars.astype(np.float64)
    mi = am.means_invvars.astype(np.float64)
    if getattr(am, "weights", None) is not None:
        w = np.asarray(am.weights, dtype=np.float32)
    else:
        lw = am.gconsts.astype(np.float64) + 0.5 * (am.dim * np.log(2 * np.pi) - np.log(iv).sum(axis=1) + (mi * mi / iv).sum(axis=1))
        w = np.exp(lw).astype(np.float32)
    cut = [(int(a), int(b)) for a, b in zip(am.pdf_offsets[:-1], am.pdf_offsets[1:])]
    return kaldi_io.RawAmDiagGmm(am.dim, [am.gconsts[a:b].astype(np.float32) for a, b in cut], [w[a:b] for a, b in cut],
                                 [am.means_invvars[a:b].astype(np.float32) for a, b in cut],
                                 [am.inv_vars[a:b].astype(np.float32) for a, b in cut])


def _check(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats) -> np.ndarray:
    offs = pdf_offsets(raw_am)
    if stats.mean_acc.shape != (int(offs[-1]), raw_am.dim):
        raise ValueError(f"statistics of shape {stats.mean_acc.shape} for a model of {int(offs[-1])} Gaussians of dim {raw_am.dim}")
    return offs


def ismooth_from_model(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats, tau: float) -> GmmStats:
    """IsmoothStatsAmDiagGmmFromModel: every Gaussian i of non-zero weight gets τ frames of its own distribution,
    occ_i += τ, mean_acc_i += τ·μ_i, var_acc_i += τ·(σ²_i + μ_i²), with μ = means_invvars ⊘ inv_vars and σ² = 1 ⊘ inv_vars
    divided in float32 (the model's own means and variances).  Returns new statistics; ``stats`` is left as it is."""
    _check(raw_am, stats)
    out = stats.copy()
    tau = float(tau)
    w = np.concatenate(raw_am.weights)
    mi, iv = np.concatenate(raw_am.means_invvars).astype(np.float32), np.concatenate(raw_am.inv_vars).astype(np.float32)
    mu = (mi / iv).astype(np.float64)
    var = (np.float32(1.0) / iv).astype(np.float64)
    on = w != 0
    out.occ[on] += tau
    out.mean_acc[on] += tau * mu[on]
    out.var_acc[on] += tau * (var[on] + mu[on] * mu[on])
    return out


def gconsts(weights: np.ndarray, means_invvars: np.ndarray, inv_vars: np.ndarray) -> np.ndarray:
    """ComputeGconsts in float64, rounded to float32: ln w − ½·dim·ln 2π + ½ Σ ln inv_var − ½ Σ means_invvars²/inv_var."""
    iv, mi = inv_vars.astype(np.float64), means_invvars.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        gc = np.log(weights.astype(np.float64)) - 0.5 * iv.shape[1] * np.log(2 * np.pi) + 0.5 * np.log(iv).sum(axis=1) \
            - 0.5 * (mi * mi / iv).sum(axis=1)
    return gc.astype(np.float32)


def map_update(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats) -> Tuple[kaldi_io.RawAmDiagGmm, int, int]:
    """``mle_update(..., update_flags_str="m", remove_low_count_gaussians=False)``: means only.  Gaussian i of a pdf with
    occ_sum = Σ occ is re-estimated iff occ_i > 10 and occ_i / occ_sum > 1e-5: μ'_i = mean_acc_i / occ_i rounded to float32,
    means_invvars' = μ'·inv_vars in float32; every other Gaussian is kept.  Weights and variances are untouched.  The gconsts
    of every Gaussian are recomputed; one that is not finite raises.  Returns (new model, Gaussians updated, kept)."""
    offs = _check(raw_am, stats)
    new = kaldi_io.RawAmDiagGmm(raw_am.dim, [], [w.copy() for w in raw_am.weights], [], [iv.copy() for iv in raw_am.inv_vars])
    updated = kept = 0
    for p in range(raw_am.num_pdfs):
        a, b = int(offs[p]), int(offs[p + 1])
        occ = stats.occ[a:b]
        occ_sum = float(occ.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            share = occ / occ_sum if occ_sum > 0 else np.zeros_like(occ)
            mu = (stats.mean_acc[a:b] / occ[:, None]).astype(np.float32)
        take = (occ > MIN_GAUSSIAN_OCCUPANCY) & (share > MIN_GAUSSIAN_WEIGHT)
        iv = raw_am.inv_vars[p].astype(np.float32)
        mi = raw_am.means_invvars[p].astype(np.float32).copy()
        mi[take] = mu[take] * iv[take]
        gc = gconsts(raw_am.weights[p], mi, iv)
        if not np.isfinite(gc).all():
            raise ValueError(f"map_update: pdf {p} has a gconst that is not finite (a zero weight, variance or a bad statistic)")
        new.means_invvars.append(mi)
        new.gconsts.append(gc)
        updated += int(take.sum())
        kept += int((~take).sum())
    return new, updated, kept


def transition_update(raw_tm: kaldi_io.RawTransitionModel, tid_count: np.ndarray) -> kaldi_io.RawTransitionModel:
    """TransitionModel::MleUpdate: for every transition-state with more than one transition and a total count of at least
    5 — and no other — p = count / total in float32, three times {p /= Σp; p = max(p, 0.01)}, log_probs[tid] = ln p."""
    tm = TransitionModel(raw_tm)
    cnt = np.asarray(tid_count)
    if cnt.shape[0] != tm.num_transition_ids + 1:
        raise ValueError(f"{cnt.shape[0]} counts for {tm.num_transition_ids} transition-ids (+ 1)")
    log_probs = raw_tm.log_probs.astype(np.float32).copy()
    for ts in range(1, tm.tuples.shape[0] + 1):
        a, b = int(tm.state2id[ts]), int(tm.state2id[ts + 1])
        if b - a <= 1:
            continue
        total = float(cnt[a:b].sum())
        if total < TRANSITION_MIN_COUNT:
            continue
        p = (cnt[a:b].astype(np.float64) / total).astype(np.float32)
        for _ in range(3):
            s = np.float32(0.0)
            for v in p:
                s = np.float32(s + v)
            p = np.maximum((p / s).astype(np.float32), TRANSITION_FLOOR)
        for k in range(b - a):
            log_probs[a + k] = _logf(p[k])
    return kaldi_io.RawTransitionModel(copy.deepcopy(raw_tm.topo), raw_tm.tuples.copy(), log_probs)


def adapt_model(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats, tau: float = 20.0):
    """Smooth and update in one step; returns (new model, Gaussians updated, kept)."""
    return map_update(raw_am, ismooth_from_model(raw_am, stats, tau))
