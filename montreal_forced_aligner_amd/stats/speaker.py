"""The speaker path's statistics from features alone: the diagonal UBM (Gaussian selection, global statistics) and the i-vector
extractor (pruning, utterance statistics, E-step), device call and host twin each.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from .._lib import twin_call
from ._common import accumulators, device_model, store_accumulators
from .alignment import GmmStats


# ---- diagonal UBM: Gaussian selection and the global statistics over the selected Gaussians (include/mfa_hip.h "Diagonal UBM")
def _ubm_feats(feats, ubm, what):
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or not feats.is_cuda or feats.dim() != 2:
        raise _lib.MfaHipError(f"{what}: features must be a float32 matrix on the device")
    if feats.shape[0] and feats.shape[1] != ubm.dim:
        raise _lib.MfaHipError(f"{what}: features {tuple(feats.shape)} for a model of dim {ubm.dim}")
    return feats.contiguous()


def gaussian_selection(engine, feats: torch.Tensor, ubm, num_gselect: int):
    """Every frame's ``min(num_gselect, G)`` best Gaussians of ``ubm`` (a ``ubm.DiagUbm``), best first, and its log-likelihood
    over them (mfa_ubm_gselect_batch; Kaldi gmm-gselect).  ``feats`` float32 [T, dim] on the device.  Returns (gselect int32
    [T, n], loglike float32 [T]) on the device."""
    feats = _ubm_feats(feats, ubm, "gaussian_selection")
    n = max(min(int(num_gselect), ubm.num_gauss), 0)
    gselect = torch.empty((feats.shape[0], n), dtype=torch.int32, device=engine.device)
    loglike = torch.empty(feats.shape[0], dtype=torch.float32, device=engine.device)
    engine._launch_ubm_gselect(feats, device_model(engine, ubm, ubm.arrays), int(num_gselect), gselect, loglike)
    return gselect, loglike


def ubm_statistics(engine, feats: torch.Tensor, ubm, gselect: Optional[torch.Tensor] = None,
                   frame_weight: Optional[torch.Tensor] = None, into: Optional[GmmStats] = None, want_post: bool = False):
    """Global GMM statistics of one batch (mfa_ubm_acc_batch; Kaldi gmm-global-acc-stats): posteriors over each frame's
    ``gselect`` row (int32 [T, n] on the device), or over every Gaussian with ``gselect=None``.  ``frame_weight``: float32 [T]
    on the device (default 1).  ``into``: one-pdf statistics to add to, and the object returned.  With ``want_post`` (needs a
    ``gselect``) also returns the posteriors, float32 [T, n] on the device."""
    feats = _ubm_feats(feats, ubm, "ubm_statistics")
    dev, G, D, T = engine.device, ubm.num_gauss, ubm.dim, int(feats.shape[0])
    st = into if into is not None else GmmStats.zeros(G, D, 1)
    if st.mean_acc.shape != (G, D):
        raise ValueError("ubm_statistics: `into` does not fit the model")
    n = 0
    if gselect is not None:
        if gselect.dtype != torch.int32 or not gselect.is_cuda or gselect.dim() != 2 or gselect.shape[0] != T:
            raise _lib.MfaHipError(f"ubm_statistics: the selection must be an int32 [frames, n] tensor on the device (got {tuple(gselect.shape)} {gselect.dtype})")
        gselect, n = gselect.contiguous(), int(gselect.shape[1])
    elif want_post:
        raise _lib.MfaHipError("ubm_statistics: posteriors come in the order of a selection: want_post needs gselect")
    if frame_weight is not None:
        if frame_weight.dtype != torch.float32 or not frame_weight.is_cuda or tuple(frame_weight.shape) != (T,):
            raise _lib.MfaHipError("ubm_statistics: frame weights must be a float32 vector on the device, one per frame")
        frame_weight = frame_weight.contiguous()
    acc = accumulators(st, dev)
    post = torch.empty((T, n), dtype=torch.float32, device=dev) if want_post else None
    engine._launch_ubm_acc(feats, device_model(engine, ubm, ubm.arrays), n, gselect, frame_weight, *acc, post)
    store_accumulators(st, acc)
    return (st, post) if want_post else st


_UBM_TWIN_CODES = {-2: "feature dimension above 48", -3: "Gaussians outside [1, 2048]", -4: "Gaussians per frame outside [1, 64]",
                   -5: "2^31 frames or more"}


def gaussian_selection_host(feats: np.ndarray, ubm, num_gselect: int):
    """``gaussian_selection`` on the host twin (mfa_debug_ubm_gselect_host): numpy arrays in and out."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    if feats.ndim != 2 or (feats.shape[0] and feats.shape[1] != ubm.dim):
        raise _lib.MfaHipError(f"gaussian_selection_host: features {feats.shape} for a model of dim {ubm.dim}")
    gc, mi, iv = ubm.arrays()
    n = max(min(int(num_gselect), ubm.num_gauss), 0)
    gselect = np.empty((feats.shape[0], n), dtype=np.int32)
    loglike = np.empty(feats.shape[0], dtype=np.float32)
    twin_call("mfa_debug_ubm_gselect_host", _UBM_TWIN_CODES, feats, int(feats.shape[0]), int(mi.shape[1]), int(gc.shape[0]), gc, mi, iv,
              int(num_gselect), gselect, loglike)
    return gselect, loglike


def ubm_statistics_host(feats: np.ndarray, ubm, gselect: Optional[np.ndarray] = None, frame_weight: Optional[np.ndarray] = None,
                        into: Optional[GmmStats] = None, want_post: bool = False):
    """``ubm_statistics`` on the host twin (mfa_debug_ubm_acc_host: frames in ascending index, plain loops): the specification
    the device is held to.  numpy arrays in; with ``want_post`` also returns the posteriors [T, n]."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    if feats.ndim != 2 or (feats.shape[0] and feats.shape[1] != ubm.dim):
        raise _lib.MfaHipError(f"ubm_statistics_host: features {feats.shape} for a model of dim {ubm.dim}")
    G, D, T = ubm.num_gauss, ubm.dim, int(feats.shape[0])
    st = into if into is not None else GmmStats.zeros(G, D, 1)
    if st.mean_acc.shape != (G, D):
        raise ValueError("ubm_statistics_host: `into` does not fit the model")
    gc, mi, iv = ubm.arrays()
    n = 0
    if gselect is not None:
        gselect = np.ascontiguousarray(gselect, dtype=np.int32)
        if gselect.ndim != 2 or gselect.shape[0] != T:
            raise _lib.MfaHipError(f"ubm_statistics_host: a selection of shape {gselect.shape} for {T} frames")
        n = int(gselect.shape[1])
    elif want_post:
        raise _lib.MfaHipError("ubm_statistics_host: want_post needs gselect")
    fw = None if frame_weight is None else np.ascontiguousarray(frame_weight, dtype=np.float32)
    if fw is not None and fw.shape != (T,):
        raise _lib.MfaHipError("ubm_statistics_host: one frame weight per frame")
    acc = accumulators(st)
    post = np.zeros((T, n), dtype=np.float32) if want_post else None
    twin_call("mfa_debug_ubm_acc_host", _UBM_TWIN_CODES, feats, T, int(mi.shape[1]), int(gc.shape[0]), gc, mi, iv, n, gselect, fw, *acc, post)
    store_accumulators(st, acc)
    return (st, post) if want_post else st


# ---- i-vector extractor: pruning, utterance statistics, E-step (include/mfa_hip.h "I-vector extractor") ------------------------
_IVEC_TWIN_CODES = {-2: "feature dimension outside [1, 48]", -3: "Gaussians outside [1, 2048]", -4: "entries per frame outside [1, 64]",
                    -5: "2^31 frames or utterances or more", -6: "i-vector dimension outside [1, 192]"}


def _ivec_frame_off(frame_off, total: int, what: str) -> np.ndarray:
    off = np.ascontiguousarray(frame_off, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise _lib.MfaHipError(f"{what}: frame offsets must ascend from 0 to the {total} frames of the batch")
    return off


def prune_posteriors(engine, post: torch.Tensor, min_post: float, scale: float = 1.0, inplace: bool = False) -> torch.Tensor:
    """gauss-to-post's pruning of ``post`` (float32 [T, n] on the device, a selection's softmax as ``ubm_statistics`` writes it
    with ``want_post``): entries below ``min_post`` dropped (the frame's first largest kept when that drops all), the survivors
    renormalised and multiplied by ``scale`` (mfa_ivector_prune_post_batch)."""
    if not isinstance(post, torch.Tensor) or post.dtype != torch.float32 or not post.is_cuda or post.dim() != 2:
        raise _lib.MfaHipError("prune_posteriors: posteriors must be a float32 [frames, n] tensor on the device")
    post = post.contiguous()
    out = post if inplace else torch.empty_like(post)
    engine._launch_ivector_prune(post, min_post, scale, out)
    return out


def prune_posteriors_host(post: np.ndarray, min_post: float, scale: float = 1.0) -> np.ndarray:
    """``prune_posteriors`` on the host twin: the same function the kernel runs, so the same float32 bits."""
    post = np.ascontiguousarray(post, dtype=np.float32)
    if post.ndim != 2:
        raise _lib.MfaHipError("prune_posteriors_host: posteriors must be a [frames, n] matrix")
    out = np.empty_like(post)
    twin_call("mfa_debug_ivector_prune_post_host", _IVEC_TWIN_CODES, post, int(post.shape[0]), int(post.shape[1]), float(min_post), float(scale), out)
    return out


def ivector_utterance_statistics(engine, feats: torch.Tensor, frame_off, gselect: torch.Tensor, post: torch.Tensor, num_gauss: int,
                                 max_count: float = 0.0, S: Optional[torch.Tensor] = None, want_S: bool = False):
    """Per-utterance γ [U, G] and X [U, G, D] (float64 on the device, where they stay for the E-steps) of the utterances
    ``frame_off`` (host int64 [U + 1]) cuts ``feats`` (float32 [T, D] on the device) into, from each frame's ``gselect`` row and
    pruned ``post`` row (mfa_ivector_utt_stats_batch).  ``S``: a float64 [G, D (D + 1) / 2] device tensor to add the global
    second-order statistics to (``want_S``: start one from zero).  ``max_count`` > 0 scales an utterance down to that count
    (extraction).  Returns (γ, X, S or None)."""
    if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or not feats.is_cuda or feats.dim() != 2:
        raise _lib.MfaHipError("ivector_utterance_statistics: features must be a float32 matrix on the device")
    feats = feats.contiguous()
    T, D, G, dev = int(feats.shape[0]), int(feats.shape[1]), int(num_gauss), engine.device
    off = _ivec_frame_off(frame_off, T, "ivector_utterance_statistics")
    for name, t, dt in (("selection", gselect, torch.int32), ("posteriors", post, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or t.dim() != 2 or t.shape[0] != T:
            raise _lib.MfaHipError(f"ivector_utterance_statistics: the {name} must be a {dt} [frames, n] tensor on the device")
    if gselect.shape != post.shape:
        raise _lib.MfaHipError("ivector_utterance_statistics: selection and posteriors differ in shape")
    U = off.shape[0] - 1
    gamma = torch.empty((U, G), dtype=torch.float64, device=dev)
    X = torch.empty((U, G, D), dtype=torch.float64, device=dev)
    if S is None and want_S:
        S = torch.zeros((G, D * (D + 1) // 2), dtype=torch.float64, device=dev)
    if S is not None and (S.dtype != torch.float64 or not S.is_cuda or tuple(S.shape) != (G, D * (D + 1) // 2) or not S.is_contiguous()):
        raise _lib.MfaHipError("ivector_utterance_statistics: S must be a contiguous float64 [G, D (D + 1) / 2] tensor on the device")
    engine._launch_ivector_utt_stats(feats, torch.from_numpy(off).to(dev), U, G, gselect.contiguous(), post.contiguous(), max_count,
                                     gamma, X, S)
    return gamma, X, S


def ivector_utterance_statistics_host(feats: np.ndarray, frame_off, gselect: np.ndarray, post: np.ndarray, num_gauss: int,
                                      max_count: float = 0.0, S: Optional[np.ndarray] = None, want_S: bool = False):
    """``ivector_utterance_statistics`` on the host twin (plain loops, utterances and frames ascending): numpy in and out."""
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    if feats.ndim != 2:
        raise _lib.MfaHipError("ivector_utterance_statistics_host: features must be a matrix")
    T, D, G = int(feats.shape[0]), int(feats.shape[1]), int(num_gauss)
    off = _ivec_frame_off(frame_off, T, "ivector_utterance_statistics_host")
    gselect = np.ascontiguousarray(gselect, dtype=np.int32)
    post = np.ascontiguousarray(post, dtype=np.float32)
    if gselect.ndim != 2 or gselect.shape[0] != T or gselect.shape != post.shape:
        raise _lib.MfaHipError("ivector_utterance_statistics_host: selection and posteriors must be [frames, n]")
    U = off.shape[0] - 1
    gamma, X = np.empty((U, G)), np.empty((U, G, D))
    if S is None and want_S:
        S = np.zeros((G, D * (D + 1) // 2))
    if S is not None and (S.dtype != np.float64 or S.shape != (G, D * (D + 1) // 2) or not S.flags.c_contiguous):
        raise _lib.MfaHipError("ivector_utterance_statistics_host: S must be a contiguous float64 [G, D (D + 1) / 2] array")
    twin_call("mfa_debug_ivector_utt_stats_host", _IVEC_TWIN_CODES, feats, off, U, D, G, int(gselect.shape[1]), gselect, post, float(max_count),
              gamma, X, S)
    return gamma, X, S


def ivector_estep(engine, model, gamma: torch.Tensor, X: torch.Tensor, into=None, want_var: bool = False):
    """The extractor's E-step over the utterances of ``gamma`` [U, G] / ``X`` [U, G, D] (float64 on the device) under ``model``
    (mfa_ivector_estep_batch).  ``into``: an ``ivector.IvectorStats`` whose Γ, Y, Rq, isum, iscat and n the device adds to
    (starting from its values) and whose ``quad`` / ``logdet`` take the utterances' sums; None is extraction.  Returns (μ [U, R],
    Var [U, P] or None, aux [U, 2] = (lin·μ, log det Q)), float64 on the device."""
    G, D, R = model.num_gauss, model.dim, model.ivector_dim
    for t, shape in ((gamma, (G,)), (X, (G, D))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or tuple(t.shape[1:]) != shape or not t.is_contiguous():
            raise _lib.MfaHipError(f"ivector_estep: statistics must be contiguous float64 [utterances, {', '.join(map(str, shape))}] tensors on the device")
    if gamma.shape[0] != X.shape[0]:
        raise _lib.MfaHipError("ivector_estep: gamma and X differ in their utterances")
    dev, U, P = engine.device, int(gamma.shape[0]), R * (R + 1) // 2
    W, Um = device_model(engine, model, model.derived)
    mean = torch.empty((U, R), dtype=torch.float64, device=dev)
    var = torch.empty((U, P), dtype=torch.float64, device=dev) if want_var else None
    aux = torch.empty((U, 2), dtype=torch.float64, device=dev)
    acc = None if into is None else tuple(torch.from_numpy(a).to(dev) for a in _ivec_accumulators(into, (G, D, R), "ivector_estep"))
    engine._launch_ivector_estep(gamma, X, W, Um, model.prior_offset, mean, var, aux, acc)
    if into is not None:
        _ivec_store(into, [t.cpu().numpy() for t in acc], aux.cpu().numpy(), gamma.cpu().numpy())
    return mean, var, aux


def _ivec_accumulators(into, shape, what: str):
    """The six accumulators of an ``ivector.IvectorStats`` (Γ, Y, Rq, isum, iscat, n) as contiguous float64 arrays."""
    if into.Y.shape != shape:
        raise ValueError(f"{what}: `into` does not fit the model")
    return [np.ascontiguousarray(a, dtype=np.float64) for a in (into.gamma, into.Y, into.Rq, into.isum, into.iscat, np.array([into.n]))]


def _ivec_store(into, acc, aux: np.ndarray, gamma: np.ndarray) -> None:
    """The accumulators back into ``into``, and onto its ``quad`` / ``logdet`` the objective's two sums over the utterances that
    took part (some γ not zero, a finite solve), utterances ascending."""
    into.gamma, into.Y, into.Rq, into.isum, into.iscat = acc[:5]
    into.n = float(acc[5][0])
    live = (gamma != 0).any(axis=1) & np.isfinite(aux).all(axis=1)
    into.quad += float(aux[live, 0].sum())
    into.logdet += float(aux[live, 1].sum())


def ivector_estep_host(model, gamma: np.ndarray, X: np.ndarray, into=None, want_var: bool = False):
    """``ivector_estep`` on the host twin (plain loops, utterances ascending): numpy in and out."""
    G, D, R = model.num_gauss, model.dim, model.ivector_dim
    gamma, X = np.ascontiguousarray(gamma, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64)
    if gamma.ndim != 2 or gamma.shape[1] != G or X.shape != (gamma.shape[0], G, D):
        raise _lib.MfaHipError("ivector_estep_host: statistics do not fit the model")
    U, P = int(gamma.shape[0]), R * (R + 1) // 2
    W, Um = model.derived()
    mean, aux = np.empty((U, R)), np.empty((U, 2))
    var = np.empty((U, P)) if want_var else None
    acc = [None] * 6 if into is None else _ivec_accumulators(into, (G, D, R), "ivector_estep_host")
    twin_call("mfa_debug_ivector_estep_host", _IVEC_TWIN_CODES, gamma, X, U, D, G, R, W, Um, float(model.prior_offset), mean, var, aux, *acc)
    if into is not None:
        _ivec_store(into, acc, aux, gamma)
    return mean, var, aux

