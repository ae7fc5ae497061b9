"""Statistics from alignments: per-speaker fMLLR statistics and GMM sufficient statistics (device call and host twin), with
the host-built tables they share.  Functions of an engine, not methods: they use its ``lib``, ``ctx``, ``device``, ``_dev``
and the loaded ``gmm``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, check
from .model import DiagGmmModel, TransitionModel
from .ragged import _speaker_groups


def model_arrays(gmm: DiagGmmModel) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """A model as the library takes it: contiguous (pdf_offsets int32, gconsts, means_invvars, inv_vars float32).  The caller
    keeps them alive across the call it passes their addresses to."""
    return (np.ascontiguousarray(gmm.pdf_offsets, dtype=np.int32), np.ascontiguousarray(gmm.gconsts, dtype=np.float32),
            np.ascontiguousarray(gmm.means_invvars, dtype=np.float32), np.ascontiguousarray(gmm.inv_vars, dtype=np.float32))


def check_delta_fmllr(fmllr, dim: int, utt2spk) -> None:
    """Host check of the per-speaker transforms of the Δ+ΔΔ path before a launch: float32, contiguous, on the device,
    [n_spk, 3·dim, 3·dim+1], a row for every speaker ``utt2spk`` names (row 0 without ``utt2spk``).  The kernel indexes the
    array by these numbers alone."""
    D = 3 * int(dim)
    if not isinstance(fmllr, torch.Tensor) or fmllr.dtype != torch.float32:
        raise _lib.MfaHipError(f"features: fMLLR transforms must be a float32 tensor (got {getattr(fmllr, 'dtype', type(fmllr))})")
    if fmllr.dim() != 3 or tuple(fmllr.shape[1:]) != (D, D + 1):
        raise _lib.MfaHipError(f"features: fMLLR transforms of shape {tuple(fmllr.shape)} do not fit Δ+ΔΔ features of dimension {D}: "
                               f"expected [n_spk, {D}, {D + 1}]")
    if not fmllr.is_contiguous():
        raise _lib.MfaHipError("features: fMLLR transforms must be contiguous")
    u2s = None if utt2spk is None else np.asarray(utt2spk)
    if u2s is not None and u2s.size and int(u2s.min()) < 0:
        raise _lib.MfaHipError("features: negative speaker row in utt2spk")
    need = 1 if u2s is None or u2s.size == 0 else int(u2s.max()) + 1
    if fmllr.shape[0] < need:
        raise _lib.MfaHipError(f"features: {fmllr.shape[0]} fMLLR transforms for speaker rows up to {need - 1}")
    if not fmllr.is_cuda:
        raise _lib.MfaHipError("features: fMLLR transforms must be on the device")


def tid_tables(tm: TransitionModel, weights: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The two host-built tables of the statistics calls: pdf of every transition-id (int32; index 0 unused) and its frame
    weight (float32; 1 for every id but 0 unless ``weights`` [transition-ids + 1] is given)."""
    id2pdf = np.maximum(tm.id2pdf, 0).astype(np.int32)
    w = np.ones(id2pdf.shape[0], dtype=np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32).copy()
    if w.shape != id2pdf.shape:
        raise ValueError(f"weights: {w.shape[0]} entries for {id2pdf.shape[0] - 1} transition-ids (+ 1)")
    w[0] = 0.0
    return id2pdf, w


def silence_weights(tm: TransitionModel, silence_phones: Sequence[int], silence_weight: float) -> np.ndarray:
    """Frame weight of every transition-id for fMLLR statistics: ``silence_weight`` for the silence phones' ids, 1 elsewhere."""
    sil = np.isin(tm.id2phone, np.asarray(list(silence_phones), dtype=np.int64))
    return np.where(sil, np.float32(silence_weight), np.float32(1.0))


def fmllr_statistics(engine, feats: torch.Tensor, frame_off: np.ndarray, ali: torch.Tensor,
                     tm: TransitionModel, utt2spk: np.ndarray, silence_phones: Sequence[int], silence_weight: float = 0.0,
                     stats_model: Optional[DiagGmmModel] = None):
    """Per-speaker fMLLR statistics from first-pass alignments (mfa_fmllr_acc_batch).

    ``ali``: int32 [ΣT] transition-ids (0 where an utterance failed: those frames get weight 0).  Returns
    (speaker ids, beta [S], K [S,D,D+1], G [S,D,D+1,D+1]) as float64 numpy arrays.

    ``stats_model``: the two-model form the reference runs for models that ship ``final.alimdl``
    (FmllrComputer(ali_model_path, model_path, …), MFA/corpus/features.py:503-511): posteriors from the model loaded in the
    engine (the alignment model), statistics with ``stats_model``'s means and variances (``final.mdl``)."""
    dev = engine.device
    if stats_model is not None:
        po, _gc, mi, iv = model_arrays(stats_model)
        check(engine.ctx, engine.lib.mfa_fmllr_stats_model(engine.ctx, stats_model.dim, stats_model.num_pdfs, po.ctypes.data,
                                                           mi.ctypes.data, iv.ctypes.data), "mfa_fmllr_stats_model")
    else:
        check(engine.ctx, engine.lib.mfa_fmllr_stats_model(engine.ctx, 0, 0, None, None, None), "mfa_fmllr_stats_model")
    id2pdf, w = tid_tables(tm, silence_weights(tm, silence_phones, silence_weight))
    id2pdf, w_of_tid = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    ali = ali.to(torch.int32).contiguous() if ali.dtype != torch.int32 else ali.contiguous()
    pdf = torch.empty(ali.shape[0], dtype=torch.int32, device=dev)       # scratch: the lookup runs inside the library
    weight = torch.empty(ali.shape[0], dtype=torch.float32, device=dev)
    spk_ids, _inv, order, spk_off = _speaker_groups(utt2spk)
    n_spk = len(spk_ids)
    D = feats.shape[1]
    beta = torch.zeros(n_spk, dtype=torch.float64, device=dev)
    K = torch.zeros((n_spk, D, D + 1), dtype=torch.float64, device=dev)
    G = torch.zeros((n_spk, D, D + 1, D + 1), dtype=torch.float64, device=dev)
    d_fo, d_so, d_su = engine._dev(frame_off), engine._dev(spk_off), engine._dev(order)
    check(engine.ctx, engine.lib.mfa_fmllr_acc_ali_batch(engine.ctx, _ptr(feats), _ptr(d_fo), len(frame_off) - 1,
                                                          int(frame_off[-1]), _ptr(ali), _ptr(id2pdf), _ptr(w_of_tid),
                                                          int(id2pdf.shape[0]), _ptr(pdf), _ptr(weight), _ptr(d_so), _ptr(d_su),
                                                          n_spk, _ptr(beta), _ptr(K), _ptr(G)), "mfa_fmllr_acc_ali_batch")
    return spk_ids, beta.cpu().numpy(), K.cpu().numpy(), G.cpu().numpy()


@dataclass
class GmmStats:
    """GMM sufficient statistics, indexed by model Gaussian (``DiagGmmModel.pdf_offsets``): float64 ``occ`` [G], ``mean_acc`` /
    ``var_acc`` [G, dim], ``tot_like`` = Σ w·loglike, ``tot_count`` = Σ w, int64 ``tid_count`` [transition-ids + 1].  Additive:
    ``a += b`` (AccumAmDiagGmm::Add); what a sum over batches, or later over ranks, needs."""

    occ: np.ndarray
    mean_acc: np.ndarray
    var_acc: np.ndarray
    tot_like: float
    tot_count: float
    tid_count: np.ndarray

    @classmethod
    def zeros(cls, num_gauss: int, dim: int, n_tids: int) -> "GmmStats":
        return cls(np.zeros(num_gauss), np.zeros((num_gauss, dim)), np.zeros((num_gauss, dim)), 0.0, 0.0, np.zeros(n_tids, dtype=np.int64))

    def copy(self) -> "GmmStats":
        return GmmStats(self.occ.copy(), self.mean_acc.copy(), self.var_acc.copy(), self.tot_like, self.tot_count, self.tid_count.copy())

    def __iadd__(self, other: "GmmStats") -> "GmmStats":
        if self.mean_acc.shape != other.mean_acc.shape or self.tid_count.shape != other.tid_count.shape:
            raise ValueError("GmmStats of different models cannot be added")
        self.occ += other.occ
        self.mean_acc += other.mean_acc
        self.var_acc += other.var_acc
        self.tot_like += other.tot_like
        self.tot_count += other.tot_count
        self.tid_count += other.tid_count
        return self

    @property
    def loglike_per_frame(self) -> float:
        """What the reference logs after accumulation: total log-likelihood over total weight."""
        return self.tot_like / self.tot_count if self.tot_count else 0.0


def gmm_statistics(engine, feats: torch.Tensor, ali: torch.Tensor, tm: TransitionModel,
                   weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None) -> GmmStats:
    """GMM statistics of one batch from its alignments (mfa_gmm_acc_batch; the contract is in include/mfa_hip.h), with the
    model loaded in the engine.

    ``feats`` float32 [ΣT, dim] and ``ali`` int32 [ΣT] transition-ids on the device (0 where an utterance failed: those frames
    take no part); ``weights``: per transition-id frame weights (default 1).  ``into``: statistics to add to — the device sums
    start from its values, so a corpus accumulated batch by batch is one chain of additions — and the object returned."""
    return _gmm_statistics(engine, feats, None, ali, tm, weights, into, "gmm_statistics")


def gmm_statistics_twofeats(engine, feats_post: torch.Tensor, feats_sum: torch.Tensor, ali: torch.Tensor, tm: TransitionModel,
                            weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None) -> GmmStats:
    """GMM statistics from two feature matrices of the same frames (mfa_gmm_acc_twofeats_batch; Kaldi
    gmm-acc-stats-twofeats): posteriors and log-likelihood from ``feats_post``, the first- and second-order sums from
    ``feats_sum``.  Everything else as ``gmm_statistics``.  What builds ``final.alimdl``: posteriors on the speaker-adapted
    features, sums of the unadapted ones."""
    if not isinstance(feats_sum, torch.Tensor) or not isinstance(feats_post, torch.Tensor):
        raise _lib.MfaHipError("gmm_statistics_twofeats: both feature matrices must be tensors on the device")
    if tuple(feats_sum.shape) != tuple(feats_post.shape) or feats_sum.dtype != feats_post.dtype:
        raise _lib.MfaHipError(f"gmm_statistics_twofeats: the matrices differ: {tuple(feats_post.shape)} {feats_post.dtype} for the "
                               f"posteriors, {tuple(feats_sum.shape)} {feats_sum.dtype} for the sums")
    if feats_sum.device != feats_post.device:
        raise _lib.MfaHipError(f"gmm_statistics_twofeats: the matrices are on different devices ({feats_post.device}, {feats_sum.device})")
    return _gmm_statistics(engine, feats_post, feats_sum, ali, tm, weights, into, "gmm_statistics_twofeats")


def _gmm_statistics(engine, feats, feats_sum, ali, tm, weights, into, what) -> GmmStats:
    if engine.gmm is None:
        raise _lib.MfaHipError(f"{what}: no acoustic model loaded (AlignmentEngine.load_gmm)")
    dev = engine.device
    gmm = engine.gmm
    G, D = gmm.num_gauss, gmm.dim
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    st = into if into is not None else GmmStats.zeros(G, D, n_tids)
    if st.mean_acc.shape != (G, D) or st.tid_count.shape != (n_tids,):
        raise ValueError(f"{what}: `into` does not fit the loaded model")
    total = int(ali.shape[0])
    if feats.shape[0] != total or (total and feats.shape[1] != D):
        raise _lib.MfaHipError(f"{what}: features {tuple(feats.shape)} for {total} frames of a model of dim {D}")
    if feats.dtype != torch.float32 or not feats.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError(f"{what}: features must be float32 and, like the alignments, on the device")
    feats = feats.contiguous()
    if feats_sum is not None:
        feats_sum = feats_sum.contiguous()
    ali = ali.to(torch.int32).contiguous()
    occ = torch.from_numpy(st.occ).to(dev)
    mean = torch.from_numpy(np.ascontiguousarray(st.mean_acc)).to(dev)
    var = torch.from_numpy(np.ascontiguousarray(st.var_acc)).to(dev)
    tot = torch.tensor([st.tot_like, st.tot_count], dtype=torch.float64, device=dev)
    cnt = torch.from_numpy(st.tid_count).to(dev)
    d_pdf, d_w = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    if feats_sum is None:
        check(engine.ctx, engine.lib.mfa_gmm_acc_batch(engine.ctx, _ptr(feats), total, _ptr(ali), _ptr(d_pdf), _ptr(d_w), n_tids,
                                                        _ptr(occ), _ptr(mean), _ptr(var), _ptr(tot), _ptr(cnt)), "mfa_gmm_acc_batch")
    else:
        check(engine.ctx, engine.lib.mfa_gmm_acc_twofeats_batch(engine.ctx, _ptr(feats), _ptr(feats_sum), total, _ptr(ali), _ptr(d_pdf),
                                                                 _ptr(d_w), n_tids, _ptr(occ), _ptr(mean), _ptr(var), _ptr(tot),
                                                                 _ptr(cnt)), "mfa_gmm_acc_twofeats_batch")
    st.occ, st.mean_acc, st.var_acc, st.tid_count = occ.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), cnt.cpu().numpy()
    t = tot.cpu().numpy()
    st.tot_like, st.tot_count = float(t[0]), float(t[1])
    return st


def gmm_statistics_host(gmm: DiagGmmModel, feats: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                        weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None, want_post: bool = False):
    """The same call on the host twin (mfa_debug_gmm_acc_host: no device, frames in ascending index): the specification the
    device is held to.  numpy arrays in; with ``want_post`` also returns every frame's posteriors [ΣT, largest pdf]."""
    return _gmm_statistics_host(gmm, feats, None, ali, tm, weights, into, want_post)


def gmm_statistics_twofeats_host(gmm: DiagGmmModel, feats_post: np.ndarray, feats_sum: np.ndarray, ali: np.ndarray,
                                 tm: TransitionModel, weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None,
                                 want_post: bool = False):
    """``gmm_statistics_twofeats`` on the host twin (mfa_debug_gmm_acc_twofeats_host): posteriors from ``feats_post``, sums
    from ``feats_sum``."""
    if feats_sum is None:
        raise _lib.MfaHipError("gmm_statistics_twofeats_host: no matrix to form the sums from")
    if np.shape(feats_sum) != np.shape(feats_post):
        raise _lib.MfaHipError(f"gmm_statistics_twofeats_host: the matrices differ in shape: {np.shape(feats_post)}, {np.shape(feats_sum)}")
    return _gmm_statistics_host(gmm, feats_post, feats_sum, ali, tm, weights, into, want_post)


def _gmm_statistics_host(gmm, feats, feats_sum, ali, tm, weights, into, want_post):
    lib = _lib.lib()
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    G, D = gmm.num_gauss, gmm.dim
    st = into if into is not None else GmmStats.zeros(G, D, n_tids)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    ok = (ali > 0) & (ali < n_tids)
    safe = np.where(ok, ali, 0)
    pdf = np.where(ok, id2pdf[safe], -1).astype(np.int32)
    fw = np.where(ok, w[safe], np.float32(0)).astype(np.float32)
    po, gc, mi, iv = model_arrays(gmm)
    occ, mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (st.occ, st.mean_acc, st.var_acc))
    tot = np.array([st.tot_like, st.tot_count], dtype=np.float64)
    cnt = np.ascontiguousarray(st.tid_count, dtype=np.int64)
    stride = int(np.diff(po).max())
    post = np.zeros((ali.shape[0], stride), dtype=np.float32) if want_post else None
    tail = (int(ali.shape[0]), pdf.ctypes.data, fw.ctypes.data, ali.ctypes.data, n_tids, occ.ctypes.data, mean.ctypes.data,
            var.ctypes.data, tot.ctypes.data, cnt.ctypes.data, None if post is None else post.ctypes.data, stride)
    if feats_sum is None:
        rc = lib.mfa_debug_gmm_acc_host(D, gmm.num_pdfs, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data,
                                        feats.ctypes.data, *tail)
    else:
        feats_sum = np.ascontiguousarray(feats_sum, dtype=np.float32)
        rc = lib.mfa_debug_gmm_acc_twofeats_host(D, gmm.num_pdfs, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data,
                                                 feats.ctypes.data, feats_sum.ctypes.data, *tail)
    if rc != 0:
        raise _lib.MfaHipError(f"mfa_debug_gmm_acc{'_twofeats' if feats_sum is not None else ''}_host: {'a pdf of more than 128 Gaussians' if rc == -2 else 'bad arguments'}")
    st.occ, st.mean_acc, st.var_acc, st.tid_count = occ, mean, var, cnt
    st.tot_like, st.tot_count = float(tot[0]), float(tot[1])
    return (st, post) if want_post else st


@dataclass
class LdaStats:
    """LDA scatter statistics in the spliced space (mfa_lda_acc_batch; Kaldi LdaEstimate): float64 ``zero`` [C] = Σ w per
    class, ``first`` [C, S] = Σ w·x, ``second`` [S, S] = Σ w·x·xᵀ (symmetric, both triangles held).  Additive: ``a += b``."""

    zero: np.ndarray
    first: np.ndarray
    second: np.ndarray

    @classmethod
    def zeros(cls, num_classes: int, dim: int) -> "LdaStats":
        return cls(np.zeros(num_classes), np.zeros((num_classes, dim)), np.zeros((dim, dim)))

    def copy(self) -> "LdaStats":
        return LdaStats(self.zero.copy(), self.first.copy(), self.second.copy())

    def __iadd__(self, other: "LdaStats") -> "LdaStats":
        if self.first.shape != other.first.shape:
            raise ValueError("LdaStats of different shapes cannot be added")
        self.zero += other.zero
        self.first += other.first
        self.second += other.second
        return self

    @property
    def num_classes(self) -> int:
        return int(self.first.shape[0])

    @property
    def dim(self) -> int:
        return int(self.first.shape[1])


def _lda_tables(tm, weights, num_classes):
    """The class and weight of every transition-id: a ``TransitionModel`` (classes are its pdfs, ``tid_tables``) or a ready
    pair (tid2class int32, tid_weight float32) with ``num_classes``."""
    if hasattr(tm, "id2pdf"):
        id2class, w = tid_tables(tm, weights)
        C = int(num_classes) if num_classes is not None else int(getattr(tm, "num_pdfs", int(id2class.max()) + 1))
    else:
        id2class = np.ascontiguousarray(tm[0], dtype=np.int32)
        w = np.ascontiguousarray(tm[1], dtype=np.float32)
        if weights is not None:
            raise ValueError("lda_statistics: `weights` goes with a TransitionModel; a (tid2class, tid_weight) pair carries its own")
        if num_classes is None:
            raise ValueError("lda_statistics: a (tid2class, tid_weight) pair needs num_classes")
        C = int(num_classes)
    if id2class.shape != w.shape or id2class.ndim != 1:
        raise ValueError("lda_statistics: tid2class and tid_weight must be vectors of one length")
    return id2class, w, C


def _lda_prune_args(rand_prune, utt_keys, n_utt):
    rand_prune = float(rand_prune)
    if rand_prune < 0:
        raise ValueError("lda_statistics: rand_prune must be >= 0")
    if rand_prune > 0 and utt_keys is None:
        raise ValueError("lda_statistics: rand_prune needs utt_keys (the utterances' corpus positions)")
    keys = None if utt_keys is None else np.ascontiguousarray(utt_keys, dtype=np.uint32)
    if keys is not None and keys.shape != (n_utt,):
        raise ValueError(f"lda_statistics: {keys.shape} utterance keys for {n_utt} utterances")
    return rand_prune, keys


def lda_statistics(engine, mfcc: torch.Tensor, frame_off: np.ndarray, utt2spk, cmvn, ali: torch.Tensor, tm,
                   splice_context: int = 3, weights: Optional[np.ndarray] = None, rand_prune: float = 0.0, utt_keys=None,
                   seed: int = 0, into: Optional[LdaStats] = None, num_classes: Optional[int] = None,
                   tid_count: Optional[np.ndarray] = None) -> LdaStats:
    """LDA statistics of one batch from its alignments (mfa_lda_acc_batch; the contract is in include/mfa_hip.h).

    ``mfcc`` float32 [ΣT, dim] base features and ``ali`` int32 [ΣT] transition-ids on the device; ``utt2spk`` / ``cmvn``
    (float64 [n_spk, 2, dim+1] on the device, or None) as ``AlignmentEngine.final_features`` takes them.  Classes are the pdfs
    of ``tm`` with per transition-id ``weights`` (``silence_weights(tm, silence_phones, 0.0)`` is the reference's
    weight-silence-post 0.0); ``tm`` may also be a ready (tid2class, tid_weight) pair with ``num_classes``.  ``rand_prune``
    with ``utt_keys`` (corpus positions) and ``seed``: Kaldi's RandPrune on counter-based draws.  ``into``: statistics to add
    to, and the object returned.  ``tid_count``: optional int64 [transition-ids + 1] counts to add to (returned in place)."""
    dev = engine.device
    id2class, w, C = _lda_tables(tm, weights, num_classes)
    n_tids = int(id2class.shape[0])
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    n_utt, total = len(frame_off) - 1, int(frame_off[-1])
    if mfcc.dim() != 2 or mfcc.shape[0] != total or ali.shape[0] != total:
        raise _lib.MfaHipError(f"lda_statistics: features {tuple(mfcc.shape)} and {ali.shape[0]} alignment frames for {total} frames")
    if mfcc.dtype != torch.float32 or not mfcc.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError("lda_statistics: features must be float32 and, like the alignments, on the device")
    dim = int(mfcc.shape[1])
    S = (2 * int(splice_context) + 1) * dim
    st = into if into is not None else LdaStats.zeros(C, max(S, 0))
    if st.first.shape != (C, S) or st.second.shape != (S, S):
        raise ValueError("lda_statistics: `into` does not fit the classes and the spliced dimension")
    rand_prune, keys = _lda_prune_args(rand_prune, utt_keys, n_utt)
    mfcc = mfcc.contiguous()
    ali = ali.to(torch.int32).contiguous()
    d_u2s = None if utt2spk is None else engine._dev(np.ascontiguousarray(utt2spk, dtype=np.int32))
    if cmvn is not None and (cmvn.dtype != torch.float64 or not cmvn.is_cuda):
        raise _lib.MfaHipError("lda_statistics: CMVN statistics must be float64 on the device")
    d_cmvn = None if cmvn is None else cmvn.contiguous()
    zero = torch.from_numpy(np.ascontiguousarray(st.zero)).to(dev)
    first = torch.from_numpy(np.ascontiguousarray(st.first)).to(dev)
    second = torch.from_numpy(np.ascontiguousarray(st.second)).to(dev)
    cnt = None if tid_count is None else torch.from_numpy(np.ascontiguousarray(tid_count, dtype=np.int64)).to(dev)
    d_cls, d_w = torch.from_numpy(id2class).to(dev), torch.from_numpy(w).to(dev)
    d_keys = None if keys is None else torch.from_numpy(keys.view(np.int32)).to(dev)
    d_fo = engine._dev(frame_off)
    check(engine.ctx, engine.lib.mfa_lda_acc_batch(engine.ctx, _ptr(mfcc), _ptr(d_fo), n_utt, total, dim, _ptr(d_u2s), _ptr(d_cmvn),
                                                    int(splice_context), _ptr(ali), _ptr(d_cls), _ptr(d_w), n_tids, C, rand_prune,
                                                    _ptr(d_keys), int(seed) & 0xFFFFFFFF, _ptr(zero), _ptr(first), _ptr(second),
                                                    _ptr(cnt)), "mfa_lda_acc_batch")
    st.zero, st.first, st.second = zero.cpu().numpy(), first.cpu().numpy(), second.cpu().numpy()
    if cnt is not None:
        tid_count[...] = cnt.cpu().numpy()
    return st


def lda_statistics_host(mfcc: np.ndarray, frame_off: np.ndarray, utt2spk, cmvn, ali: np.ndarray, tm, splice_context: int = 3,
                        weights: Optional[np.ndarray] = None, rand_prune: float = 0.0, utt_keys=None, seed: int = 0,
                        into: Optional[LdaStats] = None, num_classes: Optional[int] = None,
                        tid_count: Optional[np.ndarray] = None) -> LdaStats:
    """The same call on the host twin (mfa_debug_lda_acc_host: no device, frames in ascending index): the specification the
    device is held to.  numpy arrays in."""
    lib = _lib.lib()
    id2class, w, C = _lda_tables(tm, weights, num_classes)
    n_tids = int(id2class.shape[0])
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    n_utt, total = len(frame_off) - 1, int(frame_off[-1])
    mfcc = np.ascontiguousarray(mfcc, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    if mfcc.ndim != 2 or mfcc.shape[0] != total or ali.shape[0] != total:
        raise _lib.MfaHipError(f"lda_statistics_host: features {mfcc.shape} and {ali.shape[0]} alignment frames for {total} frames")
    dim = int(mfcc.shape[1])
    S = (2 * int(splice_context) + 1) * dim
    st = into if into is not None else LdaStats.zeros(C, max(S, 0))
    if st.first.shape != (C, S) or st.second.shape != (S, S):
        raise ValueError("lda_statistics_host: `into` does not fit the classes and the spliced dimension")
    rand_prune, keys = _lda_prune_args(rand_prune, utt_keys, n_utt)
    u2s = None if utt2spk is None else np.ascontiguousarray(utt2spk, dtype=np.int32)
    cm = None if cmvn is None else np.ascontiguousarray(cmvn, dtype=np.float64)
    zero, first, second = (np.ascontiguousarray(a, dtype=np.float64) for a in (st.zero, st.first, st.second))
    cnt = None if tid_count is None else np.ascontiguousarray(tid_count, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.mfa_debug_lda_acc_host(p(mfcc), p(frame_off), n_utt, dim, p(u2s), p(cm), int(splice_context), p(ali), p(id2class), p(w),
                                    n_tids, C, rand_prune, p(keys), int(seed) & 0xFFFFFFFF, p(zero), p(first), p(second), p(cnt))
    if rc != 0:
        why = {-2: "spliced dimension above 128", -3: "2^31 frames or more"}.get(rc, "bad arguments")
        raise _lib.MfaHipError(f"mfa_debug_lda_acc_host: {why}")
    st.zero, st.first, st.second = zero, first, second
    if cnt is not None:
        tid_count[...] = cnt
    return st


def gaussian_means(gmm: DiagGmmModel) -> np.ndarray:
    """The Gaussians' means as the MLLT statistics take them: ``means_invvars / inv_vars`` in float32, formed once and handed
    to the device and to the host twin alike."""
    return np.ascontiguousarray(np.asarray(gmm.means_invvars, dtype=np.float32) / np.asarray(gmm.inv_vars, dtype=np.float32))


class MlltStats:
    """MLLT statistics, indexed by model Gaussian (mfa_mllt_acc_batch): float64 ``occ`` [G], ``full`` [G, D, D] = Σ γ·d·dᵀ with
    d = x − μ_g (symmetric, both triangles held), ``tot_like`` = Σ w·loglike, ``tot_count`` = Σ w.  Additive: ``a += b``.

    ``full`` is hundreds of megabytes for a real model, so during a device pass the accumulators live in device tensors:
    ``mllt_statistics(into=)`` adds to them in place, batch after batch, and nothing crosses to the host until ``occ``,
    ``full``, ``tot_like`` or ``tot_count`` is read — once, after the pass.  Host arrays handed in (``zeros``, a copy, the
    result of ``+=``) go to the device at the next ``mllt_statistics`` call and stay there."""

    def __init__(self, occ: np.ndarray, full: np.ndarray, tot_like: float = 0.0, tot_count: float = 0.0):
        self._occ = np.ascontiguousarray(occ, dtype=np.float64)
        self._full = np.ascontiguousarray(full, dtype=np.float64)
        if self._full.ndim != 3 or self._full.shape[0] != self._occ.shape[0] or self._full.shape[1] != self._full.shape[2]:
            raise ValueError(f"MlltStats: occ {self._occ.shape} and full {self._full.shape} are not [G] and [G, D, D]")
        self._tot = np.array([tot_like, tot_count], dtype=np.float64)
        self._shape = tuple(self._full.shape)
        self._dev = None          # (occ, full, tot) device tensors, or None
        self._dev_newer = False   # the device tensors hold sums the host arrays do not

    @classmethod
    def zeros(cls, num_gauss: int, dim: int) -> "MlltStats":
        return cls(np.zeros(num_gauss), np.zeros((num_gauss, dim, dim)))

    @property
    def shape(self) -> Tuple[int, int, int]:
        return self._shape

    def _host(self) -> None:
        if self._dev_newer:
            occ, full, tot = self._dev
            self._occ, self._full, self._tot = occ.cpu().numpy(), full.cpu().numpy(), tot.cpu().numpy()
            self._dev_newer = False

    def _device(self, dev):
        """The accumulators as device tensors to add to; the host copies are stale from here on."""
        if self._dev is None or self._dev[0].device != torch.device(dev):
            self._host()
            self._dev = tuple(torch.from_numpy(a).to(dev) for a in (self._occ, self._full, self._tot))
        self._dev_newer = True
        return self._dev

    @property
    def occ(self) -> np.ndarray:
        self._host()
        return self._occ

    @property
    def full(self) -> np.ndarray:
        self._host()
        return self._full

    @property
    def tot_like(self) -> float:
        self._host()
        return float(self._tot[0])

    @property
    def tot_count(self) -> float:
        self._host()
        return float(self._tot[1])

    def copy(self) -> "MlltStats":
        return MlltStats(self.occ.copy(), self.full.copy(), self.tot_like, self.tot_count)

    def __iadd__(self, other: "MlltStats") -> "MlltStats":
        if self.shape != other.shape:
            raise ValueError("MlltStats of different models cannot be added")
        self._host()
        self._occ += other.occ
        self._full += other.full
        self._tot += np.array([other.tot_like, other.tot_count])
        self._dev = None          # the host arrays are the value now
        return self

    @property
    def loglike_per_frame(self) -> float:
        return self.tot_like / self.tot_count if self.tot_count else 0.0


def mllt_statistics(engine, feats: torch.Tensor, ali: torch.Tensor, tm: TransitionModel,
                    weights: Optional[np.ndarray] = None, into: Optional[MlltStats] = None) -> MlltStats:
    """MLLT statistics of one batch from its alignments (mfa_mllt_acc_batch; the contract is in include/mfa_hip.h), with the
    model loaded in the engine.  Arguments as ``gmm_statistics``.  ``into``: statistics to add to, and the object returned;
    its accumulators stay on the device between calls (``MlltStats``)."""
    if engine.gmm is None:
        raise _lib.MfaHipError("mllt_statistics: no acoustic model loaded (AlignmentEngine.load_gmm)")
    dev = engine.device
    gmm = engine.gmm
    G, D = gmm.num_gauss, gmm.dim
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    st = into if into is not None else MlltStats.zeros(G, D)
    if st.shape != (G, D, D):
        raise ValueError("mllt_statistics: `into` does not fit the loaded model")
    total = int(ali.shape[0])
    if feats.shape[0] != total or (total and feats.shape[1] != D):
        raise _lib.MfaHipError(f"mllt_statistics: features {tuple(feats.shape)} for {total} frames of a model of dim {D}")
    if feats.dtype != torch.float32 or not feats.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError("mllt_statistics: features must be float32 and, like the alignments, on the device")
    feats = feats.contiguous()
    ali = ali.to(torch.int32).contiguous()
    means = torch.from_numpy(gaussian_means(gmm)).to(dev)
    d_pdf, d_w = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    occ, full, tot = st._device(dev)
    check(engine.ctx, engine.lib.mfa_mllt_acc_batch(engine.ctx, _ptr(feats), total, _ptr(ali), _ptr(d_pdf), _ptr(d_w), n_tids,
                                                     _ptr(means), _ptr(occ), _ptr(full), _ptr(tot)), "mfa_mllt_acc_batch")
    return st


def mllt_statistics_host(gmm: DiagGmmModel, feats: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                         weights: Optional[np.ndarray] = None, into: Optional[MlltStats] = None, want_post: bool = False):
    """The same call on the host twin (mfa_debug_mllt_acc_host: no device, frames in ascending index, plain loops): the
    specification the device is held to.  numpy arrays in; with ``want_post`` also returns every frame's posteriors."""
    lib = _lib.lib()
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    G, D = gmm.num_gauss, gmm.dim
    st = into if into is not None else MlltStats.zeros(G, D)
    if st.shape != (G, D, D):
        raise ValueError("mllt_statistics_host: `into` does not fit the model")
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    if feats.ndim != 2 or feats.shape[0] != ali.shape[0] or (ali.shape[0] and feats.shape[1] != D):
        raise _lib.MfaHipError(f"mllt_statistics_host: features {feats.shape} for {ali.shape[0]} frames of a model of dim {D}")
    ok = (ali > 0) & (ali < n_tids)
    safe = np.where(ok, ali, 0)
    pdf = np.where(ok, id2pdf[safe], -1).astype(np.int32)
    fw = np.where(ok, w[safe], np.float32(0)).astype(np.float32)
    po, gc, mi, iv = model_arrays(gmm)
    means = gaussian_means(gmm)
    st._host()
    occ, full, tot = st._occ, st._full, st._tot
    stride = int(np.diff(po).max())
    post = np.zeros((ali.shape[0], stride), dtype=np.float32) if want_post else None
    rc = lib.mfa_debug_mllt_acc_host(D, gmm.num_pdfs, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data,
                                     means.ctypes.data, feats.ctypes.data, int(ali.shape[0]), pdf.ctypes.data, fw.ctypes.data,
                                     occ.ctypes.data, full.ctypes.data, tot.ctypes.data,
                                     None if post is None else post.ctypes.data, stride)
    if rc != 0:
        why = {-2: "a pdf of more than 128 Gaussians", -3: "feature dimension above 48"}.get(rc, "bad arguments")
        raise _lib.MfaHipError(f"mfa_debug_mllt_acc_host: {why}")
    st._dev = None                # the host arrays are the value now
    return (st, post) if want_post else st


TREE_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
TREE_MAX_PHONES, TREE_MAX_CLASSES = 1 << 16, 256


def tree_key(left, centre, right, pdf_class) -> np.ndarray:
    """The event key of include/mfa_hip.h ("Tree statistics"): l << 48 | c << 28 | r << 8 | pc, uint64."""
    l, c, r, pc = (np.asarray(a, dtype=np.uint64) for a in (left, centre, right, pdf_class))
    return (l << np.uint64(48)) | (c << np.uint64(28)) | (r << np.uint64(8)) | pc


@dataclass
class TreeStats:
    """Tree statistics (mfa_tree_acc_batch; Kaldi acc-tree-stats): per event — (left, centre, right) phone window and
    pdf-class, packed in ``keys`` [E] uint64 ascending — int64 ``count`` [E] and float64 ``sum`` / ``sumsq`` [E, dim].
    Additive: ``a += b`` merges by key, float64 addition in call order."""

    keys: np.ndarray
    count: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray

    @classmethod
    def zeros(cls, dim: int) -> "TreeStats":
        return cls(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros((0, dim)), np.zeros((0, dim)))

    def copy(self) -> "TreeStats":
        return TreeStats(self.keys.copy(), self.count.copy(), self.sum.copy(), self.sumsq.copy())

    @property
    def dim(self) -> int:
        return int(self.sum.shape[1])

    @property
    def num_events(self) -> int:
        return int(self.keys.shape[0])

    def windows(self) -> np.ndarray:
        """[E, 3] int32: left, centre and right phone of every event."""
        k = self.keys
        return np.stack([k >> np.uint64(48), (k >> np.uint64(28)) & np.uint64(0xFFFFF), (k >> np.uint64(8)) & np.uint64(0xFFFFF)],
                        axis=1).astype(np.int32)

    def pdf_classes(self) -> np.ndarray:
        """[E] int32: the pdf-class of every event."""
        return (self.keys & np.uint64(0xFF)).astype(np.int32)

    def __iadd__(self, other: "TreeStats") -> "TreeStats":
        if self.dim != other.dim:
            raise ValueError("TreeStats of different feature dimensions cannot be added")
        keys = np.union1d(self.keys, other.keys)
        a, b = np.searchsorted(keys, self.keys), np.searchsorted(keys, other.keys)
        count = np.zeros(keys.shape[0], dtype=np.int64)
        s, q = np.zeros((keys.shape[0], self.dim)), np.zeros((keys.shape[0], self.dim))
        count[a] = self.count
        s[a], q[a] = self.sum, self.sumsq
        count[b] += other.count
        s[b] += other.sum
        q[b] += other.sumsq
        self.keys, self.count, self.sum, self.sumsq = keys, count, s, q
        return self


def tree_tid_tables(tm: TransitionModel, ci_phones: Sequence[int]):
    """The host-built tables of the tree statistics: per transition-id (int32 [transition-ids + 1]; index 0 unused) its phone,
    the pdf-class of its arc (the state's self-loop pdf-class for a self-loop, its forward pdf-class otherwise) and its flags
    (1: final, 2: self-loop); and uint8 [phones + 1] marking the context-independent phones.  Built once per transition
    model and set of context-independent phones, and kept on the model (it is called for every batch)."""
    cache = tm.__dict__.setdefault("_tree_tables", {})
    cache_key = tuple(sorted(int(p) for p in ci_phones))
    if cache_key in cache:
        return cache[cache_key]
    n = int(tm.id2phone.shape[0])
    phone = np.ascontiguousarray(tm.id2phone, dtype=np.int32)
    flags = np.ascontiguousarray((tm.is_final != 0) * 1 + (tm.is_self_loop != 0) * 2, dtype=np.int32)
    # the two pdf-classes of every transition-state (row 0 unused), then one gather over the transition-ids
    state_cls = np.zeros((tm.tuples.shape[0] + 1, 2), dtype=np.int32)
    for ts, row in enumerate(tm.tuples, start=1):
        st = tm.topo.entry_for_phone(int(row[0]))[int(row[1])]
        state_cls[ts] = (st.forward_pdf_class, st.self_loop_pdf_class)
    cls = np.ascontiguousarray(state_cls[tm.id2state, (tm.is_self_loop != 0).astype(np.int64)], dtype=np.int32)
    cls[0] = 0
    n_phones = int(max(int(phone.max()) if n > 1 else 0, int(np.max(tm.topo.phones)) if len(tm.topo.phones) else 0))
    if n_phones >= TREE_MAX_PHONES:
        raise _lib.MfaHipError(f"tree statistics: phone id {n_phones} (the event key holds phone ids below {TREE_MAX_PHONES})")
    if n > 1 and (int(cls[1:].max()) >= TREE_MAX_CLASSES or int(cls[1:].min()) < 0):
        raise _lib.MfaHipError(f"tree statistics: pdf-class outside [0, {TREE_MAX_CLASSES})")
    ci = np.zeros(n_phones + 1, dtype=np.uint8)
    for p in ci_phones:
        if not 0 < int(p) <= n_phones:
            raise _lib.MfaHipError(f"tree statistics: context-independent phone {int(p)} is not a phone of the model")
        ci[int(p)] = 1
    cache[cache_key] = (phone, cls, flags, ci)
    return cache[cache_key]


def _tree_device_tables(engine, tm: TransitionModel, ci_phones: Sequence[int]):
    """``tree_tid_tables`` with their copies on the engine's device, uploaded once per model."""
    tables = tree_tid_tables(tm, ci_phones)
    cache = tm.__dict__.setdefault("_tree_device_tables", {})
    key = (str(engine.device), id(tables))
    if key not in cache:
        cache[key] = tuple(torch.from_numpy(a).to(engine.device) for a in tables)
    return tables, cache[key]


def _tree_check(what, feat_shape, frame_off, n_ali, context_width, central_position):
    if (int(context_width), int(central_position)) != (3, 1):
        raise _lib.MfaHipError(f"{what}: context width {context_width} with central position {central_position}: only 3 and 1")
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    if frame_off.ndim != 1 or frame_off.shape[0] < 1 or frame_off[0] != 0 or np.any(np.diff(frame_off) < 0):
        raise _lib.MfaHipError(f"{what}: frame offsets must start at 0 and ascend")
    total = int(frame_off[-1])
    if len(feat_shape) != 2 or feat_shape[0] != total or n_ali != total:
        raise _lib.MfaHipError(f"{what}: features {tuple(feat_shape)} and {n_ali} alignment frames for {total} frames")
    return frame_off, len(frame_off) - 1, total


def _elem_ptr(t: torch.Tensor, index: int):
    """Element ``index`` of a 1-D tensor as the pointer argument of a library call."""
    return ctypes.c_void_p(t.data_ptr() + index * t.element_size())


def tree_statistics(engine, feats: torch.Tensor, frame_off: np.ndarray, ali: torch.Tensor, tm: TransitionModel,
                    ci_phones: Sequence[int] = (), context_width: int = 3, central_position: int = 1, cap: Optional[int] = None):
    """Tree statistics of one batch from its alignments (mfa_tree_acc_batch; the contract is in include/mfa_hip.h).

    ``feats`` float32 [ΣT, dim] and ``ali`` int32 [ΣT] transition-ids on the device; ``ci_phones``: the context-independent
    phones (the reference passes silence and OOV phones).  Returns (``TreeStats`` of the batch, ``frame_event`` int32 [ΣT] on
    the device: every frame's row in ``TreeStats.keys`` or −1, the number of utterances skipped).  ``cap``: event rows to
    offer first (default: what the engine's last call needed); the call is repeated when the batch has more."""
    frame_off, n_utt, total = _tree_check("tree_statistics", feats.shape, frame_off, int(ali.shape[0]), context_width, central_position)
    if feats.dtype != torch.float32 or not feats.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError("tree_statistics: features must be float32 and, like the alignments, on the device")
    dev = engine.device
    dim = int(feats.shape[1])
    (phone, cls, flags, ci), (d_phone, d_cls, d_flags, d_ci) = _tree_device_tables(engine, tm, ci_phones)
    feats = feats.contiguous()
    ali = ali.to(torch.int32).contiguous()
    d_fo = engine._dev(frame_off)
    frame_event = torch.empty(total, dtype=torch.int32, device=dev)
    scal = torch.zeros(2, dtype=torch.int64, device=dev)               # n_events, skipped
    cap = int(cap) if cap is not None else int(getattr(engine, "_tree_cap", 4096))
    while True:
        key = torch.empty(cap, dtype=torch.int64, device=dev)
        cnt = torch.empty(cap, dtype=torch.int64, device=dev)
        s = torch.empty((cap, dim), dtype=torch.float64, device=dev)
        q = torch.empty((cap, dim), dtype=torch.float64, device=dev)
        check(engine.ctx, engine.lib.mfa_tree_acc_batch(engine.ctx, _ptr(feats), _ptr(d_fo), n_utt, total, dim, _ptr(ali), _ptr(d_phone),
                                                         _ptr(d_cls), _ptr(d_flags), int(phone.shape[0]), _ptr(d_ci), int(ci.shape[0]) - 1,
                                                         cap, _ptr(frame_event), _elem_ptr(scal, 0), _elem_ptr(scal, 1),
                                                         _ptr(key) if cap else None, _ptr(cnt) if cap else None,
                                                         _ptr(s) if cap else None, _ptr(q) if cap else None), "mfa_tree_acc_batch")
        n_events, skipped = (int(v) for v in scal.cpu().numpy())
        if n_events <= cap:
            break
        cap = n_events + n_events // 8
    engine._tree_cap = max(cap, 4096)
    st = TreeStats(key[:n_events].cpu().numpy().view(np.uint64), cnt[:n_events].cpu().numpy(), s[:n_events].cpu().numpy(),
                   q[:n_events].cpu().numpy())
    return st, frame_event, skipped


def tree_statistics_host(feats: np.ndarray, frame_off: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                         ci_phones: Sequence[int] = (), context_width: int = 3, central_position: int = 1):
    """The same call on the host twin (mfa_debug_tree_acc_host: no device, every event one loop in ascending frame index): the
    specification the device is held to.  numpy arrays in; ``frame_event`` comes back as a numpy array."""
    lib = _lib.lib()
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    frame_off, n_utt, total = _tree_check("tree_statistics_host", feats.shape, frame_off, int(ali.shape[0]), context_width, central_position)
    dim = int(feats.shape[1])
    phone, cls, flags, ci = tree_tid_tables(tm, ci_phones)
    frame_event = np.empty(total, dtype=np.int32)
    scal = np.zeros(2, dtype=np.int64)
    cap = 0
    while True:
        key, cnt = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.int64)
        s, q = np.empty((cap, dim)), np.empty((cap, dim))
        p = lambda a: a.ctypes.data if a.size else None
        rc = lib.mfa_debug_tree_acc_host(p(feats), frame_off.ctypes.data, n_utt, dim, p(ali), phone.ctypes.data, cls.ctypes.data,
                                         flags.ctypes.data, int(phone.shape[0]), ci.ctypes.data, int(ci.shape[0]) - 1, cap,
                                         p(frame_event), scal.ctypes.data, scal.ctypes.data + 8, p(key), p(cnt), p(s), p(q))
        if rc != 0:
            why = {-2: "feature dimension above 48", -3: "2^31 frames or more", -4: "2^16 phones or more"}.get(rc, "bad arguments")
            raise _lib.MfaHipError(f"mfa_debug_tree_acc_host: {why}")
        n_events, skipped = int(scal[0]), int(scal[1])
        if n_events <= cap:
            break
        cap = n_events
    return TreeStats(key[:n_events], cnt[:n_events], s[:n_events], q[:n_events]), frame_event, skipped


# ---- diagonal UBM: Gaussian selection and the global statistics over the selected Gaussians (include/mfa_hip.h "Diagonal UBM")
def _ubm_device_model(engine, ubm):
    """A ``ubm.DiagUbm`` as the device tensors (gconsts, means_invvars, inv_vars), uploaded once per model object and device."""
    cache = ubm.__dict__.setdefault("_device_arrays", {})
    key = str(engine.device)
    if key not in cache:
        cache.clear()
        cache[key] = tuple(torch.from_numpy(a).to(engine.device) for a in ubm.arrays())
    return cache[key]


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
    engine._launch_ubm_gselect(feats, _ubm_device_model(engine, ubm), int(num_gselect), gselect, loglike)
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
    occ = torch.from_numpy(np.ascontiguousarray(st.occ)).to(dev)
    mean = torch.from_numpy(np.ascontiguousarray(st.mean_acc)).to(dev)
    var = torch.from_numpy(np.ascontiguousarray(st.var_acc)).to(dev)
    tot = torch.tensor([st.tot_like, st.tot_count], dtype=torch.float64, device=dev)
    post = torch.empty((T, n), dtype=torch.float32, device=dev) if want_post else None
    engine._launch_ubm_acc(feats, _ubm_device_model(engine, ubm), n, gselect, frame_weight, occ, mean, var, tot, post)
    st.occ, st.mean_acc, st.var_acc = occ.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    t = tot.cpu().numpy()
    st.tot_like, st.tot_count = float(t[0]), float(t[1])
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
    rc = _lib.lib().mfa_debug_ubm_gselect_host(feats.ctypes.data, int(feats.shape[0]), int(mi.shape[1]), int(gc.shape[0]), gc.ctypes.data,
                                               mi.ctypes.data, iv.ctypes.data, int(num_gselect), gselect.ctypes.data, loglike.ctypes.data)
    if rc != 0:
        raise _lib.MfaHipError(f"mfa_debug_ubm_gselect_host: {_UBM_TWIN_CODES.get(rc, 'bad arguments')}")
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
    occ, mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (st.occ, st.mean_acc, st.var_acc))
    tot = np.array([st.tot_like, st.tot_count], dtype=np.float64)
    post = np.zeros((T, n), dtype=np.float32) if want_post else None
    p = lambda a: None if a is None else a.ctypes.data
    rc = _lib.lib().mfa_debug_ubm_acc_host(p(feats), T, int(mi.shape[1]), int(gc.shape[0]), p(gc), p(mi), p(iv), n, p(gselect), p(fw),
                                           p(occ), p(mean), p(var), p(tot), p(post))
    if rc != 0:
        raise _lib.MfaHipError(f"mfa_debug_ubm_acc_host: {_UBM_TWIN_CODES.get(rc, 'bad arguments')}")
    st.occ, st.mean_acc, st.var_acc = occ, mean, var
    st.tot_like, st.tot_count = float(tot[0]), float(tot[1])
    return (st, post) if want_post else st


# ---- i-vector extractor: pruning, utterance statistics, E-step (include/mfa_hip.h "I-vector extractor") ------------------------
_IVEC_TWIN_CODES = {-2: "feature dimension outside [1, 48]", -3: "Gaussians outside [1, 2048]", -4: "entries per frame outside [1, 64]",
                    -5: "2^31 frames or utterances or more", -6: "i-vector dimension outside [1, 192]"}


def _ivec_twin(rc: int, name: str) -> None:
    if rc != 0:
        raise _lib.MfaHipError(f"{name}: {_IVEC_TWIN_CODES.get(rc, 'bad arguments')}")


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
    _ivec_twin(_lib.lib().mfa_debug_ivector_prune_post_host(post.ctypes.data, int(post.shape[0]), int(post.shape[1]), float(min_post),
                                                           float(scale), out.ctypes.data), "mfa_debug_ivector_prune_post_host")
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
    _ivec_twin(_lib.lib().mfa_debug_ivector_utt_stats_host(feats.ctypes.data, off.ctypes.data, U, D, G, int(gselect.shape[1]),
                                                          gselect.ctypes.data, post.ctypes.data, float(max_count), gamma.ctypes.data,
                                                          X.ctypes.data, None if S is None else S.ctypes.data),
               "mfa_debug_ivector_utt_stats_host")
    return gamma, X, S


def _ivec_device_model(engine, model):
    """An ``ivector.IvectorExtractorModel`` as the device tensors (W, U), computed and uploaded once per model object and device."""
    cache = model.__dict__.setdefault("_device_arrays", {})
    key = str(engine.device)
    if key not in cache:
        cache.clear()
        cache[key] = tuple(torch.from_numpy(a).to(engine.device) for a in model.derived())
    return cache[key]


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
    W, Um = _ivec_device_model(engine, model)
    mean = torch.empty((U, R), dtype=torch.float64, device=dev)
    var = torch.empty((U, P), dtype=torch.float64, device=dev) if want_var else None
    aux = torch.empty((U, 2), dtype=torch.float64, device=dev)
    acc = None
    if into is not None:
        if into.Y.shape != (G, D, R):
            raise ValueError("ivector_estep: `into` does not fit the model")
        acc = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
                    for a in (into.gamma, into.Y, into.Rq, into.isum, into.iscat, np.array([into.n])))
    engine._launch_ivector_estep(gamma, X, W, Um, model.prior_offset, mean, var, aux, acc)
    if into is not None:
        into.gamma, into.Y, into.Rq, into.isum, into.iscat = (t.cpu().numpy() for t in acc[:5])
        into.n = float(acc[5].cpu().numpy()[0])
        _ivec_add_aux(into, aux.cpu().numpy(), gamma.cpu().numpy())
    return mean, var, aux


def _ivec_add_aux(into, aux: np.ndarray, gamma: np.ndarray) -> None:
    """The objective's two sums over the utterances that took part (some γ not zero, a finite solve), utterances ascending."""
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
    acc = [None] * 6
    if into is not None:
        if into.Y.shape != (G, D, R):
            raise ValueError("ivector_estep_host: `into` does not fit the model")
        acc = [np.ascontiguousarray(a, dtype=np.float64) for a in (into.gamma, into.Y, into.Rq, into.isum, into.iscat, np.array([into.n]))]
    p = lambda a: None if a is None else a.ctypes.data
    _ivec_twin(_lib.lib().mfa_debug_ivector_estep_host(p(gamma), p(X), U, D, G, R, p(W), p(Um), float(model.prior_offset), p(mean), p(var),
                                                      p(aux), *(p(a) for a in acc)), "mfa_debug_ivector_estep_host")
    if into is not None:
        into.gamma, into.Y, into.Rq, into.isum, into.iscat = acc[:5]
        into.n = float(acc[5][0])
        _ivec_add_aux(into, aux, gamma)
    return mean, var, aux


# ---- PLDA: the transform, the score matrix and its row-wise consumers (include/mfa_hip.h "PLDA") ---------------------------------
_PLDA_TWIN_CODES = {-2: "dimension outside [1, 1024]", -3: "list length outside [1, 64]", -4: "a psi entry that is not positive and finite",
                    -5: "2^31 vectors or more", -6: "a number of examples below 1", -7: "every output is off"}
PLDA_BLOCK_BYTES = 256 << 20        # device bytes of one row block of ``plda_scores``
PLDA_MATRIX_BYTES = 4 << 30         # the largest full matrix ``plda_scores`` hands out


def _plda_twin(rc: int, name: str) -> None:
    if rc != 0:
        raise _lib.MfaHipError(f"{name}: {_PLDA_TWIN_CODES.get(rc, 'bad arguments')}")


def _plda_device_model(engine, model):
    """A ``plda.PldaModel`` as the device tensors (transform, offset, psi), uploaded once per model object and device."""
    cache = model.__dict__.setdefault("_device_arrays", {})
    key = str(engine.device)
    if key not in cache:
        cache.clear()
        cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(engine.device)
                           for a in (model.transform, model.offset, model.psi))
    return cache[key]


def _plda_vectors(engine, x, D: int, what: str) -> torch.Tensor:
    """Rows of float64 [n, D] on the device, from a numpy array or a tensor."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64))
    if t.dim() != 2 or (t.shape[0] and t.shape[1] != D):
        raise _lib.MfaHipError(f"{what}: vectors {tuple(t.shape)} for a model of dimension {D}")
    return t.to(device=engine.device, dtype=torch.float64).contiguous()


def _plda_counts(engine, n, rows: int, what: str):
    if n is None:
        return None
    t = n if isinstance(n, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32))
    if tuple(t.shape) != (rows,):
        raise _lib.MfaHipError(f"{what}: one number of examples per vector ({tuple(t.shape)} for {rows})")
    return t.to(device=engine.device, dtype=torch.int32).contiguous()


def _plda_norm(normalize_length: bool, simple_length_norm: bool) -> int:
    return 0 if not normalize_length else (1 if simple_length_norm else 2)


def plda_transform(engine, model, x, num_examples=None, normalize_length: bool = True, simple_length_norm: bool = False) -> torch.Tensor:
    """``model.transform_ivector`` of every row of ``x`` ([n, D], numpy or a tensor) on the device (mfa_plda_transform_batch):
    float64 [n, D] on the device, where the scoring calls take it.  ``num_examples``: int32 [n], default 1."""
    x = _plda_vectors(engine, x, model.dim, "plda_transform")
    out = torch.empty_like(x)
    engine._launch_plda_transform(x, _plda_device_model(engine, model), _plda_counts(engine, num_examples, x.shape[0], "plda_transform"),
                                  _plda_norm(normalize_length, simple_length_norm), out)
    return out


def plda_transform_host(model, x, num_examples=None, normalize_length: bool = True, simple_length_norm: bool = False) -> np.ndarray:
    """``plda_transform`` on the host twin (plain loops): numpy in and out."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    if x.shape[0] and x.shape[1] != model.dim:
        raise _lib.MfaHipError(f"plda_transform_host: vectors {x.shape} for a model of dimension {model.dim}")
    n = None if num_examples is None else np.ascontiguousarray(num_examples, dtype=np.int32)
    if n is not None and n.shape != (x.shape[0],):
        raise _lib.MfaHipError("plda_transform_host: one number of examples per vector")
    out = np.empty_like(x)
    T, off, psi = (np.ascontiguousarray(a, dtype=np.float64) for a in (model.transform, model.offset, model.psi))
    _plda_twin(_lib.lib().mfa_debug_plda_transform_host(x.ctypes.data, int(x.shape[0]), model.dim, T.ctypes.data, off.ctypes.data,
                                                        psi.ctypes.data, None if n is None else n.ctypes.data,
                                                        _plda_norm(normalize_length, simple_length_norm), out.ctypes.data),
               "mfa_debug_plda_transform_host")
    return out


def _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, k, want_scores, want_best, want_knn, operands=None):
    """One scoring call: (scores or None, (best index, best score) or None, (k-NN indices, scores) or None), on the device."""
    D = model.dim if operands is None else int(np.shape(operands[0])[1])
    test = _plda_vectors(engine, test, D, "PLDA scoring")
    dev, nt = engine.device, int(test.shape[0])
    if operands is None:
        train = _plda_vectors(engine, train, D, "PLDA scoring")
        ns = int(train.shape[0])
        train_n = _plda_counts(engine, train_n, ns, "PLDA scoring")
        psi = _plda_device_model(engine, model)[2]
    else:
        operands = tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev) if not isinstance(a, torch.Tensor) else a
                         for a in operands)
        ns, psi = int(operands[2].shape[0]), None
    scores = torch.empty((nt, ns), dtype=torch.float64, device=dev) if want_scores else None
    best = (torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.float64, device=dev)) if want_best else None
    knn = (torch.empty((nt, k), dtype=torch.int32, device=dev), torch.empty((nt, k), dtype=torch.float64, device=dev)) if want_knn else None
    engine._launch_plda_score(test, train, train_n, psi, exclude_diagonal, k, scores, best, knn, operands)
    return scores, best, knn


def plda_scores(engine, model, test, train, train_n=None, block_bytes: int = PLDA_BLOCK_BYTES,
                max_bytes: int = PLDA_MATRIX_BYTES) -> np.ndarray:
    """The matrix [test, train] of log-likelihood ratios (mfa_plda_score_batch), vectors in the model's space (``plda_transform``),
    ``train_n`` the examples behind each train vector.  The device writes row blocks of at most ``block_bytes``; the matrix
    is handed out as a numpy array.  One larger than ``max_bytes`` is refused: the consumers that need no stored matrix are
    ``plda_classify`` and ``plda_knn``."""
    test = _plda_vectors(engine, test, model.dim, "plda_scores")
    train = _plda_vectors(engine, train, model.dim, "plda_scores")
    nt, ns = int(test.shape[0]), int(train.shape[0])
    if nt * ns * 8 > max_bytes:
        raise _lib.MfaHipError(f"plda_scores: a matrix of {nt} x {ns} scores ({nt * ns * 8} bytes) exceeds {max_bytes} bytes: "
                               "use plda_knn or plda_classify, which keep no matrix")
    train_n = _plda_counts(engine, train_n, ns, "plda_scores")
    out = np.empty((nt, ns))
    rows = max(1, int(block_bytes) // max(ns * 8, 1))
    for r0 in range(0, nt, rows):
        out[r0: r0 + rows] = _plda_score_call(engine, model, test[r0: r0 + rows], train, train_n, False, 1, True, False, False)[0].cpu().numpy()
    return out


def plda_classify(engine, model, test, train, train_n=None, exclude_diagonal: bool = False):
    """Every test vector's best train vector: (index int32 [n_test], score float64 [n_test]) on the device; −1 and −inf for a
    row without a finite score.  Ties go to the lower index.  No matrix is stored."""
    return _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, 1, False, True, False)[1]


def plda_knn(engine, model, test, train, k: int, train_n=None, exclude_diagonal: bool = False):
    """Every test vector's ``k`` (1 to 64) best train vectors, best first: (indices int32 [n_test, k], scores float64 [n_test, k])
    on the device, padded with −1 and −inf.  ``exclude_diagonal``: test and train are the same vectors, skip j == i."""
    return _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, int(k), False, False, True)[2]


def plda_sweep(engine, test, A, B, c, exclude_diagonal: bool = False, k: int = 1, want_scores=True, want_best=True, want_knn=True):
    """The sweep alone over the caller's operands (mfa_debug_plda_sweep_batch; tests)."""
    return _plda_score_call(engine, None, test, None, None, exclude_diagonal, int(k), want_scores, want_best, want_knn, operands=(A, B, c))


def plda_prepare_host(model, train, train_n=None):
    """(A [n, D], B [n, D], c [n]) of the train vectors on the host twin (mfa_debug_plda_prepare_host)."""
    train = np.ascontiguousarray(np.atleast_2d(train), dtype=np.float64)
    n = None if train_n is None else np.ascontiguousarray(train_n, dtype=np.int32)
    psi = np.ascontiguousarray(model.psi, dtype=np.float64)
    A, B, c = np.empty_like(train), np.empty_like(train), np.empty(train.shape[0])
    _plda_twin(_lib.lib().mfa_debug_plda_prepare_host(train.ctypes.data, int(train.shape[0]), int(train.shape[1]),
                                                      None if n is None else n.ctypes.data, psi.ctypes.data, A.ctypes.data, B.ctypes.data,
                                                      c.ctypes.data), "mfa_debug_plda_prepare_host")
    return A, B, c


def _plda_host_call(model, test, train, train_n, exclude_diagonal, k, want_scores, want_best, want_knn, operands=None):
    test = np.ascontiguousarray(np.atleast_2d(test), dtype=np.float64)
    nt, D = int(test.shape[0]), int(test.shape[1])
    p = lambda a: None if a is None else a.ctypes.data
    if operands is None:
        train = np.ascontiguousarray(np.atleast_2d(train), dtype=np.float64)
        if model.dim != D or (train.shape[0] and train.shape[1] != D):
            raise _lib.MfaHipError(f"PLDA scoring: vectors {test.shape} and {train.shape} for a model of dimension {model.dim}")
        ns = int(train.shape[0])
        n = None if train_n is None else np.ascontiguousarray(train_n, dtype=np.int32)
        if n is not None and n.shape != (ns,):
            raise _lib.MfaHipError("PLDA scoring: one number of examples per train vector")
        psi = np.ascontiguousarray(model.psi, dtype=np.float64)
    else:
        A, B, c = (np.ascontiguousarray(a, dtype=np.float64) for a in operands)
        ns = int(c.shape[0])
    scores = np.empty((nt, ns)) if want_scores else None
    bi, bs = (np.empty(nt, np.int32), np.empty(nt)) if want_best else (None, None)
    ki, ks = (np.empty((nt, k), np.int32), np.empty((nt, k))) if want_knn else (None, None)
    outs = (p(scores), p(bi), p(bs), p(ki), p(ks))
    if operands is None:
        _plda_twin(_lib.lib().mfa_debug_plda_score_host(p(test), nt, p(train), ns, D, p(n), p(psi), int(bool(exclude_diagonal)), int(k), *outs),
                   "mfa_debug_plda_score_host")
    else:
        _plda_twin(_lib.lib().mfa_debug_plda_sweep_host(p(test), nt, D, p(A), p(B), p(c), ns, int(bool(exclude_diagonal)), int(k), *outs),
                   "mfa_debug_plda_sweep_host")
    return scores, (bi, bs) if want_best else None, (ki, ks) if want_knn else None


def plda_scores_host(model, test, train, train_n=None) -> np.ndarray:
    """``plda_scores`` on the host twin (the expanded form in plain loops): numpy in and out."""
    return _plda_host_call(model, test, train, train_n, False, 1, True, False, False)[0]


def plda_classify_host(model, test, train, train_n=None, exclude_diagonal: bool = False):
    return _plda_host_call(model, test, train, train_n, exclude_diagonal, 1, False, True, False)[1]


def plda_knn_host(model, test, train, k: int, train_n=None, exclude_diagonal: bool = False):
    return _plda_host_call(model, test, train, train_n, exclude_diagonal, int(k), False, False, True)[2]


def plda_sweep_host(test, A, B, c, exclude_diagonal: bool = False, k: int = 1, want_scores=True, want_best=True, want_knn=True):
    """``plda_sweep`` on the host twin (mfa_debug_plda_sweep_host)."""
    return _plda_host_call(None, test, None, None, exclude_diagonal, int(k), want_scores, want_best, want_knn, operands=(A, B, c))


# ---- the sweep for any metric and its fourth consumer, the neighbour bit matrix; DBSCAN on it (include/mfa_hip.h "Neighbour bits",
# "Clustering") ------------------------------------------------------------------------------------------------------------------
METRIC_CODES = {"plda": 0, "euclidean": 1, "dot": 2, "cosine": 2}      # cosine: the dot metric on rows made unit length here
NEIGHBOR_BITS_BYTES = 4 << 30                                # the largest bit matrix ``neighbor_bits`` hands out
_PLDA_TWIN_CODES.update({-8: "an unknown metric", -9: "a threshold that is not a number"})
_CLUSTER_TWIN_CODES = {-2: "a number of points outside [0, 2^31)", -3: "min_samples below 1"}


def metric_code(metric) -> int:
    name = getattr(metric, "name", metric)
    if name not in METRIC_CODES:
        raise _lib.MfaHipError(f"metric {metric!r}: one of {sorted(METRIC_CODES)}")
    return METRIC_CODES[name]


def score_threshold(metric, eps: float) -> float:
    """The sweep's threshold for "distance <= eps": plda −eps (the distance is −LLR), euclidean −eps² (eps < 0: no pair passes),
    cosine 1 − eps."""
    code, eps = metric_code(metric), float(eps)
    if code == 0:
        return -eps
    if code == 1:
        return float("inf") if eps < 0 else -(eps * eps)
    return 1.0 - eps


def score_to_distance(metric, scores):
    """Distances from the sweep's scores (numpy): −score, sqrt(−score) floored at 0, 1 − score."""
    code, s = metric_code(metric), np.asarray(scores, dtype=np.float64)
    if code == 0:
        return -s
    return np.sqrt(np.maximum(-s, 0.0)) if code == 1 else 1.0 - s


def _unit_rows(x):
    """Rows made unit length in float64 (torch or numpy); a zero row becomes NaN and is nobody's neighbour."""
    if isinstance(x, torch.Tensor):
        return x / torch.sqrt((x * x).sum(dim=1, keepdim=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def _metric_dim(code: int, model, x) -> int:
    if code == 0:
        if model is None:
            raise _lib.MfaHipError("the plda metric needs the model")
        return model.dim
    return int(np.shape(x)[-1])


def metric_sweep(engine, metric, test, train, threshold=None, model=None, train_n=None, exclude_diagonal: bool = False, k: int = 1,
                 want_scores=False, want_best=False, want_knn=False, want_bits=True, operands=None):
    """One sweep on the device for ``metric`` ("plda", "euclidean", "cosine", or "dot": cosine's sweep on the rows as they are;
    mfa_neighbor_bits_batch): (scores, best, knn, bits), each
    None unless asked for.  ``threshold`` is on the score, as the library takes it (``score_threshold``); ``bits`` is int64
    [n_test, ceil(n_train / 64)] on the device, the words' bits as they are.  ``operands``: the debug entry's (A, B, c)."""
    if operands is None:
        code = metric_code(metric)
        D = _metric_dim(code, model, test)
        test, train = _plda_vectors(engine, test, D, "neighbour sweep"), _plda_vectors(engine, train, D, "neighbour sweep")
        if getattr(metric, "name", metric) == "cosine":
            test, train = _unit_rows(test), _unit_rows(train)
        ns = int(train.shape[0])
        train_n = _plda_counts(engine, train_n, ns, "neighbour sweep") if code == 0 else None
        psi = _plda_device_model(engine, model)[2] if code == 0 else None
    else:
        code, psi, train, train_n = 0, None, None, None
        operands = tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(engine.device) if not isinstance(a, torch.Tensor) else a
                         for a in operands)
        test = _plda_vectors(engine, test, int(operands[0].shape[1]), "neighbour sweep")
        ns = int(operands[2].shape[0])
    dev, nt = engine.device, int(test.shape[0])
    if want_bits and threshold is None:
        raise _lib.MfaHipError("neighbour sweep: the bits need a threshold")
    scores = torch.empty((nt, ns), dtype=torch.float64, device=dev) if want_scores else None
    best = (torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.float64, device=dev)) if want_best else None
    knn = (torch.empty((nt, k), dtype=torch.int32, device=dev), torch.empty((nt, k), dtype=torch.float64, device=dev)) if want_knn else None
    bits = torch.empty((nt, (ns + 63) // 64), dtype=torch.int64, device=dev) if want_bits else None
    if ns == 0 and not (want_scores or want_best or want_knn):
        return None, None, None, bits                  # no train vectors: rows of no words, nothing to ask the library for
    engine._launch_neighbor_bits(test, train, code, train_n, psi, exclude_diagonal, int(k), 0.0 if threshold is None else float(threshold),
                                 scores, best, knn, bits, operands)
    return scores, best, knn, bits


def metric_sweep_host(metric, test, train, threshold=None, model=None, train_n=None, exclude_diagonal: bool = False, k: int = 1,
                      want_scores=False, want_best=False, want_knn=False, want_bits=True, operands=None):
    """``metric_sweep`` on the host twins (mfa_debug_neighbor_bits_host / mfa_debug_neighbor_sweep_host): numpy in and out, ``bits``
    uint64."""
    test = np.ascontiguousarray(np.atleast_2d(test), dtype=np.float64)
    nt, D = int(test.shape[0]), int(test.shape[1])
    p = lambda a: None if a is None else a.ctypes.data
    if operands is None:
        code = metric_code(metric)
        train = np.ascontiguousarray(np.atleast_2d(train), dtype=np.float64)
        if _metric_dim(code, model, test) != D or (train.shape[0] and train.shape[1] != D):
            raise _lib.MfaHipError(f"neighbour sweep: vectors {test.shape} and {train.shape} do not go together")
        if getattr(metric, "name", metric) == "cosine":
            test, train = np.ascontiguousarray(_unit_rows(test)), np.ascontiguousarray(_unit_rows(train))
        ns = int(train.shape[0])
        n = None if train_n is None or code != 0 else np.ascontiguousarray(train_n, dtype=np.int32)
        if n is not None and n.shape != (ns,):
            raise _lib.MfaHipError("neighbour sweep: one number of examples per train vector")
        psi = np.ascontiguousarray(model.psi, dtype=np.float64) if code == 0 else None
    else:
        A, B, c = (np.ascontiguousarray(a, dtype=np.float64) for a in operands)
        ns = int(c.shape[0])
    if want_bits and threshold is None:
        raise _lib.MfaHipError("neighbour sweep: the bits need a threshold")
    thr = 0.0 if threshold is None else float(threshold)
    scores = np.empty((nt, ns)) if want_scores else None
    bi, bs = (np.empty(nt, np.int32), np.empty(nt)) if want_best else (None, None)
    ki, ks = (np.empty((nt, k), np.int32), np.empty((nt, k))) if want_knn else (None, None)
    bits = np.zeros((nt, (ns + 63) // 64), dtype=np.uint64) if want_bits else None
    outs = (p(scores), p(bi), p(bs), p(ki), p(ks), p(bits))
    if ns == 0 and not (want_scores or want_best or want_knn):
        return None, None, None, bits
    if operands is None:
        _plda_twin(_lib.lib().mfa_debug_neighbor_bits_host(p(test), nt, p(train), ns, D, code, p(n), p(psi), int(bool(exclude_diagonal)),
                                                           int(k), thr, *outs), "mfa_debug_neighbor_bits_host")
    else:
        _plda_twin(_lib.lib().mfa_debug_neighbor_sweep_host(p(test), nt, D, p(A), p(B), p(c), ns, int(bool(exclude_diagonal)), int(k), thr,
                                                            *outs), "mfa_debug_neighbor_sweep_host")
    return scores, (bi, bs) if want_best else None, (ki, ks) if want_knn else None, bits


def _bits_size_check(nt: int, ns: int, max_bytes: int) -> None:
    size = nt * ((ns + 63) // 64) * 8
    if size > max_bytes:
        raise _lib.MfaHipError(f"neighbor_bits: a bit matrix of {nt} x {ns} pairs ({size} bytes) exceeds {max_bytes} bytes")


def neighbor_bits(engine, metric, test, train, eps: float, model=None, train_n=None, max_bytes: int = NEIGHBOR_BITS_BYTES) -> torch.Tensor:
    """The ε-neighbourhoods as a bit matrix: int64 words [n_test, ceil(n_train / 64)] on the device, bit j & 63 of word j >> 6 of row i
    set iff the distance of test i to train j is at most ``eps`` in ``metric`` (plda: −LLR, vectors in the model's space).  N²/8
    bytes where the score matrix takes 8 N²; one above ``max_bytes`` is refused."""
    _bits_size_check(int(np.shape(test)[0]), int(np.shape(train)[0]), max_bytes)
    return metric_sweep(engine, metric, test, train, score_threshold(metric, eps), model, train_n)[3]


def neighbor_bits_host(metric, test, train, eps: float, model=None, train_n=None, max_bytes: int = NEIGHBOR_BITS_BYTES) -> np.ndarray:
    _bits_size_check(int(np.shape(test)[0]), int(np.shape(train)[0]), max_bytes)
    return metric_sweep_host(metric, test, train, score_threshold(metric, eps), model, train_n)[3]


def knn(engine, metric, test, train, k: int, model=None, train_n=None, exclude_diagonal: bool = False):
    """``plda_knn`` for any metric: (indices int32 [n_test, k], scores float64 [n_test, k]) on the device, the nearest first; the
    scores are the sweep's (``score_to_distance`` makes distances of them)."""
    return metric_sweep(engine, metric, test, train, None, model, train_n, exclude_diagonal, int(k), want_knn=True, want_bits=False)[2]


def knn_host(metric, test, train, k: int, model=None, train_n=None, exclude_diagonal: bool = False):
    return metric_sweep_host(metric, test, train, None, model, train_n, exclude_diagonal, int(k), want_knn=True, want_bits=False)[2]


def _square_bits(bits, n) -> int:
    n = int(bits.shape[0]) if n is None else int(n)
    if bits.ndim != 2 or tuple(bits.shape) != (n, (n + 63) // 64):
        raise _lib.MfaHipError(f"dbscan_from_bits: words {tuple(bits.shape)} for {n} points (a square matrix of [n, ceil(n / 64)] words)")
    return n


def dbscan_from_bits(engine, bits, min_samples: int, n=None):
    """DBSCAN on a square neighbour matrix (mfa_dbscan_from_bits): dict(labels, core, count: int32 [n] on the device, n_clusters, rounds,
    bits: the symmetrised matrix).  A tensor on the engine's device is symmetrised in place; anything else is copied first."""
    if isinstance(bits, torch.Tensor) and bits.dtype == torch.int64 and bits.device == engine.device and bits.is_contiguous():
        d = bits
    else:
        a = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
        d = torch.from_numpy(np.ascontiguousarray(a).astype(np.uint64, copy=False).view(np.int64).copy()).to(engine.device)
    n = _square_bits(d, n)
    labels, core, count = (torch.empty(n, dtype=torch.int32, device=engine.device) for _ in range(3))
    n_clusters, rounds = engine._launch_dbscan(d, n, int(min_samples), labels, core, count)
    return dict(labels=labels, core=core, count=count, n_clusters=n_clusters, rounds=rounds, bits=d)


def dbscan_from_bits_host(bits, min_samples: int, n=None):
    """``dbscan_from_bits`` on the host twin: numpy arrays, the input left alone."""
    import ctypes as C
    a = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    h = np.ascontiguousarray(a).view(np.uint64).copy() if a.dtype == np.int64 else np.ascontiguousarray(a, dtype=np.uint64).copy()
    n = _square_bits(h, n)
    labels, core, count = (np.empty(n, np.int32) for _ in range(3))
    n_clusters = C.c_int32(0)
    rc = _lib.lib().mfa_debug_dbscan_from_bits_host(h.ctypes.data, n, int(min_samples), labels.ctypes.data, core.ctypes.data, count.ctypes.data,
                                                   C.byref(n_clusters))
    if rc != 0:
        raise _lib.MfaHipError(f"mfa_debug_dbscan_from_bits_host: {_CLUSTER_TWIN_CODES.get(rc, 'bad arguments')}")
    return dict(labels=labels, core=core, count=count, n_clusters=int(n_clusters.value), bits=h)


# ---- HDBSCAN: the pair form, the core scores and the mutual-reachability spanning tree (include/mfa_hip.h "HDBSCAN") -------------------
_HDBSCAN_TWIN_CODES = {-2: "dimension outside [1, 1024]", -3: "neighbours outside [0, 64]", -4: "a psi entry that is not positive and finite",
                       -5: "2^31 points or more", -8: "an unknown metric"}


def pair_metric(metric):
    """(the library's metric code, rows made unit length first, the metric of ``score_to_distance``) of the pair form: cosine is
    euclidean on unit rows, which is what the reference's hdbscan branch clusters."""
    name = getattr(metric, "name", metric)
    code = metric_code(name)
    return (1, True, "euclidean") if name == "cosine" else (code, False, name)


def _hdbscan_twin(rc: int, name: str) -> None:
    if rc != 0:
        raise _lib.MfaHipError(f"{name}: {_HDBSCAN_TWIN_CODES.get(rc, 'bad arguments')}")


def _pair_k(k) -> int:
    k = int(k)
    if not 0 <= k <= 64:
        raise _lib.MfaHipError(f"core_scores: {k} neighbours (0 to 64: a row's list is one wavefront register); min_samples up to 65")
    return k


def core_scores(engine, metric, x, k: int, model=None, want_v: bool = False):
    """The pair form of ``x`` [n, D] and every point's core score (mfa_hdbscan_core_batch): dict(y [n, D], q [n], core [n], v [n, n] or
    None, code) on the device.  ``k = min_samples − 1`` (0 to 64): the core score is the k-th best score over the other points, −inf
    for a point with fewer than k finite ones, +inf at k = 0.  Scores are larger-is-nearer; ``score_to_distance`` of
    ``pair_metric(metric)[2]`` makes distances of them."""
    code, unit, _ = pair_metric(metric)
    k = _pair_k(k)
    x = _plda_vectors(engine, x, _metric_dim(code, model, x), "core_scores")
    if unit:
        x = _unit_rows(x)
    n, dev = int(x.shape[0]), engine.device
    psi = _plda_device_model(engine, model)[2] if code == 0 else None
    y, q, core = torch.empty_like(x), torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    v = torch.empty((n, n), dtype=torch.float64, device=dev) if want_v else None
    engine._launch_hdbscan_core(x, code, psi, k, y, q, core, v)
    return dict(y=y, q=q, core=core, v=v, code=code)


def pair_prepare(engine, metric, x, model=None):
    """(y [n, D], q [n]) of the pair form on the device: v(i, j) = (q_i + q_j) + w · y_i · y_j, bit-symmetric in (i, j)."""
    r = core_scores(engine, metric, x, 0, model)
    return r["y"], r["q"]


def core_scores_host(metric, x, k: int, model=None, want_v: bool = False, v=None):
    """``core_scores`` on the host twin: numpy arrays.  ``v``: a score matrix to take the core scores from (tests: the device's own)."""
    code, unit, _ = pair_metric(metric)
    k = _pair_k(k)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    if _metric_dim(code, model, x) != x.shape[1]:
        raise _lib.MfaHipError(f"core_scores_host: vectors {x.shape} for a model of dimension {model.dim}")
    if unit:
        x = np.ascontiguousarray(_unit_rows(x))
    n = int(x.shape[0])
    psi = np.ascontiguousarray(model.psi, dtype=np.float64) if code == 0 else None
    v_in = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    if v_in is not None and v_in.shape != (n, n):
        raise _lib.MfaHipError(f"core_scores_host: a score matrix {v_in.shape} for {n} points")
    y, q, core = np.empty_like(x), np.empty(n), np.empty(n)
    out_v = np.empty((n, n)) if want_v else None
    p = lambda a: None if a is None else a.ctypes.data
    _hdbscan_twin(_lib.lib().mfa_debug_hdbscan_core_host(p(x), n, int(x.shape[1]), code, p(psi), k, p(y), p(q), p(core), p(out_v), p(v_in)),
                  "mfa_debug_hdbscan_core_host")
    return dict(y=y, q=q, core=core, v=out_v, code=code)


def pair_prepare_host(metric, x, model=None):
    r = core_scores_host(metric, x, 0, model)
    return r["y"], r["q"]


def finish_tree(n: int, lo, hi, score):
    """The spanning forest's edges sorted by the edge order (larger score, then smaller lo, then smaller hi); the components that
    no finite score joins are tied to the first one's smallest member at score −inf (distance +inf): n − 1 edges."""
    lo, hi, score = np.asarray(lo, np.int32), np.asarray(hi, np.int32), np.asarray(score, np.float64)
    if n > 1 and lo.shape[0] < n - 1:
        parent = np.arange(n)

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for a, b in zip(lo.tolist(), hi.tolist()):
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)                      # the smaller root stays: a root is its component's smallest member
        roots = sorted({find(i) for i in range(n)})
        lo = np.concatenate([lo, np.full(len(roots) - 1, roots[0], np.int32)])
        hi = np.concatenate([hi, np.asarray(roots[1:], np.int32)])
        score = np.concatenate([score, np.full(len(roots) - 1, -np.inf)])
    order = np.lexsort((hi, lo, -score))
    return lo[order], hi[order], score[order]


def mreach_mst(engine, metric, y, q, core):
    """The minimum spanning tree of the mutual-reachability graph (mfa_hdbscan_mst_batch) from the pair form and the core scores on
    the device: dict(lo, hi, score: numpy [n − 1], sorted by the edge order; found: the edges the device found, rounds).  No n × n
    array is stored: every Borůvka round is one sweep."""
    code = pair_metric(metric)[0]
    dev = engine.device
    y = y.to(device=dev, dtype=torch.float64).contiguous() if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y, np.float64)).to(dev)
    q, core = (a.to(device=dev, dtype=torch.float64).contiguous() if isinstance(a, torch.Tensor)
               else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev) for a in (q, core))
    n = int(y.shape[0])
    if y.dim() != 2 or tuple(q.shape) != (n,) or tuple(core.shape) != (n,):
        raise _lib.MfaHipError(f"mreach_mst: y {tuple(y.shape)}, q {tuple(q.shape)} and core {tuple(core.shape)} do not go together")
    m = max(n - 1, 1)
    lo, hi = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
    score = torch.empty(m, dtype=torch.float64, device=dev)
    found, rounds = engine._launch_hdbscan_mst(y, q, core, code, lo, hi, score)
    flo, fhi, fs = finish_tree(n, lo[:found].cpu().numpy(), hi[:found].cpu().numpy(), score[:found].cpu().numpy())
    return dict(lo=flo, hi=fhi, score=fs, found=found, rounds=rounds)


def mreach_mst_host(metric, y, q, core, v=None):
    """``mreach_mst`` on the host twin, Kruskal under the same edge order; ``v``: a score matrix to use in place of the pair form's."""
    import ctypes as C
    code = pair_metric(metric)[0]
    y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
    q, core = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(core, dtype=np.float64)
    n = int(y.shape[0])
    v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    if q.shape != (n,) or core.shape != (n,) or (v is not None and v.shape != (n, n)):
        raise _lib.MfaHipError("mreach_mst_host: y, q, core and v do not go together")
    m = max(n - 1, 1)
    lo, hi, score = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m)
    found = C.c_int32(0)
    _hdbscan_twin(_lib.lib().mfa_debug_hdbscan_mst_host(y.ctypes.data, q.ctypes.data, core.ctypes.data, None if v is None else v.ctypes.data, n,
                                                        int(y.shape[1]), code, lo.ctypes.data, hi.ctypes.data, score.ctypes.data,
                                                        C.byref(found)), "mfa_debug_hdbscan_mst_host")
    f = int(found.value)
    flo, fhi, fs = finish_tree(n, lo[:f], hi[:f], score[:f])
    return dict(lo=flo, hi=fhi, score=fs, found=f)
