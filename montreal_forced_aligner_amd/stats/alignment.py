"""Statistics from alignments: per-speaker fMLLR statistics, GMM sufficient statistics, LDA, MLLT and tree statistics (device
call and host twin each), with the host-built tables they share.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import _elem_ptr, _np_ptr, _ptr, check, twin_call
from ..model import DiagGmmModel, TransitionModel
from ..ragged import _speaker_groups
from ._common import accumulators, check_device_frames, frame_pdf_weight, store_accumulators


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
        check(engine.ctx, engine.lib.mfa_fmllr_stats_model(engine.ctx, stats_model.dim, stats_model.num_pdfs, _np_ptr(po), _np_ptr(mi),
                                                           _np_ptr(iv)), "mfa_fmllr_stats_model")
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
    check_device_frames(what, feats, ali)
    feats = feats.contiguous()
    if feats_sum is not None:
        feats_sum = feats_sum.contiguous()
    ali = ali.to(torch.int32).contiguous()
    acc = accumulators(st, dev, tid_count=True)
    d_pdf, d_w = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    tail = (total, _ptr(ali), _ptr(d_pdf), _ptr(d_w), n_tids, *(_ptr(a) for a in acc))
    if feats_sum is None:
        check(engine.ctx, engine.lib.mfa_gmm_acc_batch(engine.ctx, _ptr(feats), *tail), "mfa_gmm_acc_batch")
    else:
        check(engine.ctx, engine.lib.mfa_gmm_acc_twofeats_batch(engine.ctx, _ptr(feats), _ptr(feats_sum), *tail), "mfa_gmm_acc_twofeats_batch")
    store_accumulators(st, acc)
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


_GMM_TWIN_CODES = {-2: "a pdf of more than 128 Gaussians"}


def _gmm_statistics_host(gmm, feats, feats_sum, ali, tm, weights, into, want_post):
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    G, D = gmm.num_gauss, gmm.dim
    st = into if into is not None else GmmStats.zeros(G, D, n_tids)
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    pdf, fw = frame_pdf_weight(ali, id2pdf, w)
    model = model_arrays(gmm)
    acc = accumulators(st, tid_count=True)
    stride = int(np.diff(model[0]).max())
    post = np.zeros((ali.shape[0], stride), dtype=np.float32) if want_post else None
    head = (D, gmm.num_pdfs, *model, feats)
    tail = (int(ali.shape[0]), pdf, fw, ali, n_tids, *acc, post, stride)
    if feats_sum is None:
        twin_call("mfa_debug_gmm_acc_host", _GMM_TWIN_CODES, *head, *tail)
    else:
        twin_call("mfa_debug_gmm_acc_twofeats_host", _GMM_TWIN_CODES, *head, np.ascontiguousarray(feats_sum, dtype=np.float32), *tail)
    store_accumulators(st, acc)
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


def _lda_setup(what, feat_shape, n_ali, frame_off, tm, weights, num_classes, splice_context, into, rand_prune, utt_keys):
    """What the device call and its twin derive from their arguments alike, checked: (tid2class, tid_weight, classes, frame
    offsets, utterances, feature dimension, the statistics to add to, rand_prune, utterance keys or None)."""
    id2class, w, C = _lda_tables(tm, weights, num_classes)
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    n_utt, total = len(frame_off) - 1, int(frame_off[-1])
    if len(feat_shape) != 2 or feat_shape[0] != total or n_ali != total:
        raise _lib.MfaHipError(f"{what}: features {tuple(feat_shape)} and {n_ali} alignment frames for {total} frames")
    dim = int(feat_shape[1])
    S = (2 * int(splice_context) + 1) * dim
    st = into if into is not None else LdaStats.zeros(C, max(S, 0))
    if st.first.shape != (C, S) or st.second.shape != (S, S):
        raise ValueError(f"{what}: `into` does not fit the classes and the spliced dimension")
    rand_prune = float(rand_prune)
    if rand_prune < 0:
        raise ValueError("lda_statistics: rand_prune must be >= 0")
    if rand_prune > 0 and utt_keys is None:
        raise ValueError("lda_statistics: rand_prune needs utt_keys (the utterances' corpus positions)")
    keys = None if utt_keys is None else np.ascontiguousarray(utt_keys, dtype=np.uint32)
    if keys is not None and keys.shape != (n_utt,):
        raise ValueError(f"lda_statistics: {keys.shape} utterance keys for {n_utt} utterances")
    return id2class, w, C, frame_off, n_utt, dim, st, rand_prune, keys


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
    check_device_frames("lda_statistics", mfcc, ali)
    id2class, w, C, frame_off, n_utt, dim, st, rand_prune, keys = _lda_setup(
        "lda_statistics", mfcc.shape, ali.shape[0], frame_off, tm, weights, num_classes, splice_context, into, rand_prune, utt_keys)
    mfcc = mfcc.contiguous()
    ali = ali.to(torch.int32).contiguous()
    d_u2s = None if utt2spk is None else engine._dev(np.ascontiguousarray(utt2spk, dtype=np.int32))
    if cmvn is not None and (cmvn.dtype != torch.float64 or not cmvn.is_cuda):
        raise _lib.MfaHipError("lda_statistics: CMVN statistics must be float64 on the device")
    d_cmvn = None if cmvn is None else cmvn.contiguous()
    zero, first, second = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (st.zero, st.first, st.second))
    cnt = None if tid_count is None else torch.from_numpy(np.ascontiguousarray(tid_count, dtype=np.int64)).to(dev)
    d_cls, d_w = torch.from_numpy(id2class).to(dev), torch.from_numpy(w).to(dev)
    d_keys = None if keys is None else torch.from_numpy(keys.view(np.int32)).to(dev)
    d_fo = engine._dev(frame_off)
    check(engine.ctx, engine.lib.mfa_lda_acc_batch(engine.ctx, _ptr(mfcc), _ptr(d_fo), n_utt, int(frame_off[-1]), dim, _ptr(d_u2s),
                                                    _ptr(d_cmvn), int(splice_context), _ptr(ali), _ptr(d_cls), _ptr(d_w),
                                                    int(id2class.shape[0]), C, rand_prune, _ptr(d_keys), int(seed) & 0xFFFFFFFF,
                                                    _ptr(zero), _ptr(first), _ptr(second), _ptr(cnt)), "mfa_lda_acc_batch")
    st.zero, st.first, st.second = zero.cpu().numpy(), first.cpu().numpy(), second.cpu().numpy()
    if cnt is not None:
        tid_count[...] = cnt.cpu().numpy()
    return st


_LDA_TWIN_CODES = {-2: "spliced dimension above 128", -3: "2^31 frames or more"}


def lda_statistics_host(mfcc: np.ndarray, frame_off: np.ndarray, utt2spk, cmvn, ali: np.ndarray, tm, splice_context: int = 3,
                        weights: Optional[np.ndarray] = None, rand_prune: float = 0.0, utt_keys=None, seed: int = 0,
                        into: Optional[LdaStats] = None, num_classes: Optional[int] = None,
                        tid_count: Optional[np.ndarray] = None) -> LdaStats:
    """The same call on the host twin (mfa_debug_lda_acc_host: no device, frames in ascending index): the specification the
    device is held to.  numpy arrays in."""
    mfcc = np.ascontiguousarray(mfcc, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    id2class, w, C, frame_off, n_utt, dim, st, rand_prune, keys = _lda_setup(
        "lda_statistics_host", mfcc.shape, ali.shape[0], frame_off, tm, weights, num_classes, splice_context, into, rand_prune, utt_keys)
    u2s = None if utt2spk is None else np.ascontiguousarray(utt2spk, dtype=np.int32)
    cm = None if cmvn is None else np.ascontiguousarray(cmvn, dtype=np.float64)
    zero, first, second = (np.ascontiguousarray(a, dtype=np.float64) for a in (st.zero, st.first, st.second))
    cnt = None if tid_count is None else np.ascontiguousarray(tid_count, dtype=np.int64)
    twin_call("mfa_debug_lda_acc_host", _LDA_TWIN_CODES, mfcc, frame_off, n_utt, dim, u2s, cm, int(splice_context), ali, id2class, w,
              int(id2class.shape[0]), C, rand_prune, keys, int(seed) & 0xFFFFFFFF, zero, first, second, cnt)
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
    check_device_frames("mllt_statistics", feats, ali)
    feats = feats.contiguous()
    ali = ali.to(torch.int32).contiguous()
    means = torch.from_numpy(gaussian_means(gmm)).to(dev)
    d_pdf, d_w = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    occ, full, tot = st._device(dev)
    check(engine.ctx, engine.lib.mfa_mllt_acc_batch(engine.ctx, _ptr(feats), total, _ptr(ali), _ptr(d_pdf), _ptr(d_w), n_tids,
                                                     _ptr(means), _ptr(occ), _ptr(full), _ptr(tot)), "mfa_mllt_acc_batch")
    return st


_MLLT_TWIN_CODES = {-2: "a pdf of more than 128 Gaussians", -3: "feature dimension above 48"}


def mllt_statistics_host(gmm: DiagGmmModel, feats: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                         weights: Optional[np.ndarray] = None, into: Optional[MlltStats] = None, want_post: bool = False):
    """The same call on the host twin (mfa_debug_mllt_acc_host: no device, frames in ascending index, plain loops): the
    specification the device is held to.  numpy arrays in; with ``want_post`` also returns every frame's posteriors."""
    id2pdf, w = tid_tables(tm, weights)
    G, D = gmm.num_gauss, gmm.dim
    st = into if into is not None else MlltStats.zeros(G, D)
    if st.shape != (G, D, D):
        raise ValueError("mllt_statistics_host: `into` does not fit the model")
    feats = np.ascontiguousarray(feats, dtype=np.float32)
    ali = np.ascontiguousarray(ali, dtype=np.int32)
    if feats.ndim != 2 or feats.shape[0] != ali.shape[0] or (ali.shape[0] and feats.shape[1] != D):
        raise _lib.MfaHipError(f"mllt_statistics_host: features {feats.shape} for {ali.shape[0]} frames of a model of dim {D}")
    pdf, fw = frame_pdf_weight(ali, id2pdf, w)
    model = model_arrays(gmm)
    st._host()
    stride = int(np.diff(model[0]).max())
    post = np.zeros((ali.shape[0], stride), dtype=np.float32) if want_post else None
    twin_call("mfa_debug_mllt_acc_host", _MLLT_TWIN_CODES, D, gmm.num_pdfs, *model, gaussian_means(gmm), feats, int(ali.shape[0]), pdf, fw,
              st._occ, st._full, st._tot, post, stride)
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


def tree_statistics(engine, feats: torch.Tensor, frame_off: np.ndarray, ali: torch.Tensor, tm: TransitionModel,
                    ci_phones: Sequence[int] = (), context_width: int = 3, central_position: int = 1, cap: Optional[int] = None):
    """Tree statistics of one batch from its alignments (mfa_tree_acc_batch; the contract is in include/mfa_hip.h).

    ``feats`` float32 [ΣT, dim] and ``ali`` int32 [ΣT] transition-ids on the device; ``ci_phones``: the context-independent
    phones (the reference passes silence and OOV phones).  Returns (``TreeStats`` of the batch, ``frame_event`` int32 [ΣT] on
    the device: every frame's row in ``TreeStats.keys`` or −1, the number of utterances skipped).  ``cap``: event rows to
    offer first (default: what the engine's last call needed); the call is repeated when the batch has more."""
    frame_off, n_utt, total = _tree_check("tree_statistics", feats.shape, frame_off, int(ali.shape[0]), context_width, central_position)
    check_device_frames("tree_statistics", feats, ali)
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


_TREE_TWIN_CODES = {-2: "feature dimension above 48", -3: "2^31 frames or more", -4: "2^16 phones or more"}


def tree_statistics_host(feats: np.ndarray, frame_off: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                         ci_phones: Sequence[int] = (), context_width: int = 3, central_position: int = 1):
    """The same call on the host twin (mfa_debug_tree_acc_host: no device, every event one loop in ascending frame index): the
    specification the device is held to.  numpy arrays in; ``frame_event`` comes back as a numpy array."""
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
        x, a, fe, *rows = (v if v.size else None for v in (feats, ali, frame_event, key, cnt, s, q))    # no pointer where there are no rows
        twin_call("mfa_debug_tree_acc_host", _TREE_TWIN_CODES, x, frame_off, n_utt, dim, a, phone, cls, flags, int(phone.shape[0]), ci,
                  int(ci.shape[0]) - 1, cap, fe, scal[:1], scal[1:], *rows)
        n_events, skipped = int(scal[0]), int(scal[1])
        if n_events <= cap:
            break
        cap = n_events
    return TreeStats(key[:n_events], cnt[:n_events], s[:n_events], q[:n_events]), frame_event, skipped
