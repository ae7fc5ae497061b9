"""Batched device pipeline: PCM → MFCC → CMVN → Δ/LDA/fMLLR → GMM scores → Viterbi alignment.

Host orchestration over the C ABI (include/mfa_hip.h).  torch is used only for device memory and streams
("plumbing, not the product"): every kernel runs inside libmfa_hip.so.  The stages mirror the reference's job
functions — MfccFunction / calc_cmvn / FinalFeatureFunction / AlignFunction
(MFA/corpus/features.py:193-376, MFA/corpus/acoustic_corpus.py:1315-1367, MFA/alignment/multiprocessing.py:791-863) —
but operate on ragged batches resident in HBM instead of ark/scp files between processes.

Here: the engine proper (context, configuration, ``_launch_*`` entry points, stage methods, capacity ladder).  ``packing``
and ``frontend`` hold base classes of ``AlignmentEngine``; ``pipeline`` and ``stats`` hold what is re-exported from here.
"""
from __future__ import annotations

import ctypes as C
from functools import partialmethod
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, hostcpu
from ._lib import AlignOpts, GraphBatch, MfccOpts, ScorePlan, _ptr, check   # noqa: F401
from .frontend import DEFAULT_PITCH, _PITCH_ALIAS, FrontEndStages   # noqa: F401
from .kaldi_io import Fst
from .model import DiagGmmModel, TransitionModel
from .packing import GraphPacking, PackedGraphs
from .pipeline import Pipeline   # noqa: F401
from .ragged import _rows_by_group, _speaker_groups, max_len, offsets   # noqa: F401
from .staging import StagingPool, StagingRing
from .stats import (GmmStats, LdaStats, MlltStats, TreeStats, check_delta_fmllr, fmllr_statistics, gmm_statistics, gmm_statistics_host,   # noqa: F401
                    gmm_statistics_twofeats, gmm_statistics_twofeats_host, lda_statistics, lda_statistics_host, mllt_statistics, mllt_statistics_host, model_arrays, tid_tables, tree_statistics, tree_statistics_host)

STATUS_OK, STATUS_RETRIED, STATUS_FAILED, STATUS_TOKEN_OVERFLOW, STATUS_BP_OVERFLOW, STATUS_UNSUPPORTED = 0, 1, 2, 3, 4, 5

DEFAULT_MFCC = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemphasis=0.97,
                    low_frequency=20.0, high_frequency=7800.0, cepstral_lifter=22.0, energy_floor=0.0,
                    num_mel_bins=23, num_coefficients=13, snip_edges=0, remove_dc_offset=1, use_energy=0, raw_energy=1)

# The kernel-timing slots by name, in the order of the MFA_K_* enum of csrc/ctx.hpp: the two lists go together.
KERNEL_SLOTS = ("mfcc", "cmvn", "feats", "gmm", "viterbi", "resample", "pitch", "compress",
                "acc_lookup", "acc_sort", "acc_sums", "acc_reduce", "equal_align",
                "lda_lookup", "lda_second", "lda_class", "lda_reduce",
                "mllt_lookup", "mllt_sort", "mllt_sums", "mllt_reduce",
                "tree_keys", "tree_order", "tree_sums", "vad",
                "ubm_select", "ubm_post", "ubm_sums", "ubm_reduce",
                "ivec_prune", "ivec_utt", "ivec_scatter", "ivec_products", "ivec_solve", "ivec_acc",
                "plda_transform", "plda_prepare", "plda_sweep", "plda_merge",
                "cluster_symmetrise", "cluster_degree", "cluster_rounds", "cluster_labels",
                "silhouette_offsets", "silhouette_sweep")


def _out_ptrs(out: Dict[str, Optional[torch.Tensor]]):
    """The decoders' six output arguments, in the order all three entry points take them, from an ``_align_outputs`` dict."""
    return [_ptr(out[k]) for k in ("ali", "words", "n_words", "like", "frame_like", "status")]


class AlignmentEngine(GraphPacking, FrontEndStages):
    """One engine per (process, GPU).  All tensors handed in must live on ``device``."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise _lib.MfaHipError("no GPU visible: the alignment engine has no CPU fallback")
        self.lib = _lib.lib()
        self.device = torch.device("cuda", device)
        self.ctx = self.lib.mfa_create(device)
        if not self.ctx:
            raise _lib.MfaHipError(f"mfa_create({device}) failed")
        self.ctx = C.c_void_p(self.ctx)
        self.use_torch_stream()
        self.mfcc_opts: Optional[MfccOpts] = None
        self.num_ceps = 13
        self.gmm: Optional[DiagGmmModel] = None
        self.slot_class: Optional[np.ndarray] = None
        # pinned staging buffers for packing calls that bring no pool of their own (pack_graphs(..., pool=None)): three sets
        # in turn, each reused once the copies last started from it are done.  (CorpusAligner's batch pipeline keeps a
        # rotation of its own: no call here can hand out a pool that still backs one of its batches.)
        self._staging = StagingRing(self.device, 3)
        self._pcm_staging = StagingRing(self.device, 2)   # PCM has its own pair: gathered while graphs compile
        self._nf_checked: Optional[tuple] = None         # (window, shift, snip_edges) num_frames_array was checked for
        self._slab, self._slab_off = None, 0             # _dev: pinned memory once asked for (False once refused), bump offset

    def next_staging(self) -> StagingPool:
        """The staging pool to fill next (round robin; waits until the copies last started from it are done)."""
        return self._staging.next()

    def close(self) -> None:
        if self.ctx:
            self.lib.mfa_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self) -> None:
        self.stream = torch.cuda.current_stream(self.device)
        check(self.ctx, self.lib.mfa_set_stream(self.ctx, C.c_void_p(self.stream.cuda_stream), 0), "mfa_set_stream")

    # ------------------------------------------------------------------ configuration
    def configure_mfcc(self, **kw) -> None:
        opts = _lib.options(MfccOpts, DEFAULT_MFCC, kw, "MFCC")
        check(self.ctx, self.lib.mfa_mfcc_configure(self.ctx, C.byref(opts)), "mfa_mfcc_configure")
        self.mfcc_opts = opts            # (a refused option set leaves the library, and so this object, at the previous one)
        self.num_ceps = int(opts.num_coefficients)

    def mfcc_path(self) -> str:
        """Which tail of the MFCC kernel the configured options take now: ``"specialised"`` (compile-time trip counts) or
        ``"generic"`` (a filterbank plan beyond its bounds, or ``MFA_MFCC_GENERIC=1``, read at every call)."""
        return {1: "specialised", 2: "generic"}[int(self.lib.mfa_mfcc_path(self.ctx))]

    def load_gmm(self, gmm: DiagGmmModel) -> None:
        po, gc, mi, iv = model_arrays(gmm)
        check(self.ctx, self.lib.mfa_load_gmm(self.ctx, gmm.dim, gmm.num_pdfs, po.ctypes.data, gc.ctypes.data,
                                              mi.ctypes.data, iv.ctypes.data), "mfa_load_gmm")
        self.gmm = gmm
        slots = np.array([self.lib.mfa_gmm_slot(self.ctx, p) for p in range(gmm.num_pdfs)], dtype=np.int32)
        n_gauss = np.diff(gmm.pdf_offsets)
        # classes in kernel order: 32 rows single block, 32 rows multi-block (> 32 Gaussians), 16, 8, 4, 1
        cls = np.full(gmm.num_pdfs, 5, dtype=np.int32)
        for i, s in enumerate((32, 16, 8, 4, 1)):
            cls[slots == s] = i + 1
        cls[(slots == 32) & (n_gauss <= 32)] = 0
        self.slot_class = cls

    def num_frames(self, num_samples: int) -> int:
        return int(self.lib.mfa_mfcc_num_frames(self.ctx, num_samples))

    def num_frames_array(self, num_samples: np.ndarray) -> np.ndarray:
        """``num_frames`` for a whole batch (Kaldi NumFrames, both snip_edges settings), with the window and shift computed as
        the library computes them (float32 arithmetic, mfa_mfcc_configure); checked against the library on first use."""
        n = np.asarray(num_samples, dtype=np.int64)
        if self.mfcc_opts is None:
            self.configure_mfcc()
        o = self.mfcc_opts
        f32 = np.float32
        win = int(f32(f32(o.sample_frequency) * f32(0.001)) * f32(o.frame_length_ms))
        shift = int(f32(f32(o.sample_frequency) * f32(0.001)) * f32(o.frame_shift_ms))
        snip = int(o.snip_edges)
        out = np.where(n < win, 0, 1 + (n - win) // shift) if snip else (n + shift // 2) // shift
        key = (win, shift, snip)
        if self._nf_checked != key:
            for probe in (0, 1, win - 1, win, win + shift - 1, win + shift, 159999, 160000, 160001, 1 << 20):
                ref = (0 if probe < win else 1 + (probe - win) // shift) if snip else (probe + shift // 2) // shift
                if self.num_frames(probe) != ref:
                    raise _lib.MfaHipError("num_frames_array disagrees with mfa_mfcc_num_frames")
            self._nf_checked = key
        return out.astype(np.int64)

    def frame_offsets(self, sample_off: np.ndarray) -> np.ndarray:
        return offsets(self.num_frames_array(np.diff(sample_off)))

    # ------------------------------------------------------------------ host → device
    _SLAB_BYTES = 512 << 20

    def _dev(self, a: np.ndarray) -> torch.Tensor:
        """Host array → device, without making the host wait for the device: the array is copied into a slab of pinned
        memory (bump allocation, wrap-around after a device synchronisation — once every several batches) and sent
        asynchronously.  A pageable ``.to(device)`` would block until everything queued on the stream before it has finished,
        i.e. until the previous batch has been decoded; ``Tensor.pin_memory()`` per array costs a pinned allocation (3 ms on
        this runtime)."""
        a = np.ascontiguousarray(a)
        nbytes = a.nbytes
        if nbytes == 0 or nbytes > self._SLAB_BYTES // 4:
            return torch.from_numpy(a).to(self.device)
        slab = self._slab
        if slab is None:
            try:
                slab = self._slab = torch.empty(self._SLAB_BYTES, dtype=torch.uint8, pin_memory=True)
            except RuntimeError:
                self._slab = False
                return torch.from_numpy(a).to(self.device)
        elif slab is False:
            return torch.from_numpy(a).to(self.device)
        off = (self._slab_off + 255) & ~255
        if off + nbytes > self._SLAB_BYTES:
            torch.cuda.synchronize(self.device)      # every copy out of the slab has run, whichever stream it was queued on
            off = 0
        self._slab_off = off + nbytes
        view = slab.numpy()[off: off + nbytes].view(a.dtype).reshape(a.shape)
        view[...] = a
        with torch.cuda.device(self.device):
            return torch.from_numpy(view).to(self.device, non_blocking=True)

    def gather_pcm(self, arrays: Sequence[np.ndarray], pool: Optional[StagingPool] = None):
        """int16 arrays (one per utterance, host) → one device tensor + sample offsets: threaded gather into pinned staging
        memory (mfa_gather_pcm), one asynchronous H2D copy."""
        arrays = [a if isinstance(a, np.ndarray) else np.asarray(a, dtype=np.int16) for a in arrays]   # (lists, tensors)
        n = len(arrays)
        so = offsets(np.fromiter((a.shape[0] for a in arrays), dtype=np.int64, count=n))
        if pool is None:
            pool = self._pcm_staging.next()
        stage = pool.get("pcm", int(so[-1]), np.int16)
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []
        for k, a in enumerate(arrays):
            if a.dtype != np.int16 or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=np.int16)
                keep.append(a)
            ptrs[k] = a.__array_interface__["data"][0]
        if self.lib.mfa_gather_pcm(n, ptrs, so.ctypes.data, stage.ctypes.data, hostcpu.threads(0.5, 8)) != 0:
            raise _lib.MfaHipError("mfa_gather_pcm: bad arguments")
        return pool.to_device(stage, self.stream), so

    def gather_rows(self, feats: torch.Tensor, rows: np.ndarray) -> torch.Tensor:
        """Rows ``rows`` of a device matrix as a new contiguous device matrix (device-to-device copies of the contiguous
        runs; no arithmetic)."""
        rows = np.asarray(rows, dtype=np.int64)
        out = torch.empty((rows.shape[0], feats.shape[1]), dtype=feats.dtype, device=feats.device)
        if rows.shape[0] == 0:
            return out
        cuts = np.nonzero(np.diff(rows) != 1)[0] + 1
        starts = np.concatenate([[0], cuts]); ends = np.concatenate([cuts, [rows.shape[0]]])
        for a, b in zip(starts, ends):
            out[a:b].copy_(feats[int(rows[a]): int(rows[a]) + int(b - a)])
        return out

    # ------------------------------------------------------------------ the hot path's entry points, each called from here alone
    # Device tensors and offsets already on the device in, nothing allocated or uploaded: the stage methods below and
    # ``Pipeline`` (persistent tensors) both launch through these.  ``out`` of the decoders: the dict of ``_align_outputs``.
    def _launch_mfcc(self, pcm, d_sample_off, d_frame_off, n_utt: int, max_frames: int, out) -> None:
        check(self.ctx, self.lib.mfa_mfcc_batch(self.ctx, _ptr(pcm), _ptr(d_sample_off), _ptr(d_frame_off), n_utt, max_frames,
                                                _ptr(out)), "mfa_mfcc_batch")

    def _launch_cmvn_stats(self, feats, d_frame_off, n_utt: int, dim: int, d_spk_off, d_spk_utt, n_spk: int, stats) -> None:
        check(self.ctx, self.lib.mfa_cmvn_stats(self.ctx, _ptr(feats), _ptr(d_frame_off), n_utt, dim, _ptr(d_spk_off),
                                                _ptr(d_spk_utt), n_spk, _ptr(stats)), "mfa_cmvn_stats")

    def _launch_feats(self, mfcc, d_frame_off, n_utt: int, max_frames: int, dim: int, d_utt2spk, cmvn, lda, splice_context: int,
                      fmllr, out) -> None:
        """Δ+ΔΔ without ``lda``, splice + LDA with it."""
        transform = (0, 0, None, 0, 0) if lda is None else (1, splice_context, _ptr(lda), int(lda.shape[0]), int(lda.shape[1]))
        check(self.ctx, self.lib.mfa_feats_batch(self.ctx, _ptr(mfcc), _ptr(d_frame_off), n_utt, max_frames, dim, _ptr(d_utt2spk),
                                                 _ptr(cmvn), *transform, _ptr(fmllr), _ptr(out)), "mfa_feats_batch")

    def _launch_compress(self, feats, d_frame_off, n_utt: int, c0: int, c1: int, cmvn, d_utt2spk, out, glob, colhdr, data) -> None:
        check(self.ctx, self.lib.mfa_compress_batch(self.ctx, _ptr(feats), _ptr(d_frame_off), n_utt, int(feats.shape[1]), c0, c1,
                                                    _ptr(cmvn), _ptr(d_utt2spk), int(cmvn.shape[2]) - 1 if cmvn is not None else 0,
                                                    _ptr(out), _ptr(glob), _ptr(colhdr), _ptr(data)), "mfa_compress_batch")

    def _launch_vad(self, feats, d_frame_off, n_utt: int, total: int, max_frames: int, opts, vad, thr, voiced) -> None:
        check(self.ctx, self.lib.mfa_vad_batch(self.ctx, _ptr(feats), int(feats.shape[1]), _ptr(d_frame_off), n_utt, total, max_frames,
                                               C.byref(opts), _ptr(vad), _ptr(thr), _ptr(voiced)), "mfa_vad_batch")

    def _launch_sliding_cmvn(self, feats, d_frame_off, n_utt: int, max_frames: int, dim: int, opts, out) -> None:
        check(self.ctx, self.lib.mfa_sliding_cmvn_batch(self.ctx, _ptr(feats), _ptr(d_frame_off), n_utt, max_frames, dim,
                                                        int(feats.shape[1]), C.byref(opts), _ptr(out)), "mfa_sliding_cmvn_batch")

    def _launch_select_count(self, vad, d_frame_off, n_utt: int, total: int, n: int, src, out_off) -> None:
        check(self.ctx, self.lib.mfa_select_frames_count(self.ctx, _ptr(vad), _ptr(d_frame_off), n_utt, total, n, _ptr(src),
                                                         _ptr(out_off)), "mfa_select_frames_count")

    def _launch_select(self, feats, src, n_out: int, out) -> None:
        check(self.ctx, self.lib.mfa_select_frames_batch(self.ctx, _ptr(feats), int(feats.shape[1]), int(feats.shape[1]), _ptr(src),
                                                         n_out, _ptr(out), int(out.shape[1])), "mfa_select_frames_batch")

    def _launch_vad_runs(self, vad, d_frame_off, n_utt: int, total: int, capacity: int, begin, end, run_off) -> None:
        check(self.ctx, self.lib.mfa_vad_runs_batch(self.ctx, _ptr(vad), _ptr(d_frame_off), n_utt, total, capacity, _ptr(begin),
                                                    _ptr(end), _ptr(run_off)), "mfa_vad_runs_batch")

    def _launch_ubm_gselect(self, feats, model, num_gselect: int, gselect, loglike) -> None:
        """``model``: the device tensors (gconsts, means_invvars, inv_vars) of one mixture."""
        gc, mi, iv = model
        check(self.ctx, self.lib.mfa_ubm_gselect_batch(self.ctx, _ptr(feats), int(feats.shape[0]), int(mi.shape[1]), int(gc.shape[0]),
                                                       _ptr(gc), _ptr(mi), _ptr(iv), num_gselect, _ptr(gselect), _ptr(loglike)),
              "mfa_ubm_gselect_batch")

    def _launch_ubm_acc(self, feats, model, n: int, gselect, frame_weight, occ, mean, var, tot, post) -> None:
        gc, mi, iv = model
        check(self.ctx, self.lib.mfa_ubm_acc_batch(self.ctx, _ptr(feats), int(feats.shape[0]), int(mi.shape[1]), int(gc.shape[0]),
                                                   _ptr(gc), _ptr(mi), _ptr(iv), n, _ptr(gselect), _ptr(frame_weight), _ptr(occ),
                                                   _ptr(mean), _ptr(var), _ptr(tot), _ptr(post)), "mfa_ubm_acc_batch")

    def _launch_ivector_prune(self, post, min_post: float, scale: float, out) -> None:
        check(self.ctx, self.lib.mfa_ivector_prune_post_batch(self.ctx, _ptr(post), int(post.shape[0]), int(post.shape[1]), float(min_post),
                                                              float(scale), _ptr(out)), "mfa_ivector_prune_post_batch")

    def _launch_ivector_utt_stats(self, feats, d_frame_off, n_utt: int, G: int, gselect, post, max_count: float, gamma, X, S) -> None:
        check(self.ctx, self.lib.mfa_ivector_utt_stats_batch(self.ctx, _ptr(feats), _ptr(d_frame_off), n_utt, int(feats.shape[0]),
                                                             int(feats.shape[1]), G, int(gselect.shape[1]), _ptr(gselect), _ptr(post),
                                                             float(max_count), _ptr(gamma), _ptr(X), _ptr(S)),
              "mfa_ivector_utt_stats_batch")

    def _launch_ivector_estep(self, gamma, X, W, U, prior_offset: float, mean, var, aux, acc) -> None:
        """``acc``: None (extraction) or the six accumulators (Γ, Y, Rq, isum, iscat, n)."""
        a = acc if acc is not None else (None,) * 6
        check(self.ctx, self.lib.mfa_ivector_estep_batch(self.ctx, _ptr(gamma), _ptr(X), int(gamma.shape[0]), int(W.shape[1]),
                                                         int(W.shape[0]), int(W.shape[2]), _ptr(W), _ptr(U), float(prior_offset),
                                                         _ptr(mean), _ptr(var), _ptr(aux), *(_ptr(t) for t in a)),
              "mfa_ivector_estep_batch")

    def _launch_plda_transform(self, x, model, num_examples, norm: int, out) -> None:
        """``model``: the device tensors (transform, offset, psi) of a ``plda.PldaModel``; ``norm`` 0 none, 1 simple, 2 the model's."""
        T, off, psi = model
        check(self.ctx, self.lib.mfa_plda_transform_batch(self.ctx, _ptr(x), int(x.shape[0]), int(T.shape[0]), _ptr(T), _ptr(off), _ptr(psi),
                                                          _ptr(num_examples), int(norm), _ptr(out)), "mfa_plda_transform_batch")

    def _launch_plda_score(self, test, train, train_n, psi, exclude_diagonal: bool, k: int, scores, best, knn, operands=None) -> None:
        """``best`` / ``knn``: None or the (index, score) pair of tensors.  ``operands``: the debug entry's (A, B, c) in place of
        ``train``, ``train_n`` and ``psi`` (mfa_debug_plda_sweep_batch)."""
        b, q = best or (None, None), knn or (None, None)
        outs = (_ptr(scores), _ptr(b[0]), _ptr(b[1]), _ptr(q[0]), _ptr(q[1]))
        nt, D = int(test.shape[0]), int(test.shape[1])
        if operands is not None:
            A, B, c = operands
            check(self.ctx, self.lib.mfa_debug_plda_sweep_batch(self.ctx, _ptr(test), nt, D, _ptr(A), _ptr(B), _ptr(c), int(c.shape[0]),
                                                                int(bool(exclude_diagonal)), int(k), *outs), "mfa_debug_plda_sweep_batch")
        else:
            check(self.ctx, self.lib.mfa_plda_score_batch(self.ctx, _ptr(test), nt, _ptr(train), int(train.shape[0]), D, _ptr(train_n),
                                                          _ptr(psi), int(bool(exclude_diagonal)), int(k), *outs), "mfa_plda_score_batch")

    def _launch_neighbor_bits(self, test, train, metric: int, train_n, psi, exclude_diagonal: bool, k: int, threshold: float, scores, best,
                              knn, bits, operands=None) -> None:
        """The sweep for a metric (0 plda, 1 euclidean, 2 dot) with the neighbour words among its outputs (mfa_neighbor_bits_batch);
        ``operands`` as in ``_launch_plda_score`` (mfa_debug_neighbor_sweep_batch)."""
        b, q = best or (None, None), knn or (None, None)
        outs = (_ptr(scores), _ptr(b[0]), _ptr(b[1]), _ptr(q[0]), _ptr(q[1]), _ptr(bits))
        nt, D = int(test.shape[0]), int(test.shape[1])
        if operands is not None:
            A, B, c = operands
            check(self.ctx, self.lib.mfa_debug_neighbor_sweep_batch(self.ctx, _ptr(test), nt, D, _ptr(A), _ptr(B), _ptr(c), int(c.shape[0]),
                                                                    int(bool(exclude_diagonal)), int(k), float(threshold), *outs),
                  "mfa_debug_neighbor_sweep_batch")
        else:
            check(self.ctx, self.lib.mfa_neighbor_bits_batch(self.ctx, _ptr(test), nt, _ptr(train), int(train.shape[0]), D, int(metric),
                                                             _ptr(train_n), _ptr(psi), int(bool(exclude_diagonal)), int(k), float(threshold),
                                                             *outs), "mfa_neighbor_bits_batch")

    def _launch_dbscan(self, bits, n: int, min_samples: int, labels, core, count):
        """DBSCAN on the neighbour words ``bits`` [n, ceil(n / 64)], symmetrised in place (mfa_dbscan_from_bits): (clusters, rounds)."""
        n_clusters, rounds = C.c_int32(0), C.c_int32(0)
        check(self.ctx, self.lib.mfa_dbscan_from_bits(self.ctx, _ptr(bits), int(n), int(min_samples), _ptr(labels), _ptr(core), _ptr(count),
                                                      C.byref(n_clusters), C.byref(rounds)), "mfa_dbscan_from_bits")
        return int(n_clusters.value), int(rounds.value)

    def _launch_hdbscan_core(self, x, metric: int, psi, k: int, y, q, core, v) -> None:
        """The pair form's prepare step and the core scores (mfa_hdbscan_core_batch); ``v``: None or the [n, n] score matrix."""
        check(self.ctx, self.lib.mfa_hdbscan_core_batch(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(metric), _ptr(psi), int(k),
                                                        _ptr(y), _ptr(q), _ptr(core), _ptr(v)), "mfa_hdbscan_core_batch")

    def _launch_hdbscan_mst(self, y, q, core, metric: int, lo, hi, score):
        """Borůvka on the mutual-reachability graph (mfa_hdbscan_mst_batch): (edges, rounds)."""
        n_edges, rounds = C.c_int32(0), C.c_int32(0)
        check(self.ctx, self.lib.mfa_hdbscan_mst_batch(self.ctx, _ptr(y), _ptr(q), _ptr(core), int(y.shape[0]), int(y.shape[1]), int(metric),
                                                       _ptr(lo), _ptr(hi), _ptr(score), C.byref(n_edges), C.byref(rounds)),
              "mfa_hdbscan_mst_batch")
        return int(n_edges.value), int(rounds.value)

    def _launch_silhouette(self, x, metric: int, psi, off, sil, a, b, bj, v) -> None:
        """Every row's silhouette coefficient under the cluster column ranges ``off`` (int32 [C + 1]; mfa_silhouette_batch)."""
        check(self.ctx, self.lib.mfa_silhouette_batch(self.ctx, _ptr(x), int(x.shape[0]), int(x.shape[1]), int(metric), _ptr(psi), _ptr(off),
                                                      int(off.shape[0]) - 1, _ptr(sil), _ptr(a), _ptr(b), _ptr(bj), _ptr(v)),
              "mfa_silhouette_batch")

    def _launch_scan(self, values, d_frame_off, n_utt: int, total: int, scan, totals) -> None:
        check(self.ctx, self.lib.mfa_vad_scan_batch(self.ctx, _ptr(values), _ptr(d_frame_off), n_utt, total, _ptr(scan),
                                                    _ptr(totals)), "mfa_vad_scan_batch")

    def _launch_score(self, feats, d_frame_off, n_utt: int, max_frames: int, pdf_list, d_pdf_off, class_counts, pdf_first_frame,
                      d_ll_off, out) -> None:
        check(self.ctx, self.lib.mfa_gmm_score_batch(self.ctx, _ptr(feats), _ptr(d_frame_off), n_utt, max_frames, _ptr(pdf_list),
                                                     _ptr(d_pdf_off), _ptr(class_counts), _ptr(pdf_first_frame), _ptr(d_ll_off),
                                                     _ptr(out)), "mfa_gmm_score_batch")

    def _launch_align(self, graphs: PackedGraphs, gstruct: GraphBatch, loglikes, d_ll_off, d_ll_cols, d_frame_off, total: int,
                      opts: AlignOpts, out: Dict[str, Optional[torch.Tensor]]) -> None:
        check(self.ctx, self.lib.mfa_align_batch(
            self.ctx, C.byref(gstruct), _ptr(loglikes), _ptr(d_ll_off), _ptr(d_ll_cols), _ptr(d_frame_off), total,
            graphs.total_arcs, graphs.max_states, graphs.max_arcs, C.byref(opts), *_out_ptrs(out)), "mfa_align_batch")

    def _launch_align_features(self, graphs: PackedGraphs, gstruct: GraphBatch, plan: ScorePlan, feats, d_frame_off,
                               max_frames: int, total: int, opts: AlignOpts, window: int, loglikes, d_ll_off, d_ll_cols,
                               out: Dict[str, Optional[torch.Tensor]]) -> None:
        check(self.ctx, self.lib.mfa_align_features_batch(
            self.ctx, C.byref(gstruct), C.byref(plan), _ptr(feats), _ptr(d_frame_off), max_frames, total, graphs.total_arcs,
            graphs.max_states, graphs.max_arcs, C.byref(opts), window, _ptr(loglikes), _ptr(d_ll_off), _ptr(d_ll_cols),
            *_out_ptrs(out)), "mfa_align_features_batch")

    def _align_outputs(self, n: int, total: int, want_frame_likes: bool) -> Dict[str, Optional[torch.Tensor]]:
        """What a decoder writes: ali, words, frame_like (or None) [total]; n_words, like, status (−1: not decoded) [n]."""
        dev, i32, f32 = self.device, torch.int32, torch.float32
        return dict(ali=torch.zeros(total, dtype=i32, device=dev), words=torch.zeros(total, dtype=i32, device=dev),
                    n_words=torch.zeros(n, dtype=i32, device=dev), like=torch.zeros(n, dtype=f32, device=dev),
                    status=torch.full((n,), -1, dtype=i32, device=dev),
                    frame_like=torch.zeros(total, dtype=f32, device=dev) if want_frame_likes else None)

    # ------------------------------------------------------------------ stages
    def mfcc(self, pcm: torch.Tensor, sample_off: np.ndarray, frame_off: Optional[np.ndarray] = None):
        """pcm: int16 [ΣN] on device.  Returns (mfcc float32 [ΣT, num_ceps], frame_off host int64 [n+1])."""
        if self.mfcc_opts is None:
            self.configure_mfcc()
        assert pcm.dtype == torch.int16 and pcm.is_cuda
        if frame_off is None:
            frame_off = self.frame_offsets(sample_off)
        out = torch.empty((int(frame_off[-1]), self.num_ceps), dtype=torch.float32, device=self.device)
        d_so, d_fo = self._dev(sample_off.astype(np.int64)), self._dev(frame_off)
        self._launch_mfcc(pcm, d_so, d_fo, len(sample_off) - 1, max_len(frame_off), out)
        return out, frame_off

    def cmvn_stats(self, feats: torch.Tensor, frame_off: np.ndarray, utt2spk: np.ndarray, n_spk: int) -> torch.Tensor:
        n_utt = len(frame_off) - 1
        order, spk_off = _rows_by_group(utt2spk, n_spk)
        dim = feats.shape[1]
        stats = torch.empty((n_spk, 2, dim + 1), dtype=torch.float64, device=self.device)
        d_fo, d_so, d_su = self._dev(frame_off), self._dev(spk_off), self._dev(order)
        self._launch_cmvn_stats(feats, d_fo, n_utt, dim, d_so, d_su, n_spk, stats)
        return stats

    def features(self, mfcc: torch.Tensor, frame_off: np.ndarray, utt2spk: Optional[np.ndarray] = None,
                 cmvn: Optional[torch.Tensor] = None, lda: Optional[torch.Tensor] = None,
                 fmllr: Optional[torch.Tensor] = None, splice_context: int = 3) -> torch.Tensor:
        """CMVN → Δ+ΔΔ (no ``lda``) or splice+LDA, then per-speaker fMLLR when ``fmllr`` is given: [n_spk, D, D+1] with
        D = 3·dim after the deltas, the LDA's rows after the LDA.  Mirrors FeatureArchive's chain (MFA/db.py:2101-2136)."""
        n_utt = len(frame_off) - 1
        dim = mfcc.shape[1]
        if lda is None and fmllr is not None:
            check_delta_fmllr(fmllr, dim, utt2spk)
        d_fo = self._dev(frame_off)
        d_u2s = self._dev(np.asarray(utt2spk, dtype=np.int32)) if utt2spk is not None else None
        out = torch.empty((int(frame_off[-1]), 3 * dim if lda is None else lda.shape[0]), dtype=torch.float32, device=self.device)
        self._launch_feats(mfcc, d_fo, n_utt, max_len(frame_off), dim, d_u2s, cmvn, lda, splice_context, fmllr, out)
        return out

    def _check_width(self, feats: torch.Tensor, what: str) -> None:
        """The scoring kernels read ``feats`` by pointer, at the loaded model's width: a matrix of another width is refused
        here, on the host."""
        if self.gmm is not None and (feats.dim() != 2 or int(feats.shape[1]) != int(self.gmm.dim)):
            raise _lib.MfaHipError(f"{what}: the features have {int(feats.shape[1]) if feats.dim() == 2 else tuple(feats.shape)} "
                                   f"columns, the loaded acoustic model has {int(self.gmm.dim)} dimensions")

    def score(self, feats: torch.Tensor, frame_off: np.ndarray, pdf_list: torch.Tensor, pdf_off_host: np.ndarray,
              class_counts: torch.Tensor, pdf_first_frame: Optional[torch.Tensor] = None):
        """Returns (loglikes float32 flat, ll_off host int64 [n+1], ll_cols int32 tensor).  With ``pdf_first_frame``
        (PackedGraphs.pdf_first_frame) cells no decoder token can ask for are left unwritten (zero here)."""
        self._check_width(feats, "score")
        P = np.diff(pdf_off_host)
        ll_off = offsets(np.diff(frame_off) * P)
        alloc = torch.empty if pdf_first_frame is None else torch.zeros
        out = alloc(int(ll_off[-1]), dtype=torch.float32, device=self.device)
        d_fo, d_po, d_lo = self._dev(frame_off), self._dev(pdf_off_host.astype(np.int64)), self._dev(ll_off)
        self._launch_score(feats, d_fo, len(frame_off) - 1, max_len(frame_off), pdf_list, d_po, class_counts, pdf_first_frame,
                           d_lo, out)
        return out, ll_off, self._dev(P.astype(np.int32))

    def _decoder_prologue(self, graphs: PackedGraphs, frame_off: np.ndarray, ll_off: np.ndarray, want_frame_likes: bool, *opts):
        """What the three decoders start from: (AlignOpts(*opts), the output dict, ``ll_off`` and ``frame_off`` on the device)."""
        return (AlignOpts(*opts), self._align_outputs(graphs.n_utt, int(frame_off[-1]), want_frame_likes),
                self._dev(ll_off), self._dev(frame_off))

    def align(self, graphs: PackedGraphs, loglikes: torch.Tensor, ll_off: np.ndarray, ll_cols: torch.Tensor,
              frame_off: np.ndarray, beam: float = 10.0, retry_beam: float = 40.0, acoustic_scale: float = 0.1,
              max_tokens: int = 1024, bp_tokens_per_frame: int = 512, want_frame_likes: bool = False):
        """Returns device tensors: ali [ΣT], words [ΣT] (+ n_words [n]), like [n], status [n], frame_like or None."""
        opts, out, d_lo, d_fo = self._decoder_prologue(graphs, frame_off, ll_off, want_frame_likes, beam, retry_beam,
                                                       acoustic_scale, max_tokens, bp_tokens_per_frame)
        self._launch_align(graphs, graphs.struct(), loglikes, d_lo, ll_cols, d_fo, int(frame_off[-1]), opts, out)
        return out

    def align_general(self, graphs: PackedGraphs, feats: torch.Tensor, frame_off: np.ndarray, beam: float = 10.0,
                      retry_beam: float = 40.0, acoustic_scale: float = 0.1, bp_tokens_per_frame: int = 512,
                      want_frame_likes: bool = False):
        """Alignment over graphs with epsilon input arcs / wide states: dense scores, then FasterDecoder as Kaldi runs it
        (ProcessNonemitting included), one GPU thread per utterance — mfa_align_general_batch."""
        self._check_width(feats, "align_general")
        ll, ll_off, ll_cols = self.score(feats, frame_off, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts)
        opts, out, d_lo, d_fo = self._decoder_prologue(graphs, frame_off, ll_off, want_frame_likes, beam, retry_beam,
                                                       acoustic_scale, 0, bp_tokens_per_frame)
        gs = graphs.struct()
        h_fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        check(self.ctx, self.lib.mfa_align_general_batch(self.ctx, C.byref(gs), _ptr(ll), _ptr(d_lo), _ptr(ll_cols), _ptr(d_fo),
                                                         h_fo.ctypes.data, graphs.max_states, graphs.max_arcs, C.byref(opts),
                                                         *_out_ptrs(out)), "mfa_align_general_batch")
        return out

    def align_features(self, graphs: PackedGraphs, feats: torch.Tensor, frame_off: np.ndarray, beam: float = 10.0,
                       retry_beam: float = 40.0, acoustic_scale: float = 0.1, max_tokens: int = 1024,
                       bp_tokens_per_frame: int = 512, want_frame_likes: bool = False, window: int = 64,
                       loglikes: Optional[torch.Tensor] = None):
        """features + graphs → alignments with acoustic scores evaluated lazily, window by window, for the pdfs live tokens
        can reach (mfa_align_features_batch) — the shape of GmmAligner.align_utterance(fst, feats)
        (MFA/alignment/multiprocessing.py:846-853).  Same results as ``score`` + ``align``.  ``loglikes``: optional scratch
        [Σ T·P] (zero-filled here when omitted, so tests can see which cells were written)."""
        self._check_width(feats, "align_features")
        P = np.diff(graphs.pdf_off_host)
        ll_off = offsets(np.diff(frame_off) * P)
        if loglikes is None:
            loglikes = torch.zeros(int(ll_off[-1]), dtype=torch.float32, device=self.device)
        opts, out, d_lo, d_fo = self._decoder_prologue(graphs, frame_off, ll_off, want_frame_likes, beam, retry_beam,
                                                       acoustic_scale, max_tokens, bp_tokens_per_frame)
        self._launch_align_features(graphs, graphs.struct(), graphs.plan(), feats, d_fo, max_len(frame_off), int(frame_off[-1]),
                                    opts, int(window), loglikes, d_lo, self._dev(P.astype(np.int32)), out)
        return dict(out, loglikes=loglikes, ll_off=ll_off)

    # ------------------------------------------------------------------ timing helpers (bench.py)
    def kernel_timing(self, enable: bool) -> None:
        check(self.ctx, self.lib.mfa_kernel_timing(self.ctx, int(enable)), "mfa_kernel_timing")

    def _kernel_time(self, slot: int) -> Dict[str, float]:
        ms, n = C.c_float(0), C.c_int(0)
        check(self.ctx, self.lib.mfa_kernel_time_ms(self.ctx, slot, C.byref(ms), C.byref(n)), "mfa_kernel_time_ms")
        return dict(ms=float(ms.value), launches=int(n.value))

    def kernel_times(self) -> Dict[str, Dict[str, float]]:
        """The five stages of the benchmark's step (its stage table lists these and no others)."""
        return {name: self._kernel_time(i) for i, name in enumerate(KERNEL_SLOTS[:5])}

    def kernel_time(self, name: str) -> Dict[str, float]:
        """Accumulated time and launches (pitch: launch groups) of one of ``KERNEL_SLOTS`` under ``kernel_timing``."""
        return self._kernel_time(KERNEL_SLOTS.index(name))

    resample_time = partialmethod(kernel_time, "resample")
    pitch_time = partialmethod(kernel_time, "pitch")
    compress_time = partialmethod(kernel_time, "compress")

    def reset_kernel_times(self) -> None:
        check(self.ctx, self.lib.mfa_kernel_time_reset(self.ctx), "mfa_kernel_time_reset")


_PER_FRAME = ("ali", "words", "frame_like")          # decoder outputs over an utterance's frames; the others are one per utterance


def _decode_again(eng, ks: List[int], feats, frame_off: np.ndarray, host: Dict[str, np.ndarray], run) -> None:
    """Utterances ``ks`` of a batch as a batch of their own (their feature rows gathered) through ``run(feats, frame_off)``,
    and what it returns merged over their entries of ``host``."""
    fo_s = offsets([frame_off[k + 1] - frame_off[k] for k in ks])
    r = run(eng.gather_rows(feats, np.concatenate([np.arange(frame_off[k], frame_off[k + 1]) for k in ks])), fo_s)
    r = {key: r[key].cpu().numpy() for key in host}
    for j, k in enumerate(ks):
        a, b, a2, b2 = int(frame_off[k]), int(frame_off[k + 1]), int(fo_s[j]), int(fo_s[j + 1])
        for key, dst in host.items():
            if key in _PER_FRAME:
                dst[a:b] = r[key][a2:b2]
            else:
                dst[k] = r[key][j]


def redo_capacity(eng, fsts: Sequence[Fst], tm: TransitionModel, feats: torch.Tensor, frame_off: np.ndarray,
                  host: Dict[str, np.ndarray], decode, beam: float, retry_beam: float, acoustic_scale: float) -> List[int]:
    """The capacity ladder of a decoded batch.  Token / back-pointer overflows (status 3 / 4) are not alignment failures —
    FasterDecoder has no such limits: those utterances are decoded again on their own with ``PackedGraphs.hard_bounds()``
    (one token per graph state), which cannot overflow; what still reports a capacity status then (the epsilon closure's pop
    budget on a pathological epsilon sub-graph) goes to the general decoder, which runs Kaldi's loops as they are, with
    ``bp_tokens_per_frame = 2 * max_states + 64``.

    ``fsts``: the batch's graphs with transition probabilities applied, by position; ``feats`` / ``frame_off``: its features
    on the device and frame offsets on the host; ``host``: the first decode's results as host arrays, updated in place — its
    keys say what is merged (``frame_like`` only when the caller brings it); ``decode(graphs, feats, frame_off, max_tokens,
    bp_tokens_per_frame)``: the caller's decoder for the hard-bounds step.  Merging: per-utterance values by position,
    per-frame arrays over the utterance's whole frame range — of ``words`` only the first ``n_words`` entries mean
    anything, to the decoder and to every consumer.  Returns the positions decoded again; with none there is no device call
    and nothing is packed."""
    status = host["status"]
    over = np.flatnonzero((status == 3) | (status == 4)).tolist()
    if not over:
        return over
    sub = eng.pack_graphs([fsts[k] for k in over], tm)
    _decode_again(eng, over, feats, frame_off, host, lambda f, fo: decode(sub, f, fo, *sub.hard_bounds()))
    still = [k for k in over if status[k] in (3, 4)]
    if still:
        gg = eng.pack_graphs_general([fsts[k] for k in still], tm)
        _decode_again(eng, still, feats, frame_off, host, lambda f, fo: eng.align_general(
            gg, f, fo, beam=beam, retry_beam=retry_beam, acoustic_scale=acoustic_scale,
            bp_tokens_per_frame=2 * gg.max_states + 64, want_frame_likes="frame_like" in host))
    return over
