"""Batched device pipeline: PCM → MFCC → CMVN → Δ/LDA/fMLLR → GMM scores → Viterbi alignment.

Host orchestration over the C ABI (include/mfa_hip.h).  torch is used only for device memory and streams
("plumbing, not the product"): every kernel runs inside libmfa_hip.so.  The stages mirror the reference's job
functions — MfccFunction / calc_cmvn / FinalFeatureFunction / AlignFunction
(MFA/corpus/features.py:193-376, MFA/corpus/acoustic_corpus.py:1315-1367, MFA/alignment/multiprocessing.py:791-863) —
but operate on ragged batches resident in HBM instead of ark/scp files between processes.
"""
from __future__ import annotations

import os
import ctypes as C
from dataclasses import dataclass
from typing import Tuple, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import AlignOpts, GraphBatch, MfccOpts, PitchOpts, ScorePlan, check
from .kaldi_io import Fst
from .model import DiagGmmModel, TransitionModel

STATUS_OK, STATUS_RETRIED, STATUS_FAILED, STATUS_TOKEN_OVERFLOW, STATUS_BP_OVERFLOW, STATUS_UNSUPPORTED = 0, 1, 2, 3, 4, 5

DEFAULT_MFCC = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemphasis=0.97,
                    low_frequency=20.0, high_frequency=7800.0, cepstral_lifter=22.0, energy_floor=0.0,
                    num_mel_bins=23, num_coefficients=13, snip_edges=0, remove_dc_offset=1, use_energy=0, raw_energy=1)

# Kaldi's PitchExtractionOptions / ProcessPitchOptions at MFA's values (MFA/models.py:551-576 sets max_f0 800 and
# snip_edges True; Kaldi's own max_f0 is 400)
DEFAULT_PITCH = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, min_f0=50.0, max_f0=800.0,
                     soft_min_f0=10.0, penalty_factor=0.1, lowpass_cutoff=1000.0, resample_frequency=4000.0, delta_pitch=0.005,
                     nccf_ballast=7000.0, preemphasis=0.0, pov_scale=2.0, pov_offset=0.0, pitch_scale=2.0,
                     lowpass_filter_width=1, upsample_filter_width=5, snip_edges=1, normalization_context=75,
                     add_pov_feature=1, add_normalized_log_pitch=1, add_raw_log_pitch=0, add_delta_pitch=0)
_PITCH_INT = ("lowpass_filter_width", "upsample_filter_width", "snip_edges", "normalization_context", "add_pov_feature",
              "add_normalized_log_pitch", "add_raw_log_pitch", "add_delta_pitch")
_PITCH_ALIAS = {"frame_length": "frame_length_ms", "frame_shift": "frame_shift_ms"}    # kalpy's names (milliseconds)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _out_ptrs(out: Dict[str, Optional[torch.Tensor]]):
    """The decoders' six output arguments, in the order all three entry points take them, from an ``_align_outputs`` dict."""
    return [_ptr(out[k]) for k in ("ali", "words", "n_words", "like", "frame_like", "status")]


def _split_passes(mono: bool, gauss_per_pdf: int) -> Tuple[bool, bool]:
    """(split-operand scoring at all, its f16x2 pass) for a model, as MFA_GMM_BF16 / MFA_GMM_F16 say right now (tests and the
    benchmark flip them inside one process, so nothing is cached)."""
    split = os.environ.get("MFA_GMM_BF16", "1") != "0" and not mono and gauss_per_pdf != 1
    return split, split and os.environ.get("MFA_GMM_F16", "1") != "0"


def _host_threads(share: float = 1.0, cap: int = 32) -> int:
    from . import hostcpu
    return hostcpu.threads(share, cap)


def offsets(lengths, dtype=np.int64) -> np.ndarray:
    """Lengths of n pieces laid end to end → where each starts, and the total last: [0, l0, l0 + l1, …], ``dtype`` [n + 1]."""
    return np.concatenate([[0], np.cumsum(lengths)]).astype(dtype)


def _rows_by_group(rows: np.ndarray, n_groups: int) -> Tuple[np.ndarray, np.ndarray]:
    """Utterances listed group by group (stable) and each group's range in that list, as the per-speaker kernels take them:
    int32 [n], int32 [n_groups + 1].  A group may be empty."""
    return np.argsort(rows, kind="stable").astype(np.int32), offsets(np.bincount(rows, minlength=n_groups), np.int32)


def _speaker_groups(utt2spk) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Speaker labels of any kind → (sorted distinct labels, each utterance's row among them, ``_rows_by_group`` of the rows)."""
    spk_ids, inv = np.unique(np.asarray(utt2spk), return_inverse=True)
    return (spk_ids, inv) + _rows_by_group(inv, len(spk_ids))


def _flatten_fsts(fsts: Sequence[Fst]):
    """A list of graphs end to end: (S [n], A [n], state_off, arc_base, arc_off int32 [ΣS + n], final float32 [ΣS], arcs)."""
    S = np.array([f.num_states for f in fsts], dtype=np.int64)
    A = np.array([f.num_arcs for f in fsts], dtype=np.int64)
    arc_off = np.concatenate([f.arc_offsets.astype(np.int32) for f in fsts]) if len(fsts) else np.zeros(0, np.int32)
    final = np.concatenate([f.final for f in fsts]).astype(np.float32)
    return S, A, offsets(S), offsets(A), arc_off, final, np.concatenate([f.arcs for f in fsts])


class RaggedView:
    """``np.split(flat, offsets[1:-1])`` without making the pieces up front: piece u is ``flat[offsets[u]: offsets[u + 1]]``."""

    def __init__(self, flat: np.ndarray, offsets: np.ndarray):
        self.flat, self.offsets = flat, offsets

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, u):
        if isinstance(u, slice):
            return [self[k] for k in range(*u.indices(len(self)))]
        if u < 0:
            u += len(self)
        return self.flat[int(self.offsets[u]): int(self.offsets[u + 1])]

    def __iter__(self):
        for u in range(len(self)):
            yield self[u]


class StagingPool:
    """Named host staging buffers in pinned memory, reused from batch to batch (a fresh 200 MB numpy array costs more in page
    faults than the copy it is for).  ``get`` hands out a numpy view; ``to_device`` starts an asynchronous H2D copy of a view
    and remembers it: ``wait`` blocks until every copy started since the last ``wait`` has left the buffers — call it before
    writing into them again."""

    def __init__(self, device: torch.device, pinned: bool = True):
        self.device = device
        self.pinned = pinned
        self._buf: Dict[str, torch.Tensor] = {}
        self._event: Optional[torch.cuda.Event] = None

    def get(self, name: str, count: int, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        need = max(1, int(count)) * dtype.itemsize
        t = self._buf.get(name)
        if t is None or t.numel() < need:
            size = int(need * 1.25) + 64
            t = None
            if self.pinned:
                try:
                    t = torch.empty(size, dtype=torch.uint8, pin_memory=True)
                except RuntimeError:      # pinned allocation refused (constrained container): pageable still works
                    self.pinned = False
            if t is None:
                t = torch.empty(size, dtype=torch.uint8)
            self._buf[name] = t
        return t.numpy()[: int(count) * dtype.itemsize].view(dtype)

    def to_device(self, view: np.ndarray, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        src = torch.from_numpy(view)
        with torch.cuda.device(self.device):
            out = src.to(self.device, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(self.device) if stream is None else stream)
        return out

    def wait(self) -> None:
        if self._event is not None:
            self._event.synchronize()
            self._event = None


@dataclass
class PackedGraphs:
    """Graphs of a batch in the device layout mfa_align_batch consumes (see mfa_graph_batch)."""

    n_utt: int
    max_states: int
    max_arcs: int
    total_arcs: int
    tensors: Dict[str, torch.Tensor]
    pdf_list: torch.Tensor      # int32 [ΣP_u] (slot-sorted per utterance)
    pdf_off: torch.Tensor       # int64 [n_utt+1]
    class_counts: torch.Tensor  # int32 [n_utt,6]
    pdf_off_host: np.ndarray
    pdf_lists_host: Sequence[np.ndarray]                  # per-utterance views of the host copy of pdf_list
    pdf_first_frame: Optional[torch.Tensor] = None        # int32 [ΣP_u]: first frame a pdf can be asked for
    pdf_first_frame_host: Optional[List[np.ndarray]] = None
    # lazy (windowed) scoring keys — mfa_score_plan: running max inside each class of the longest-path depth of a pdf's
    # source states, and {BFS depth, longest-path depth} of every graph state
    pdf_last_depth: Optional[torch.Tensor] = None         # int32 [ΣP_u]
    state_depth: Optional[torch.Tensor] = None            # int32 [ΣS_u, 2]
    # class-0 columns laid out in `groups` runs (pdf id mod groups), one per XCD of the scoring kernel: columns per run
    groups: int = 1
    group_counts: Optional[torch.Tensor] = None           # int32 [n_utt, groups]

    def plan(self) -> ScorePlan:
        if self.pdf_last_depth is None or self.state_depth is None or self.pdf_first_frame is None:
            raise _lib.MfaHipError("these graphs were packed without depth keys (lazy scoring needs them)")
        return ScorePlan(self.pdf_list.data_ptr(), self.pdf_off.data_ptr(), self.class_counts.data_ptr(),
                         self.pdf_first_frame.data_ptr(), self.pdf_last_depth.data_ptr(), self.state_depth.data_ptr(),
                         int(np.diff(self.pdf_off_host).max()) if self.n_utt else 0, int(self.groups),
                         self.group_counts.data_ptr() if self.group_counts is not None else None)

    @property
    def has_eps(self) -> bool:
        """Some graph of the batch has epsilon input arcs (the decoder then runs ProcessNonemitting after every frame)."""
        return self.tensors.get("state_nemit") is not None

    def hard_bounds(self) -> Tuple[int, int]:
        """(max_tokens, bp_tokens_per_frame) that the decoder's capacity statuses cannot occur with: one token per graph state
        — and, for graphs with epsilon arcs, room behind the back-pointer trail for the path the traceback writes there
        (T + E arc indices, E ≤ T·S in the worst case: half a record per frame and state)."""
        s = max(1, int(self.max_states))
        return s, s + (s // 2 + 2 if self.has_eps else 0)

    def struct(self) -> GraphBatch:
        t = self.tensors
        nemit = t.get("state_nemit")
        return GraphBatch(self.n_utt, t["state_off"].data_ptr(), t["arc_base"].data_ptr(), t["start"].data_ptr(),
                          t["arc_off"].data_ptr(), t["final"].data_ptr(), t["arc_next"].data_ptr(),
                          t["arc_weight"].data_ptr(), t["arc_col"].data_ptr(), t["arc_ilabel"].data_ptr(),
                          t["arc_olabel"].data_ptr(), nemit.data_ptr() if nemit is not None else None)


class AlignmentEngine:
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
        self._staging = [StagingPool(self.device), StagingPool(self.device), StagingPool(self.device)]
        self._staging_turn = 0
        self._pcm_staging = [StagingPool(self.device), StagingPool(self.device)]   # PCM has its own pair: gathered while graphs compile
        self._pcm_turn = 0
        self.pitch_opts: Optional[PitchOpts] = None      # configure_pitch
        self.num_pitch_cols = 0
        self._nf_checked: Optional[tuple] = None         # (window, shift, snip_edges) num_frames_array was checked for
        self._slab, self._slab_off = None, 0             # _dev: pinned memory once asked for (False once refused), bump offset

    def next_staging(self) -> StagingPool:
        """The staging pool to fill next (round robin; waits until the copies last started from it are done)."""
        self._staging_turn = (self._staging_turn + 1) % len(self._staging)
        pool = self._staging[self._staging_turn]
        pool.wait()
        return pool

    def gather_pcm(self, arrays: Sequence[np.ndarray], pool: Optional[StagingPool] = None):
        """int16 arrays (one per utterance, host) → one device tensor + sample offsets: threaded gather into pinned staging
        memory (mfa_gather_pcm), one asynchronous H2D copy."""
        arrays = [a if isinstance(a, np.ndarray) else np.asarray(a, dtype=np.int16) for a in arrays]   # (lists, tensors)
        n = len(arrays)
        lens = np.fromiter((a.shape[0] for a in arrays), dtype=np.int64, count=n)
        so = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=so[1:])
        if pool is None:
            self._pcm_turn ^= 1
            pool = self._pcm_staging[self._pcm_turn]
            pool.wait()
        stage = pool.get("pcm", int(so[-1]), np.int16)
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []
        for k, a in enumerate(arrays):
            if a.dtype != np.int16 or not a.flags.c_contiguous:
                a = np.ascontiguousarray(a, dtype=np.int16)
                keep.append(a)
            ptrs[k] = a.__array_interface__["data"][0]
        if self.lib.mfa_gather_pcm(n, ptrs, so.ctypes.data, stage.ctypes.data, _host_threads(0.5, 8)) != 0:
            raise _lib.MfaHipError("mfa_gather_pcm: bad arguments")
        return pool.to_device(stage, self.stream), so

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
        d = dict(DEFAULT_MFCC)
        for k, v in kw.items():
            if k not in d:
                raise KeyError(f"unknown MFCC option {k!r}")
            d[k] = v
        for k in ("num_mel_bins", "num_coefficients", "snip_edges", "remove_dc_offset", "use_energy", "raw_energy"):
            d[k] = int(d[k])
        opts = MfccOpts(**d)
        check(self.ctx, self.lib.mfa_mfcc_configure(self.ctx, C.byref(opts)), "mfa_mfcc_configure")
        self.mfcc_opts = opts            # (a refused option set leaves the library, and so this object, at the previous one)
        self.num_ceps = d["num_coefficients"]

    def load_gmm(self, gmm: DiagGmmModel) -> None:
        po = np.ascontiguousarray(gmm.pdf_offsets, dtype=np.int32)
        gc = np.ascontiguousarray(gmm.gconsts, dtype=np.float32)
        mi = np.ascontiguousarray(gmm.means_invvars, dtype=np.float32)
        iv = np.ascontiguousarray(gmm.inv_vars, dtype=np.float32)
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

    # ------------------------------------------------------------------ stages
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

    # ------------------------------------------------------------------ sample-rate conversion (ahead of the MFCC)
    def model_rate(self) -> int:
        """The rate the MFCC is configured for (``sample_frequency``), in whole Hz: what every utterance is brought to."""
        if self.mfcc_opts is None:
            self.configure_mfcc()
        f = float(self.mfcc_opts.sample_frequency)
        if f != int(f):
            raise _lib.MfaHipError(f"the resampler takes whole rates in Hz (sample_frequency is {f})")
        return int(f)

    def resample_block_outputs(self) -> int:
        """Consecutive output samples per workgroup of the resampling kernel (mfa_resample_block_outputs)."""
        return int(self.lib.mfa_resample_block_outputs())

    def num_resampled(self, n: int, rate: Optional[int]) -> int:
        """Samples at the model's rate that ``n`` samples at ``rate`` become (Kaldi GetNumOutputSamples with flush)."""
        target = self.model_rate()
        if rate is None or int(rate) == target:
            return int(n)
        out = int(self.lib.mfa_resample_num_samples(int(rate), target, int(n)))
        if out < 0:
            raise _lib.MfaHipError(f"mfa_resample_num_samples({int(rate)} Hz -> {target} Hz, {int(n)}): rates must lie in 1000 - 384000 Hz")
        return out

    def num_resampled_array(self, num_samples: np.ndarray, rates: Sequence[Optional[int]]) -> np.ndarray:
        """``num_resampled`` for a batch: the same integer arithmetic per distinct rate, checked against the library on the
        longest utterance of each."""
        n = np.asarray(num_samples, dtype=np.int64)
        target = self.model_rate()
        r = np.fromiter((target if x is None else int(x) for x in rates), dtype=np.int64, count=n.shape[0])
        out = n.copy()
        for rate in np.unique(r[r != target]).tolist():
            sel = r == rate
            g = int(np.gcd(rate, target))
            per_in, per_out = target // g, rate // g                  # ticks of 1 / lcm seconds per input / output sample
            length = n[sel] * per_in
            last = length // per_out
            last -= (last * per_out == length)
            cnt = np.where(length <= 0, 0, last + 1)
            probe = int(np.argmax(n[sel]))
            if int(cnt[probe]) != self.num_resampled(int(n[sel][probe]), rate):
                raise _lib.MfaHipError("num_resampled_array disagrees with mfa_resample_num_samples")
            out[sel] = cnt
        return out

    def resample(self, pcm: torch.Tensor, sample_off: np.ndarray, rates: Sequence[Optional[int]]):
        """pcm: int16 [ΣN] on device, utterance u recorded at ``rates[u]`` Hz (None: the model's rate).  Returns
        (pcm at the model's rate, its sample offsets): utterances already at that rate are copied, the others converted on
        the device, one launch per distinct rate (mfa_resample_batch).  A batch with nothing to convert comes back as it
        is, without a device call."""
        assert pcm.dtype == torch.int16 and pcm.is_cuda
        target = self.model_rate()
        so = np.ascontiguousarray(sample_off, dtype=np.int64)
        n_utt = so.shape[0] - 1
        r = np.fromiter((target if x is None else int(x) for x in rates), dtype=np.int64, count=n_utt)
        if not np.any(r != target):
            return pcm, so
        out_len = self.num_resampled_array(np.diff(so), r)
        oo = np.zeros(n_utt + 1, dtype=np.int64)
        np.cumsum(out_len, out=oo[1:])
        out = torch.empty(int(oo[-1]), dtype=torch.int16, device=self.device)
        # utterances at the model's rate: device-to-device copies of their contiguous runs
        same = r == target
        edges = np.flatnonzero(np.diff(np.concatenate([[False], same, [False]]).astype(np.int8)))
        for a, b in zip(edges[::2].tolist(), edges[1::2].tolist()):
            if so[b] > so[a]:
                out[int(oo[a]): int(oo[b])].copy_(pcm[int(so[a]): int(so[b])])
        d_so, d_oo = self._dev(so), self._dev(oo)
        for rate in np.unique(r[~same]).tolist():
            sel = np.flatnonzero(r == rate).astype(np.int32)
            max_out = int(out_len[sel].max())
            for a in range(0, sel.shape[0], 65535):           # (the kernel indexes the selected utterances in blockIdx.y)
                d_sel = self._dev(sel[a: a + 65535])
                check(self.ctx, self.lib.mfa_resample_batch(self.ctx, int(rate), target, _ptr(pcm), _ptr(d_so), _ptr(out), _ptr(d_oo),
                                                            _ptr(d_sel), int(d_sel.shape[0]), max_out), "mfa_resample_batch")
        return out, oo

    # ------------------------------------------------------------------ pitch and voicing (pasted after CMVN)
    def configure_pitch(self, **kw) -> None:
        """Options of kalpy's PitchComputer (``frame_length`` / ``frame_shift`` in milliseconds are accepted under kalpy's
        names).  A refused set — add_delta_pitch, bad f0 bounds — raises and leaves the previous one in force; the set in force
        is called for again at no cost.  The options are state of the ENGINE: whoever shares it (a CorpusAligner and a kalpy
        PitchComputer on the process's engine) shares them, as they share the MFCC options."""
        d = dict(DEFAULT_PITCH)
        for k, v in kw.items():
            k = _PITCH_ALIAS.get(k, k)
            if k not in d:
                raise KeyError(f"unknown pitch option {k!r}")
            d[k] = v
        for k in _PITCH_INT:
            d[k] = int(d[k])
        opts = PitchOpts(**d)
        if self.pitch_opts is not None and bytes(opts) == bytes(self.pitch_opts):
            return                       # already in force: no tables to rebuild and upload
        check(self.ctx, self.lib.mfa_pitch_configure(self.ctx, C.byref(opts)), "mfa_pitch_configure")
        self.pitch_opts = opts
        self.num_pitch_cols = int(self.lib.mfa_pitch_num_columns(self.ctx))

    def _need_pitch(self) -> None:
        if self.pitch_opts is None:
            raise _lib.MfaHipError("configure_pitch has not been called")

    def pitch_num_frames(self, num_samples: int) -> int:
        self._need_pitch()
        n = int(self.lib.mfa_pitch_num_frames(self.ctx, int(num_samples)))
        if n < 0:
            check(self.ctx, -1, "mfa_pitch_num_frames")
        return n

    def pitch_frame_offsets(self, sample_off: np.ndarray) -> np.ndarray:
        """Frame offsets of a batch's pitch features (the tracker's own frame counts, mfa_pitch_num_frames)."""
        self._need_pitch()
        frames = np.fromiter((self.pitch_num_frames(int(n)) for n in np.diff(sample_off)), dtype=np.int64, count=len(sample_off) - 1)
        return offsets(frames)

    @staticmethod
    def paste_frame_offsets(mfcc_frame_off: np.ndarray, pitch_frame_off: np.ndarray) -> np.ndarray:
        """The paste rule: an utterance gets min(mfcc, pitch) frames when the two counts differ by at most 1 (paste-feats,
        length tolerance 1); a larger difference is refused — on the host, before anything is launched."""
        mf, pf = np.diff(np.asarray(mfcc_frame_off, dtype=np.int64)), np.diff(np.asarray(pitch_frame_off, dtype=np.int64))
        bad = np.flatnonzero(np.abs(mf - pf) > 1)
        if bad.size:
            u = int(bad[0])
            raise _lib.MfaHipError(f"utterance {u}: {int(mf[u])} MFCC frames and {int(pf[u])} pitch frames differ by more than 1 "
                                   "(the two option sets must share frame shift, length and snip_edges)")
        return offsets(np.minimum(mf, pf))

    def pitch_workspace_bytes(self, sample_off: np.ndarray, frame_off: np.ndarray) -> int:
        self._need_pitch()
        ns, nf = np.diff(sample_off), np.diff(frame_off)
        return int(self.lib.mfa_pitch_workspace_bytes(self.ctx, len(ns), int(ns.sum()), int(nf.sum()), int(ns.max()) if len(ns) else 0,
                                                      int(nf.max()) if len(nf) else 0))

    def pitch_raw(self, pcm: torch.Tensor, sample_off: np.ndarray, frame_off: Optional[np.ndarray] = None):
        """pcm: int16 [ΣN] on device at the pitch options' sample_frequency.  Returns (raw float32 [ΣT, 2] = (POV NCCF, pitch in
        Hz) per frame, frame_off): the tracker's output before ProcessPitch (mfa_pitch_batch).  ``frame_off``, when given,
        must hold the tracker's own frame counts."""
        self._need_pitch()
        assert pcm.dtype == torch.int16 and pcm.is_cuda
        so = np.ascontiguousarray(sample_off, dtype=np.int64)
        fo = self.pitch_frame_offsets(so) if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
        n_utt = so.shape[0] - 1
        raw = torch.empty((int(fo[-1]), 2), dtype=torch.float32, device=self.device)
        max_frames = int(np.diff(fo).max()) if n_utt else 0
        d_so, d_fo = self._dev(so), self._dev(fo)
        check(self.ctx, self.lib.mfa_pitch_batch(self.ctx, _ptr(pcm), _ptr(d_so), _ptr(d_fo), so.ctypes.data, fo.ctypes.data, n_utt,
                                                 max_frames, _ptr(raw)), "mfa_pitch_batch")
        return raw, fo

    def pitch_process(self, raw: torch.Tensor, frame_off: np.ndarray, out: Optional[torch.Tensor] = None, col0: int = 0) -> torch.Tensor:
        """ProcessPitch on the raw output: [ΣT, n_pitch_cols], or written into columns col0 … of ``out`` (a wider matrix)."""
        self._need_pitch()
        fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        n_utt = fo.shape[0] - 1
        if out is None:
            out = torch.empty((int(fo[-1]), self.num_pitch_cols), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == int(fo[-1])
        max_frames = int(np.diff(fo).max()) if n_utt else 0
        check(self.ctx, self.lib.mfa_pitch_process_batch(self.ctx, _ptr(raw), _ptr(self._dev(fo)), n_utt, max_frames, _ptr(out),
                                                         int(out.shape[1]), int(col0)), "mfa_pitch_process_batch")
        return out

    def pitch(self, pcm: torch.Tensor, sample_off: np.ndarray, frame_off: Optional[np.ndarray] = None) -> torch.Tensor:
        """kalpy PitchComputer.compute_pitch for a batch: [ΣT, n_pitch_cols] (POV feature, normalised log-pitch, raw
        log-pitch, each if configured)."""
        raw, fo = self.pitch_raw(pcm, sample_off, frame_off)
        return self.pitch_process(raw, fo)

    def base_features(self, pcm: torch.Tensor, sample_off: np.ndarray):
        """The base matrix of a use_pitch model: (float32 [ΣT, num_ceps + n_pitch_cols] = MFCC columns followed by the pitch
        columns, frame_off), rows by the paste rule of ``paste_frame_offsets``.  The tracker always runs over its own frame
        count (its trace-back starts at its last frame); a row the paste drops is dropped afterwards, as paste-feats does."""
        self._need_pitch()
        if self.mfcc_opts is None:
            self.configure_mfcc()
        so = np.ascontiguousarray(sample_off, dtype=np.int64)
        pfo = self.pitch_frame_offsets(so)
        fo = self.paste_frame_offsets(self.frame_offsets(so), pfo)
        mfcc, _ = self.mfcc(pcm, so, fo)        # (fewer rows than the MFCC has: its frames do not depend on each other)
        nc = self.num_ceps
        base = torch.empty((int(fo[-1]), nc + self.num_pitch_cols), dtype=torch.float32, device=self.device)
        base[:, :nc] = mfcc
        raw, _ = self.pitch_raw(pcm, so, pfo)
        if np.array_equal(pfo, fo):
            self.pitch_process(raw, pfo, base, nc)
        else:
            rows = np.repeat(pfo[:-1] - fo[:-1], np.diff(fo)) + np.arange(int(fo[-1]), dtype=np.int64)
            base[:, nc:] = self.pitch_process(raw, pfo)[self._dev(rows)]
        return base, fo

    def pad_cmvn_stats(self, stats: torch.Tensor, n_extra: int) -> torch.Tensor:
        """Speaker CMVN statistics [n_spk, 2, dim + 1] of the MFCC columns → [n_spk, 2, dim + n_extra + 1] with zero sums in
        the pitch columns (the count stays last): the feature kernel's offset −(0 / count) leaves those columns as they are —
        pitch is pasted AFTER CMVN in the reference (MFA/alignment/multiprocessing.py:1290-1294)."""
        n_spk, _, d1 = stats.shape
        out = torch.zeros((n_spk, 2, d1 + n_extra), dtype=stats.dtype, device=stats.device)
        out[:, :, : d1 - 1] = stats[:, :, : d1 - 1]
        out[:, :, -1] = stats[:, :, -1]
        return out

    # ------------------------------------------------------------------ feature codec (Kaldi CompressedMatrix, "CM")
    def compress_resident_values(self) -> int:
        """Values of the largest table the codec kernel holds in LDS; a larger one runs the same passes from memory."""
        return int(self.lib.mfa_compress_resident_values())

    def _codec_input(self, feats: torch.Tensor, frame_off, cols):
        if not (feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2 and feats.is_contiguous()):
            raise _lib.MfaHipError("compress: the features must be a contiguous float32 [frames, dim] tensor on the device")
        fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        if fo.ndim != 1 or fo.shape[0] < 1 or fo[0] < 0 or (np.diff(fo) < 0).any() or fo[-1] > feats.shape[0]:
            raise _lib.MfaHipError(f"compress: frame offsets do not lie inside the {feats.shape[0]} rows of the features")
        c0, c1 = (0, int(feats.shape[1])) if cols is None else (int(cols[0]), int(cols[1]))
        return fo, fo.shape[0] - 1, c0, c1

    def compress_round_trip(self, feats: torch.Tensor, frame_off: np.ndarray, cols: Optional[Tuple[int, int]] = None,
                            cmvn: Optional[torch.Tensor] = None, utt2spk: Optional[np.ndarray] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What a reader gets back after every utterance's columns ``cols`` = [c0, c1) (default: all) were written as one
        Kaldi CompressedMatrix table — ``kaldi_io.compress_round_trip`` per utterance, bit for bit, on the device.  Returns a
        new tensor (or ``out``, which may not be ``feats``); columns outside ``cols`` are copied through.  With ``cmvn``
        (float64 [n_spk, 2, d + 1], d >= c1) and ``utt2spk`` the speaker's mean is subtracted before the table is compressed:
        ApplyCmvn, then FinalFeatureFunction's trip through the codec."""
        fo, n_utt, c0, c1 = self._codec_input(feats, frame_off, cols)
        d_u2s = None
        if cmvn is not None:
            if utt2spk is None or len(utt2spk) != n_utt:
                raise _lib.MfaHipError("compress: CMVN statistics need one speaker row per utterance")
            if not (cmvn.is_cuda and cmvn.dtype == torch.float64 and cmvn.dim() == 3 and cmvn.shape[1] == 2 and cmvn.is_contiguous()):
                raise _lib.MfaHipError("compress: CMVN statistics must be a contiguous float64 [n_spk, 2, dim + 1] tensor on the device")
            u2s = np.ascontiguousarray(utt2spk, dtype=np.int32)
            if n_utt and (u2s.min() < 0 or u2s.max() >= cmvn.shape[0]):
                raise _lib.MfaHipError(f"compress: utt2spk names a speaker outside the {cmvn.shape[0]} rows of the CMVN statistics")
            d_u2s = self._dev(u2s)
        if out is None:
            out = torch.empty_like(feats) if (c0, c1) == (0, feats.shape[1]) and int(fo[0]) == 0 and int(fo[-1]) == feats.shape[0] \
                else feats.clone()
        elif out.shape != feats.shape or out.dtype != feats.dtype or not out.is_cuda or not out.is_contiguous():
            raise _lib.MfaHipError("compress: the output must match the features' shape and type")
        self._launch_compress(feats, self._dev(fo), n_utt, c0, c1, cmvn, d_u2s, out, None, None, None)
        return out

    def compress(self, feats: torch.Tensor, frame_off: np.ndarray, cols: Optional[Tuple[int, int]] = None):
        """The parts of every utterance's "CM" table for the writers (``kaldi_io.write_compressed_parts``), on the device:
        (global float32 [n_utt, 2] = min, range; colhdr uint16 [n_utt, c1 - c0, 4]; bytes uint8 [frames · (c1 - c0)], utterance
        k at frame_off[k] · (c1 - c0), column after column).  An utterance without rows has no table: its headers stay zero."""
        fo, n_utt, c0, c1 = self._codec_input(feats, frame_off, cols)
        nc = max(c1 - c0, 0)
        glob = torch.zeros((n_utt, 2), dtype=torch.float32, device=self.device)
        colhdr = torch.zeros((n_utt, nc, 4), dtype=torch.int16, device=self.device).view(torch.uint16)
        data = torch.empty(int(fo[-1]) * nc, dtype=torch.uint8, device=self.device)
        self._launch_compress(feats, self._dev(fo), n_utt, c0, c1, None, None, None, glob, colhdr, data)
        return glob, colhdr, data

    def compress_time(self) -> Dict[str, float]:
        """Accumulated time and launches of the codec kernel under ``kernel_timing`` (slot 7)."""
        return self._kernel_time(7)

    def pitch_time(self) -> Dict[str, float]:
        """Accumulated time and launch groups of the pitch kernels under ``kernel_timing`` (slot 6)."""
        return self._kernel_time(6)

    def frame_offsets(self, sample_off: np.ndarray) -> np.ndarray:
        frames = self.num_frames_array(np.diff(sample_off))
        return offsets(frames)

    def mfcc(self, pcm: torch.Tensor, sample_off: np.ndarray, frame_off: Optional[np.ndarray] = None):
        """pcm: int16 [ΣN] on device.  Returns (mfcc float32 [ΣT, num_ceps], frame_off host int64 [n+1])."""
        if self.mfcc_opts is None:
            self.configure_mfcc()
        assert pcm.dtype == torch.int16 and pcm.is_cuda
        if frame_off is None:
            frame_off = self.frame_offsets(sample_off)
        n_utt = len(sample_off) - 1
        total = int(frame_off[-1])
        out = torch.empty((total, self.num_ceps), dtype=torch.float32, device=self.device)
        d_so, d_fo = self._dev(sample_off.astype(np.int64)), self._dev(frame_off)
        max_frames = int(np.diff(frame_off).max()) if n_utt else 0
        self._launch_mfcc(pcm, d_so, d_fo, n_utt, max_frames, out)
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
        total = int(frame_off[-1])
        if lda is None and fmllr is not None:
            check_delta_fmllr(fmllr, dim, utt2spk)
        d_fo = self._dev(frame_off)
        d_u2s = self._dev(np.asarray(utt2spk, dtype=np.int32)) if utt2spk is not None else None
        max_frames = int(np.diff(frame_off).max()) if n_utt else 0
        out = torch.empty((total, 3 * dim if lda is None else lda.shape[0]), dtype=torch.float32, device=self.device)
        self._launch_feats(mfcc, d_fo, n_utt, max_frames, dim, d_u2s, cmvn, lda, splice_context, fmllr, out)
        return out

    def sort_pdf_list(self, pdfs: np.ndarray, first_frame: Optional[np.ndarray] = None):
        """Order a pdf list by slot class as the scoring kernels require; returns (sorted, counts[6]) or, with
        ``first_frame`` keys, (sorted, counts[6], sorted keys) with ascending keys inside each class
        (mfa_gmm_sort_pdf_list / mfa_gmm_sort_pdf_list_keyed)."""
        pdfs = np.ascontiguousarray(pdfs, dtype=np.int32).copy()
        counts = np.zeros(6, dtype=np.int32)
        if first_frame is None:
            check(self.ctx, self.lib.mfa_gmm_sort_pdf_list(self.ctx, pdfs.ctypes.data, len(pdfs), counts.ctypes.data),
                  "mfa_gmm_sort_pdf_list")
            return pdfs, counts
        keys = np.ascontiguousarray(first_frame, dtype=np.int32).copy()
        check(self.ctx, self.lib.mfa_gmm_sort_pdf_list_keyed(self.ctx, pdfs.ctypes.data, keys.ctypes.data, len(pdfs),
                                                             counts.ctypes.data), "mfa_gmm_sort_pdf_list_keyed")
        return pdfs, counts, keys

    def state_first_frames(self, fst: Fst) -> np.ndarray:
        """depth[s] = fewest arcs from the start state to s = first frame a token can sit on s (mfa_fst_first_frames)."""
        arc_off = np.ascontiguousarray(fst.arc_offsets, dtype=np.int32)
        nxt = np.ascontiguousarray(fst.arcs["nextstate"], dtype=np.int32)
        depth = np.empty(fst.num_states, dtype=np.int32)
        if self.lib.mfa_fst_first_frames(fst.num_states, arc_off.ctypes.data, nxt.ctypes.data, int(fst.start),
                                         depth.ctypes.data) != 0:
            raise _lib.MfaHipError("mfa_fst_first_frames: malformed graph")
        return depth

    def state_last_depths(self, fst: Fst, bfs_depth: Optional[np.ndarray] = None) -> np.ndarray:
        """m[s] = smallest BFS depth among the states reachable from s (mfa_fst_last_depths): non-decreasing along every
        arc — the lower bound of the lazy-scoring band."""
        arc_off = np.ascontiguousarray(fst.arc_offsets, dtype=np.int32)
        nxt = np.ascontiguousarray(fst.arcs["nextstate"], dtype=np.int32)
        bfs = np.ascontiguousarray(self.state_first_frames(fst) if bfs_depth is None else bfs_depth, dtype=np.int32)
        depth = np.zeros(fst.num_states, dtype=np.int32)
        if self.lib.mfa_fst_last_depths(fst.num_states, arc_off.ctypes.data, nxt.ctypes.data, int(fst.start), bfs.ctypes.data,
                                        depth.ctypes.data) < 0:
            raise _lib.MfaHipError("mfa_fst_last_depths: malformed graph")
        return depth

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
        n_utt = len(frame_off) - 1
        T = np.diff(frame_off)
        P = np.diff(pdf_off_host)
        ll_off = offsets(T * P)
        alloc = torch.empty if pdf_first_frame is None else torch.zeros
        out = alloc(int(ll_off[-1]), dtype=torch.float32, device=self.device)
        d_fo, d_po, d_lo = self._dev(frame_off), self._dev(pdf_off_host.astype(np.int64)), self._dev(ll_off)
        max_frames = int(T.max()) if n_utt else 0
        self._launch_score(feats, d_fo, n_utt, max_frames, pdf_list, d_po, class_counts, pdf_first_frame, d_lo, out)
        return out, ll_off, self._dev(P.astype(np.int32))

    def pack_graphs_general(self, fsts: Sequence[Fst], tm: TransitionModel) -> PackedGraphs:
        """Device layout for the general-graph decoder (mfa_align_general_batch): graphs may hold epsilon input arcs
        (ilabel 0) and states of any out-degree.  One score column per pdf, no depth keys (scores are computed densely)."""
        n = len(fsts)
        S, A, state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
        if np.any(arcs["ilabel"] < 0) or np.any(arcs["ilabel"] > tm.num_transition_ids):
            raise _lib.MfaHipError("a graph arc carries an input label outside the model's transition-ids")
        pdf_of_arc = tm.id2pdf[arcs["ilabel"]]            # -1 for epsilon arcs
        cols = np.zeros(arcs.shape[0], dtype=np.int32)
        pdf_lists, counts = [], []
        lut = np.full(tm.num_pdfs, -1, dtype=np.int32)
        for u in range(n):
            a0, a1 = int(arc_base[u]), int(arc_base[u + 1])
            pa = pdf_of_arc[a0:a1]
            emit = pa >= 0
            pl, cc = self.sort_pdf_list(np.unique(pa[emit])) if emit.any() else (np.zeros(0, np.int32), np.zeros(6, np.int32))
            lut[pl] = np.arange(pl.shape[0], dtype=np.int32)
            cols[a0:a1] = np.where(emit, lut[np.maximum(pa, 0)], 0)
            pdf_lists.append(pl)
            counts.append(cc)
        pdf_off = offsets([len(p) for p in pdf_lists])
        t = self._arc_tensors(state_off, arc_base, np.array([f.start for f in fsts], dtype=np.int32), arc_off, final, arcs,
                              self._dev(cols))
        return PackedGraphs(n, int(S.max()) if n else 0, int(A.max()) if n else 0, int(A.sum()), t,
                            self._dev(np.concatenate(pdf_lists).astype(np.int32) if n else np.zeros(0, np.int32)),
                            self._dev(pdf_off), self._dev(np.stack(counts).astype(np.int32)), pdf_off, pdf_lists)

    def _arc_tensors(self, state_off, arc_base, starts, arc_off, final, arcs, arc_col: torch.Tensor) -> Dict[str, torch.Tensor]:
        """mfa_graph_batch's arrays on the device from host arc records, one plain upload per column (``arc_col``: uploaded
        by the caller, whose staging differs)."""
        return dict(
            state_off=self._dev(state_off), arc_base=self._dev(arc_base), start=self._dev(starts),
            arc_off=self._dev(arc_off), final=self._dev(final),
            arc_next=self._dev(arcs["nextstate"].astype(np.int32)), arc_weight=self._dev(arcs["weight"].astype(np.float32)),
            arc_col=arc_col, arc_ilabel=self._dev(arcs["ilabel"].astype(np.int32)),
            arc_olabel=self._dev(arcs["olabel"].astype(np.int32)),
        )

    def align_general(self, graphs: PackedGraphs, feats: torch.Tensor, frame_off: np.ndarray, beam: float = 10.0,
                      retry_beam: float = 40.0, acoustic_scale: float = 0.1, bp_tokens_per_frame: int = 512,
                      want_frame_likes: bool = False):
        """Alignment over graphs with epsilon input arcs / wide states: dense scores, then FasterDecoder as Kaldi runs it
        (ProcessNonemitting included), one GPU thread per utterance — mfa_align_general_batch."""
        self._check_width(feats, "align_general")
        ll, ll_off, ll_cols = self.score(feats, frame_off, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts)
        out = self._align_outputs(graphs.n_utt, int(frame_off[-1]), want_frame_likes)
        opts = AlignOpts(beam, retry_beam, acoustic_scale, 0, bp_tokens_per_frame)
        gs = graphs.struct()
        d_lo, d_fo = self._dev(ll_off), self._dev(frame_off)
        h_fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        check(self.ctx, self.lib.mfa_align_general_batch(self.ctx, C.byref(gs), _ptr(ll), _ptr(d_lo), _ptr(ll_cols), _ptr(d_fo),
                                                         h_fo.ctypes.data, graphs.max_states, graphs.max_arcs, C.byref(opts),
                                                         *_out_ptrs(out)), "mfa_align_general_batch")
        return out

    @staticmethod
    def needs_general_decoder(fst: Fst) -> bool:
        """True for graphs the wavefront-parallel decoder does not take: a state with more than 64 emitting (or more than 64
        epsilon) arcs.  Epsilon input arcs as such are fine since round 3 (``pack_graphs`` stores every state's arcs [emitting | epsilon] and the decoder runs
        ProcessNonemitting after every frame)."""
        if not fst.num_arcs:
            return False
        eps = fst.arcs["ilabel"] == 0
        deg = np.diff(fst.arc_offsets)
        if not eps.any():
            return bool(int(deg.max()) > 64)
        src = np.repeat(np.arange(fst.num_states), deg)
        n_eps = np.bincount(src[eps], minlength=fst.num_states)
        return bool(int(n_eps.max()) > 64 or int((deg - n_eps).max()) > 64)

    def pack_graphs(self, fsts: Sequence[Fst], tm: TransitionModel, cluster_gap: Optional[int] = 32,
                    groups: Optional[int] = None, pool: Optional[StagingPool] = None) -> PackedGraphs:
        """Concatenate per-utterance graphs (with transition probabilities already applied) into the device layout.

        Score columns: one per (pdf, depth cluster) of the utterance.  A pdf whose arcs leave states far apart in the graph
        (the same phone in two words) gets one column per cluster of occurrences — occurrences whose BFS depths differ by
        more than ``cluster_gap``, or lie in different ``cluster_gap``-wide depth ranges, start a new column — so that the
        lazy-scoring band, which is a range of graph depths, does not have to keep the pdf alive for everything in
        between (optional silence after every word would otherwise chain into one column spanning the utterance).
        ``cluster_gap=None``: one column per pdf.

        ``groups`` (default 8, env MFA_PLAN_GROUPS): the single-block pdfs' columns are laid out in that many runs — pdf id
        mod groups — so that the lazy scoring kernel can give each run to one XCD (mfa_build_score_plan_grouped)."""
        if groups is None:
            groups = int(os.environ.get("MFA_PLAN_GROUPS", "8"))
        if cluster_gap == 32 and os.environ.get("MFA_PLAN_SPAN"):          # (diagnostics: tools/band_study.py)
            cluster_gap = int(os.environ["MFA_PLAN_SPAN"])
        n = len(fsts)
        whole = getattr(fsts, "arcs", None) is not None and len(getattr(fsts, "state_off", ())) == n + 1
        columns = whole and getattr(fsts, "arc_pdf", None) is not None and getattr(fsts, "arc_next", None) is not None \
            and getattr(fsts, "arc_off32", None) is not None
        if whole:
            # a batch from the native compiler (graph_native.FstBatch): its elements are views of these arrays
            state_off, arc_base = np.ascontiguousarray(fsts.state_off, dtype=np.int64), np.ascontiguousarray(fsts.arc_base, dtype=np.int64)
            S, A = np.diff(state_off), np.diff(arc_base)
            arc_off = fsts.arc_off32 if columns else fsts.arc_off.astype(np.int32)
            final, arcs = np.ascontiguousarray(fsts.final, dtype=np.float32), fsts.arcs
        else:
            S, A, state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
        if self.slot_class is None:
            raise _lib.MfaHipError("pack_graphs needs the acoustic model's slot classes: call load_gmm first")
        nemit = None          # emitting arcs per state, for graphs with epsilon input arcs
        if columns:
            # (the compiler produced next-state and pdf columns; an input label outside the model was refused there)
            nxt, pdf_of_arc = fsts.arc_next, fsts.arc_pdf
            if arcs.shape[0] and (fsts.min_ilabel <= 0 if getattr(fsts, "min_ilabel", None) is not None else int(pdf_of_arc.min()) < 0):
                raise _lib.MfaHipError("a natively compiled batch cannot hold epsilon input arcs")
        else:
            il = arcs["ilabel"]
            if np.any(il < 0) or np.any(il > tm.num_transition_ids):
                raise _lib.MfaHipError("a graph arc carries an input label outside the model's transition-ids")
            is_eps = il == 0
            if is_eps.any():
                # epsilon input arcs (kalpy / Kaldi-compiled graphs): every state's arcs stored [emitting | epsilon], each
                # kind in its original order — FasterDecoder's two loops never see the interleaving (include/mfa_hip.h)
                deg = np.concatenate([np.diff(f.arc_offsets) for f in fsts]).astype(np.int64)
                src = np.repeat(np.arange(deg.shape[0], dtype=np.int64), deg)
                perm = np.argsort(src * 2 + is_eps, kind="stable")
                arcs = arcs[perm]
                is_eps = is_eps[perm]
                n_eps = np.bincount(src[perm][is_eps], minlength=deg.shape[0])
                nemit = (deg - n_eps).astype(np.int32)
                if int(n_eps.max()) > 64 or int(nemit.max()) > 64:
                    raise _lib.MfaHipError("a graph state has more than 64 arcs of a kind; the device decoder supports at most 64 "
                                           "emitting and 64 epsilon arcs per state (needs_general_decoder)")
            pdf_of_arc = np.ascontiguousarray(np.where(il[perm] > 0, tm.id2pdf[np.maximum(il[perm], 0)], -1) if nemit is not None
                                              else tm.id2pdf[il], dtype=np.int32)
            nxt = np.ascontiguousarray(arcs["nextstate"], dtype=np.int32)
        # (the concatenated offsets restart at every utterance: those steps are <= 0 and do not disturb the maximum)
        if columns and getattr(fsts, "max_degree", None) is not None:
            max_deg = int(fsts.max_degree)
        else:
            max_deg = int(np.diff(arc_off).max()) if arc_off.shape[0] > 1 else 0
        if max_deg > 64 and nemit is None:
            raise _lib.MfaHipError(f"a graph state has {max_deg} arcs; the device decoder supports at most 64")
        span = 0 if cluster_gap is None else int(cluster_gap)
        pdf_class = np.ascontiguousarray(self.slot_class, dtype=np.int32)
        # columns (pdf, depth cluster) in kernel order, their depth keys, and every arc's column: one host call for the batch,
        # utterances spread over the host's threads (mfa_build_score_plans_batch); outputs land in reused pinned staging
        # buffers and travel to the device asynchronously
        total_s, total_a = int(state_off[-1]), int(arc_base[-1])
        starts = np.zeros(n, dtype=np.int32) if whole else np.array([f.start for f in fsts], dtype=np.int32)
        # ``pool``: the staging buffers of this batch (the ones a native-compiled batch already lives in, when the caller
        # compiled it with ``alloc=pool.get``); default: the engine's next pair
        in_pool = pool is not None and getattr(fsts, "staging", None) is pool
        pool = pool or self.next_staging()
        sd_all = pool.get("sd", max(total_s, 1) * 2, np.int32).reshape(-1, 2)
        cols = pool.get("cols", max(total_a, 1), np.int32)
        cp, cf, cl = (pool.get(k, max(total_a, 1), np.int32) for k in ("cp", "cf", "cl"))
        cc_all = np.zeros((max(n, 1), 6), dtype=np.int32)
        gc_all = np.zeros((max(n, 1), max(groups, 1)), dtype=np.int32)
        n_cols = np.zeros(max(n, 1), dtype=np.int32)
        bad = C.c_int32(-1)
        rc = self.lib.mfa_build_score_plans_batch(n, state_off.ctypes.data, arc_base.ctypes.data, arc_off.ctypes.data,
                                                  nxt.ctypes.data, pdf_of_arc.ctypes.data, starts.ctypes.data,
                                                  int(pdf_class.shape[0]), pdf_class.ctypes.data, span, groups,
                                                  _host_threads(), sd_all.ctypes.data, cols.ctypes.data, cp.ctypes.data,
                                                  cf.ctypes.data, cl.ctypes.data, cc_all.ctypes.data, gc_all.ctypes.data,
                                                  n_cols.ctypes.data, C.byref(bad)) if n else 0
        if rc != 0:
            raise _lib.MfaHipError(f"mfa_build_score_plan: utterance {int(bad.value)}: " +
                                   ("a pdf id outside the loaded model" if rc == -2 else
                                    "unsupported number of plan groups" if rc == -3 else "malformed graph"))
        cols = cols[:total_a]
        n_cols = n_cols[:n].astype(np.int64)
        pdf_off = offsets(n_cols)
        # utterance u's columns sit at [arc_base[u], arc_base[u] + n_cols[u]) of the column arrays: compact them
        take = np.repeat(arc_base[:-1] - pdf_off[:-1], n_cols) + np.arange(int(pdf_off[-1]), dtype=np.int64)
        pdf_all, first_all, last_all = cp[take], cf[take], cl[take]
        pdf_lists = RaggedView(pdf_all, pdf_off)
        first_frames = RaggedView(first_all, pdf_off)
        counts, group_counts = cc_all[:n], gc_all[:n]
        up = lambda a: pool.to_device(a, self.stream)       # noqa: E731  (pinned staging → device, asynchronous)
        if columns:
            # the 16-byte arc records travel once; their four columns are split on the device (strided device copies)
            flat = arcs.view(np.int32).reshape(-1)
            if not in_pool:
                stage = pool.get("arcs_copy", max(total_a, 1) * 4, np.int32)[: total_a * 4]
                stage[:] = flat
                flat = stage
            rec = up(flat).view(-1, 4)
            t = dict(
                state_off=self._dev(state_off), arc_base=self._dev(arc_base), start=self._dev(starts),
                arc_off=up(arc_off) if in_pool else self._dev(arc_off), final=up(final) if in_pool else self._dev(final),
                arc_next=rec[:, 3].contiguous(), arc_weight=rec[:, 2].contiguous().view(torch.float32),
                arc_col=up(cols), arc_ilabel=rec[:, 0].contiguous(), arc_olabel=rec[:, 1].contiguous(),
            )
            del rec
        else:
            t = self._arc_tensors(state_off, arc_base, starts, arc_off, final, arcs, up(cols))
        if nemit is not None:
            t["state_nemit"] = self._dev(nemit)
        sd_dev = up(sd_all[:total_s].reshape(-1)).view(-1, 2)
        return PackedGraphs(n, int(S.max()) if n else 0, int(A.max()) if n else 0, int(A.sum()), t, self._dev(pdf_all),
                            self._dev(pdf_off), self._dev(counts), pdf_off, pdf_lists,
                            self._dev(first_all), first_frames, self._dev(last_all),
                            sd_dev, groups,
                            self._dev(group_counts) if groups > 1 else None)

    def align(self, graphs: PackedGraphs, loglikes: torch.Tensor, ll_off: np.ndarray, ll_cols: torch.Tensor,
              frame_off: np.ndarray, beam: float = 10.0, retry_beam: float = 40.0, acoustic_scale: float = 0.1,
              max_tokens: int = 1024, bp_tokens_per_frame: int = 512, want_frame_likes: bool = False):
        """Returns device tensors: ali [ΣT], words [ΣT] (+ n_words [n]), like [n], status [n], frame_like or None."""
        total = int(frame_off[-1])
        out = self._align_outputs(graphs.n_utt, total, want_frame_likes)
        opts = AlignOpts(beam, retry_beam, acoustic_scale, max_tokens, bp_tokens_per_frame)
        d_lo, d_fo = self._dev(ll_off), self._dev(frame_off)
        self._launch_align(graphs, graphs.struct(), loglikes, d_lo, ll_cols, d_fo, total, opts, out)
        return out

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

    def align_features(self, graphs: PackedGraphs, feats: torch.Tensor, frame_off: np.ndarray, beam: float = 10.0,
                       retry_beam: float = 40.0, acoustic_scale: float = 0.1, max_tokens: int = 1024,
                       bp_tokens_per_frame: int = 512, want_frame_likes: bool = False, window: int = 64,
                       loglikes: Optional[torch.Tensor] = None):
        """features + graphs → alignments with acoustic scores evaluated lazily, window by window, for the pdfs live tokens
        can reach (mfa_align_features_batch) — the shape of GmmAligner.align_utterance(fst, feats)
        (MFA/alignment/multiprocessing.py:846-853).  Same results as ``score`` + ``align``.  ``loglikes``: optional scratch
        [Σ T·P] (zero-filled here when omitted, so tests can see which cells were written)."""
        self._check_width(feats, "align_features")
        n = graphs.n_utt
        total = int(frame_off[-1])
        T = np.diff(frame_off)
        P = np.diff(graphs.pdf_off_host)
        ll_off = offsets(T * P)
        if loglikes is None:
            loglikes = torch.zeros(int(ll_off[-1]), dtype=torch.float32, device=self.device)
        out = self._align_outputs(n, total, want_frame_likes)
        opts = AlignOpts(beam, retry_beam, acoustic_scale, max_tokens, bp_tokens_per_frame)
        gs, plan = graphs.struct(), graphs.plan()
        d_lo, d_fo, d_cols = self._dev(ll_off), self._dev(frame_off), self._dev(P.astype(np.int32))
        self._launch_align_features(graphs, gs, plan, feats, d_fo, int(T.max()) if n else 0, total, opts, int(window), loglikes,
                                    d_lo, d_cols, out)
        return dict(out, loglikes=loglikes, ll_off=ll_off)

    # ------------------------------------------------------------------ timing helpers (bench.py)
    def kernel_timing(self, enable: bool) -> None:
        check(self.ctx, self.lib.mfa_kernel_timing(self.ctx, int(enable)), "mfa_kernel_timing")

    def _kernel_time(self, slot: int) -> Dict[str, float]:
        ms, n = C.c_float(0), C.c_int(0)
        check(self.ctx, self.lib.mfa_kernel_time_ms(self.ctx, slot, C.byref(ms), C.byref(n)), "mfa_kernel_time_ms")
        return dict(ms=float(ms.value), launches=int(n.value))

    def kernel_times(self) -> Dict[str, Dict[str, float]]:
        return {name: self._kernel_time(i) for i, name in enumerate(("mfcc", "cmvn", "feats", "gmm", "viterbi"))}

    def resample_time(self) -> Dict[str, float]:
        """Accumulated time and launches of the resampling kernel under ``kernel_timing`` (kept out of ``kernel_times``: the
        benchmark's stage table lists the five stages of its step)."""
        return self._kernel_time(5)

    def reset_kernel_times(self) -> None:
        check(self.ctx, self.lib.mfa_kernel_time_reset(self.ctx), "mfa_kernel_time_reset")


class Pipeline:
    """A fixed-shape batch whose inputs, offsets, graphs and output buffers all live in HBM, so that one ``step()`` is
    nothing but the five kernel launches of the hot path (MFCC → CMVN stats → features → GMM scores → Viterbi).

    This is the unit bench.py times and the shape a corpus aligner would feed: build once per batch shape, refill the
    PCM/graph tensors, call ``step()``.
    """

    def __init__(self, engine: AlignmentEngine, pcm: torch.Tensor, sample_off: np.ndarray, utt2spk: np.ndarray,
                 graphs: PackedGraphs, lda: Optional[torch.Tensor] = None, fmllr: Optional[torch.Tensor] = None,
                 splice_context: int = 3, beam: float = 10.0, retry_beam: float = 40.0, acoustic_scale: float = 0.1,
                 max_tokens: int = 1024, bp_tokens_per_frame: int = 256, reachability: bool = True, lazy: bool = True,
                 window: int = 64):
        e = self.e = engine
        # lazy: scores are evaluated window by window for the pdfs live decoder tokens can reach
        # (mfa_align_features_batch); otherwise the (reachability-bounded) matrix is scored first, then decoded
        self.lazy = bool(lazy) and graphs.pdf_last_depth is not None
        self.window = int(window)
        # reachability: score a pdf only from the first frame a decoder token can ask for it (Kaldi evaluates its
        # decodable lazily; the dense score matrix here skips the cells that provably are never read)
        self.reachability = bool(reachability) and graphs.pdf_first_frame is not None
        dev = e.device
        self.pcm = pcm
        self.n_utt = len(sample_off) - 1
        self.graphs = graphs
        self.lda, self.fmllr, self.ctx_frames = lda, fmllr, splice_context
        self.frame_off = e.frame_offsets(sample_off)
        T = np.diff(self.frame_off)
        self.total_frames = int(self.frame_off[-1])
        self.max_frames = int(T.max())
        P = np.diff(graphs.pdf_off_host)
        self.ll_off = offsets(T * P)
        spk_ids, inv, order, spk_off = _speaker_groups(np.asarray(utt2spk, dtype=np.int32))
        self.n_spk = len(spk_ids)
        d = e._dev
        self.d_sample_off, self.d_frame_off = d(sample_off.astype(np.int64)), d(self.frame_off)
        self.d_utt2spk, self.d_spk_off, self.d_spk_utt = d(inv.astype(np.int32)), d(spk_off), d(order)
        self.d_ll_off, self.d_ll_cols = d(self.ll_off), d(P.astype(np.int32))
        self.num_ceps = e.num_ceps
        self.feat_dim = 3 * self.num_ceps if lda is None else int(lda.shape[0])
        if lda is None and fmllr is not None:
            check_delta_fmllr(fmllr, self.num_ceps, inv)
        f32 = torch.float32
        self.mfcc = torch.empty((self.total_frames, self.num_ceps), dtype=f32, device=dev)
        self.cmvn = torch.empty((self.n_spk, 2, self.num_ceps + 1), dtype=torch.float64, device=dev)
        self.feats = torch.empty((self.total_frames, self.feat_dim), dtype=f32, device=dev)
        self.loglikes = torch.empty(int(self.ll_off[-1]), dtype=f32, device=dev)
        self._out = e._align_outputs(self.n_utt, self.total_frames, False)     # (persistent: every step decodes into these)
        self.ali, self.words, self.n_words, self.like, self.status = (self._out[k] for k in ("ali", "words", "n_words", "like", "status"))
        self.opts = AlignOpts(beam, retry_beam, acoustic_scale, max_tokens, bp_tokens_per_frame)
        self.gstruct = graphs.struct()
        self._plan: Optional[ScorePlan] = None          # graphs.plan(), made by the first lazy step
        self._states_times_frames: Optional[float] = None
        # measure_scored_cells (bench.py hands one pipeline's figures to the others of the same shape)
        self.cells_scored = self.cells_scored_fraction = self.scored_flops = None
        # algorithmic work of one step: GMM flops 4·D·g·P·T summed over utterances
        # With reachability a (frame, pdf) cell is algorithmically needed only from the pdf's first possible frame on.
        g_of_pdf = np.diff(e.gmm.pdf_offsets).astype(np.float64)
        cells = 0.0
        for u, pl in enumerate(graphs.pdf_lists_host):
            if self.reachability and graphs.pdf_first_frame_host is not None:
                live = np.clip(float(T[u]) - graphs.pdf_first_frame_host[u].astype(np.float64), 0.0, None)
            else:
                live = np.full(len(pl), float(T[u]))
            cells += float((g_of_pdf[pl] * live).sum())
        self.gmm_flops = 4.0 * e.gmm.dim * cells
        self.audio_seconds = float(np.diff(sample_off).sum() / e.mfcc_opts.sample_frequency)

    def step(self) -> None:
        self.front()
        if self.lazy:
            self.score_and_decode()
        else:
            self.score()
            self.decode()

    def score_and_decode(self) -> None:
        """features + graphs → alignments, scores evaluated lazily per window (mfa_align_features_batch)."""
        if self._plan is None:
            self._plan = self.graphs.plan()
        self.e._launch_align_features(self.graphs, self.gstruct, self._plan, self.feats, self.d_frame_off, self.max_frames,
                                      self.total_frames, self.opts, self.window, self.loglikes, self.d_ll_off, self.d_ll_cols,
                                      self._out)

    # ---- host side of the boundary: alignments land in (pinned) host memory
    def host_output_buffers(self, pinned: bool = True) -> Dict[str, torch.Tensor]:
        out = {}
        for name in ("ali", "words", "n_words", "like", "status"):
            t = getattr(self, name)
            out[name] = torch.empty(t.shape, dtype=t.dtype, pin_memory=pinned)
        return out

    def outputs_to_host(self, host: Dict[str, torch.Tensor]) -> None:
        """Asynchronous D2H of ali / words / n_words / like / status on the engine's stream."""
        for name, dst in host.items():
            dst.copy_(getattr(self, name), non_blocking=True)

    # ---- bench.py reporting helpers
    def scores_string(self) -> str:
        if self.lazy:
            return (f"lazy: per {self.window}-frame window, only the pdfs arcs within {self.window} arcs of the live tokens "
                    "can emit (a superset of what Kaldi's lazy decodable evaluates)")
        return "reachable cells only (pdf j from its first possible frame on)" if self.reachability else "dense T x P"

    def dtype_string(self, mono: bool, gauss_per_pdf: int) -> str:
        split, f16 = _split_passes(mono, gauss_per_pdf)
        if f16:
            return "f32 scores from 2-way f16-split products (3*2^-22 per term worst case), f64 path costs"
        if split:
            return "f32 scores from 3-way bf16-split products (2^-24 per term), f64 path costs"
        return "f32 (scores), f64 (path costs)"

    def algorithmic_bytes(self, score_cells_read: Optional[float] = None) -> Dict[str, float]:
        """SURVEY §8(d) staged-pipeline bytes of one step, per stage (each tensor written once and read once).  The score
        matrix counts for what is actually moved: the scoring stage writes the cells it computes, the decoder reads
        ``score_cells_read`` cells (counted by the oracle's lazy decodable on a sample — the device decoder asks for exactly
        the same cells) or, without that count, at most the cells written."""
        T = np.diff(self.frame_off).astype(np.float64)
        P = np.diff(self.graphs.pdf_off_host).astype(np.float64)
        n_samples = float(self.pcm.numel())
        A = float(self.graphs.total_arcs)
        S = float(self.graphs.tensors["final"].numel())
        D = float(self.feat_dim)
        tot = float(T.sum())
        written = self.cells_scored if self.lazy else None
        if written is None:
            written = float((P * T).sum())
        if score_cells_read is not None:
            read, how = float(score_cells_read), "4 B x cells the decoder read (oracle's lazy-decodable count on the CPU sample, scaled to the batch)"
        else:
            read, how = written, "4 B x cells the scoring stage wrote (upper bound of the cells the decoder read)"
        if self._states_times_frames is None:
            self._states_times_frames = float((T * np.diff(self.graphs.tensors["state_off"].cpu().numpy())).sum())
        return {
            "mfcc": 2.0 * n_samples + 4.0 * self.num_ceps * tot,
            "feats": 4.0 * self.num_ceps * tot + 4.0 * D * tot,
            "gmm": 4.0 * D * tot + 4.0 * written,                  # model slice cache-resident (SURVEY's 6.0 MB variant)
            "viterbi": 4.0 * read + 16.0 * A + 2.0 * self._states_times_frames + 6.0 * tot,
            "viterbi_score_bytes_how": how,
            "states": S,
        }

    def measure_scored_cells(self) -> Dict[str, float]:
        """One step on a zero-filled score scratch: which cells did the scoring kernels write?  Returns the count, the
        fraction of the T x P matrix, and the flops those cells cost (4*D*g per cell, g = Gaussians of the cell's pdf) —
        the work the scoring stage EXECUTES, which is what bench.py's roofline prices."""
        self.loglikes.zero_()
        self.step()
        torch.cuda.synchronize(self.e.device)
        g_of_pdf = torch.from_numpy(np.diff(self.e.gmm.pdf_offsets).astype(np.float64)).to(self.e.device)
        pdf_list = self.graphs.pdf_list.long()
        T = np.diff(self.frame_off)
        cells = torch.zeros((), dtype=torch.float64, device=self.e.device)
        weighted = torch.zeros((), dtype=torch.float64, device=self.e.device)
        po = self.graphs.pdf_off_host
        for u in range(self.n_utt):
            a, b = int(self.ll_off[u]), int(self.ll_off[u + 1])
            if b == a:
                continue
            per_col = (self.loglikes[a:b].view(int(T[u]), -1) != 0).sum(dim=0).to(torch.float64)
            cells += per_col.sum()
            weighted += (per_col * g_of_pdf[pdf_list[int(po[u]): int(po[u + 1])]]).sum()
        self.cells_scored = float(cells.item())
        self.cells_scored_fraction = self.cells_scored / max(1, self.loglikes.numel())
        self.scored_flops = 4.0 * self.e.gmm.dim * float(weighted.item())
        return {"cells": self.cells_scored, "fraction": self.cells_scored_fraction, "flops": self.scored_flops}

    def roofline(self, dominant: str, ktimes: Dict[str, Dict[str, float]], steps: int, mono: bool, gauss_per_pdf: int,
                 score_cells_read: Optional[float] = None) -> Dict:
        """Roofline object for a stage of the step (bench.py): per-step stage time from the HIP-event timers.  Everything
        priced here is work the kernels EXECUTE: scoring = the cells the lazy path wrote (``measure_scored_cells``), the
        decoder's score bytes = the cells it read (``score_cells_read`` when the oracle counted them on a sample, else the
        cells written — an upper bound)."""
        ms = ktimes[dominant]["ms"] / max(1, steps)
        launches = ktimes[dominant]["launches"] / max(1, steps)
        lazy_measured = self.lazy and self.scored_flops is not None
        if dominant == "gmm":
            split, f16 = _split_passes(mono, gauss_per_pdf)
            mult = 3.0 if f16 else (6.0 if split else 1.0)
            peak = 2500.0 if split else 157.3
            flops = self.scored_flops if lazy_measured else self.gmm_flops
            ach = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            equiv = self.gmm_flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            return {"kernel": "diagonal-GMM scoring (" + ("f16x2" if f16 else "bf16x3" if split else "f32") + " MFMA)",
                    "kernel_key": "gmm", "bound": "mfma", "achieved": round(ach, 3), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(ach / peak, 4), "traffic": None,
                    "executed_flops_per_step": flops, "mfma_flops_per_algorithmic_flop": int(mult),
                    "executed_mfma_tflops": round(mult * ach, 3), "executed_mfma_frac_of_peak": round(mult * ach / peak, 4),
                    "cells_scored_fraction": self.cells_scored_fraction,
                    "algorithmic_equivalent_tflops": round(equiv, 3), "ms_per_step": round(ms, 4), "launches_per_step": launches,
                    "note": "achieved = 4*D*g flops of the (frame, pdf) cells the scoring kernels actually computed / stage time; "
                            "executed_mfma_* = the same times the split-operand products per term; algorithmic_equivalent_tflops "
                            "prices every cell of the reachability-bounded matrix (what a dense scorer would do) and is NOT work done"}
        by = self.algorithmic_bytes(score_cells_read)
        b = by.get(dominant, 0.0)
        gbs = b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        names = {"viterbi": "viterbi kernels (beam Viterbi, one wavefront per utterance)", "mfcc": "mfcc_kernel",
                 "feats": "feats_lda_kernel / feats_kernel", "cmvn": "cmvn kernels"}
        out = {"kernel": names.get(dominant, dominant), "kernel_key": dominant, "bound": "hbm", "achieved": round(gbs, 2),
               "peak": 8000.0, "unit": "GB/s", "frac": round(gbs / 8000.0, 5), "traffic": None,
               "algorithmic_bytes_per_step": b, "ms_per_step": round(ms, 4), "launches_per_step": launches,
               "note": "algorithmic bytes = SURVEY 8(d) staged-pipeline bytes of this stage (each tensor written once, read once)"}
        if dominant == "viterbi":
            out["score_bytes"] = by["viterbi_score_bytes_how"]
        return out

    def front(self) -> None:
        """PCM → MFCC → CMVN statistics → final features (three launches on the engine's stream)."""
        e = self.e
        e._launch_mfcc(self.pcm, self.d_sample_off, self.d_frame_off, self.n_utt, self.max_frames, self.mfcc)
        e._launch_cmvn_stats(self.mfcc, self.d_frame_off, self.n_utt, self.num_ceps, self.d_spk_off, self.d_spk_utt, self.n_spk,
                             self.cmvn)
        e._launch_feats(self.mfcc, self.d_frame_off, self.n_utt, self.max_frames, self.num_ceps, self.d_utt2spk, self.cmvn,
                        self.lda, self.ctx_frames, self.fmllr, self.feats)

    def score(self) -> None:
        """features → GMM log-likelihoods of every utterance's pdf list."""
        g = self.graphs
        self.e._launch_score(self.feats, self.d_frame_off, self.n_utt, self.max_frames, g.pdf_list, g.pdf_off, g.class_counts,
                             g.pdf_first_frame if self.reachability else None, self.d_ll_off, self.loglikes)

    def decode(self) -> None:
        """log-likelihoods + graphs → alignments (beam Viterbi, retry beam for the utterances that need it)."""
        self.e._launch_align(self.graphs, self.gstruct, self.loglikes, self.d_ll_off, self.d_ll_cols, self.d_frame_off,
                             self.total_frames, self.opts, self._out)


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


def fmllr_statistics(engine: "AlignmentEngine", feats: torch.Tensor, frame_off: np.ndarray, ali: torch.Tensor,
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
        po = np.ascontiguousarray(stats_model.pdf_offsets, dtype=np.int32)
        mi = np.ascontiguousarray(stats_model.means_invvars, dtype=np.float32)
        iv = np.ascontiguousarray(stats_model.inv_vars, dtype=np.float32)
        check(engine.ctx, engine.lib.mfa_fmllr_stats_model(engine.ctx, stats_model.dim, stats_model.num_pdfs, po.ctypes.data,
                                                           mi.ctypes.data, iv.ctypes.data), "mfa_fmllr_stats_model")
    else:
        check(engine.ctx, engine.lib.mfa_fmllr_stats_model(engine.ctx, 0, 0, None, None, None), "mfa_fmllr_stats_model")
    id2pdf = torch.from_numpy(np.maximum(tm.id2pdf, 0).astype(np.int32)).to(dev)
    sil = np.zeros(tm.id2phone.shape[0], dtype=np.float32)
    sil[np.isin(tm.id2phone, np.asarray(list(silence_phones), dtype=np.int64))] = 1.0
    w_host = np.where(sil > 0, np.float32(silence_weight), np.float32(1.0)).astype(np.float32)
    w_host[0] = 0.0
    w_of_tid = torch.from_numpy(w_host).to(dev)
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


def tid_tables(tm: TransitionModel, weights: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The two host-built tables of mfa_gmm_acc_batch: pdf of every transition-id (int32; index 0 unused) and its frame
    weight (float32; 1 for every id but 0 unless ``weights`` [transition-ids + 1] is given)."""
    id2pdf = np.maximum(tm.id2pdf, 0).astype(np.int32)
    w = np.ones(id2pdf.shape[0], dtype=np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32).copy()
    if w.shape != id2pdf.shape:
        raise ValueError(f"weights: {w.shape[0]} entries for {id2pdf.shape[0] - 1} transition-ids (+ 1)")
    w[0] = 0.0
    return id2pdf, w


def gmm_statistics(engine: "AlignmentEngine", feats: torch.Tensor, ali: torch.Tensor, tm: TransitionModel,
                   weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None) -> GmmStats:
    """GMM statistics of one batch from its alignments (mfa_gmm_acc_batch; the contract is in include/mfa_hip.h), with the
    model loaded in the engine.

    ``feats`` float32 [ΣT, dim] and ``ali`` int32 [ΣT] transition-ids on the device (0 where an utterance failed: those frames
    take no part); ``weights``: per transition-id frame weights (default 1).  ``into``: statistics to add to — the device sums
    start from its values, so a corpus accumulated batch by batch is one chain of additions — and the object returned."""
    if engine.gmm is None:
        raise _lib.MfaHipError("gmm_statistics: no acoustic model loaded (AlignmentEngine.load_gmm)")
    dev = engine.device
    gmm = engine.gmm
    G, D = gmm.num_gauss, gmm.dim
    id2pdf, w = tid_tables(tm, weights)
    n_tids = int(id2pdf.shape[0])
    st = into if into is not None else GmmStats.zeros(G, D, n_tids)
    if st.mean_acc.shape != (G, D) or st.tid_count.shape != (n_tids,):
        raise ValueError("gmm_statistics: `into` does not fit the loaded model")
    total = int(ali.shape[0])
    if feats.shape[0] != total or (total and feats.shape[1] != D):
        raise _lib.MfaHipError(f"gmm_statistics: features {tuple(feats.shape)} for {total} frames of a model of dim {D}")
    if feats.dtype != torch.float32 or not feats.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError("gmm_statistics: features must be float32 and, like the alignments, on the device")
    feats = feats.contiguous()
    ali = ali.to(torch.int32).contiguous()
    occ = torch.from_numpy(st.occ).to(dev)
    mean = torch.from_numpy(np.ascontiguousarray(st.mean_acc)).to(dev)
    var = torch.from_numpy(np.ascontiguousarray(st.var_acc)).to(dev)
    tot = torch.tensor([st.tot_like, st.tot_count], dtype=torch.float64, device=dev)
    cnt = torch.from_numpy(st.tid_count).to(dev)
    d_pdf, d_w = torch.from_numpy(id2pdf).to(dev), torch.from_numpy(w).to(dev)
    check(engine.ctx, engine.lib.mfa_gmm_acc_batch(engine.ctx, _ptr(feats), total, _ptr(ali), _ptr(d_pdf), _ptr(d_w), n_tids,
                                                    _ptr(occ), _ptr(mean), _ptr(var), _ptr(tot), _ptr(cnt)), "mfa_gmm_acc_batch")
    st.occ, st.mean_acc, st.var_acc, st.tid_count = occ.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), cnt.cpu().numpy()
    t = tot.cpu().numpy()
    st.tot_like, st.tot_count = float(t[0]), float(t[1])
    return st


def gmm_statistics_host(gmm: DiagGmmModel, feats: np.ndarray, ali: np.ndarray, tm: TransitionModel,
                        weights: Optional[np.ndarray] = None, into: Optional[GmmStats] = None, want_post: bool = False):
    """The same call on the host twin (mfa_debug_gmm_acc_host: no device, frames in ascending index): the specification the
    device is held to.  numpy arrays in; with ``want_post`` also returns every frame's posteriors [ΣT, largest pdf]."""
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
    po = np.ascontiguousarray(gmm.pdf_offsets, dtype=np.int32)
    gc = np.ascontiguousarray(gmm.gconsts, dtype=np.float32)
    mi = np.ascontiguousarray(gmm.means_invvars, dtype=np.float32)
    iv = np.ascontiguousarray(gmm.inv_vars, dtype=np.float32)
    occ, mean, var = (np.ascontiguousarray(a, dtype=np.float64) for a in (st.occ, st.mean_acc, st.var_acc))
    tot = np.array([st.tot_like, st.tot_count], dtype=np.float64)
    cnt = np.ascontiguousarray(st.tid_count, dtype=np.int64)
    stride = int(np.diff(po).max())
    post = np.zeros((ali.shape[0], stride), dtype=np.float32) if want_post else None
    rc = lib.mfa_debug_gmm_acc_host(D, gmm.num_pdfs, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data,
                                    feats.ctypes.data, int(ali.shape[0]), pdf.ctypes.data, fw.ctypes.data, ali.ctypes.data, n_tids,
                                    occ.ctypes.data, mean.ctypes.data, var.ctypes.data, tot.ctypes.data, cnt.ctypes.data,
                                    None if post is None else post.ctypes.data, stride)
    if rc != 0:
        raise _lib.MfaHipError(f"mfa_debug_gmm_acc_host: {'a pdf of more than 128 Gaussians' if rc == -2 else 'bad arguments'}")
    st.occ, st.mean_acc, st.var_acc, st.tid_count = occ, mean, var, cnt
    st.tot_like, st.tot_count = float(tot[0]), float(tot[1])
    return (st, post) if want_post else st
