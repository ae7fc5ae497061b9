"""Stages around the MFCC: sample-rate conversion ahead of it, pitch and voicing pasted after CMVN, the 8-bit feature
codec (Kaldi CompressedMatrix), and speech activity (energy VAD, sliding-window CMVN, voiced-frame selection with
subsampling, voiced runs) — ``FrontEndStages``, methods of ``AlignmentEngine``; the speech-activity stage's host twins
as functions.

Uses of the engine: ``lib``, ``ctx``, ``device``, ``_dev``, ``_launch_compress``, ``_launch_vad`` / ``_launch_sliding_cmvn`` /
``_launch_select_count`` / ``_launch_select`` / ``_launch_vad_runs`` / ``_launch_scan``; ``mfcc_opts`` / ``num_ceps`` /
``configure_mfcc`` / ``frame_offsets`` / ``mfcc`` (the MFCC stage); its own fields ``pitch_opts`` and ``num_pitch_cols``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PitchOpts, SlidingCmvnOpts, VadOpts, _ptr, check
from .ragged import max_len, offsets

# Kaldi's PitchExtractionOptions / ProcessPitchOptions at MFA's values (MFA/models.py:551-576 sets max_f0 800 and
# snip_edges True; Kaldi's own max_f0 is 400)
DEFAULT_PITCH = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, min_f0=50.0, max_f0=800.0,
                     soft_min_f0=10.0, penalty_factor=0.1, lowpass_cutoff=1000.0, resample_frequency=4000.0, delta_pitch=0.005,
                     nccf_ballast=7000.0, preemphasis=0.0, pov_scale=2.0, pov_offset=0.0, pitch_scale=2.0,
                     lowpass_filter_width=1, upsample_filter_width=5, snip_edges=1, normalization_context=75,
                     add_pov_feature=1, add_normalized_log_pitch=1, add_raw_log_pitch=0, add_delta_pitch=0)
_PITCH_ALIAS = {"frame_length": "frame_length_ms", "frame_shift": "frame_shift_ms"}    # kalpy's names (milliseconds)

# Kaldi's VadEnergyOptions (kalpy VadComputer's arguments; the reference's segmenter passes energy_threshold 5.5) and
# SlidingWindowCmnOptions (the reference's speaker-task archive: cmn_window 300, center)
DEFAULT_VAD = dict(energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6, frames_context=0)
_VAD_ALIAS = {"vad_energy_threshold": "energy_threshold", "vad_energy_mean_scale": "energy_mean_scale",
              "vad_frames_context": "frames_context", "vad_proportion_threshold": "proportion_threshold"}
DEFAULT_SLIDING_CMVN = dict(cmn_window=600, min_window=100, center=0, norm_vars=0)


class FrontEndStages:
    pitch_opts: Optional[PitchOpts] = None      # configure_pitch
    num_pitch_cols = 0

    # ------------------------------------------------------------------ sample-rate conversion (ahead of the MFCC)
    def model_rate(self) -> int:
        """The rate the MFCC is configured for (``sample_frequency``), in whole Hz: what every utterance is brought to."""
        if self.mfcc_opts is None:
            self.configure_mfcc()
        f = float(self.mfcc_opts.sample_frequency)
        if f != int(f):
            raise _lib.MfaHipError(f"the resampler takes whole rates in Hz (sample_frequency is {f})")
        return int(f)

    def _rate_vector(self, rates: Sequence[Optional[int]], n: int) -> np.ndarray:
        """Per-utterance rates as int64 [n], the model's rate where none is given."""
        target = self.model_rate()
        return np.fromiter((target if x is None else int(x) for x in rates), dtype=np.int64, count=n)

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
        r = self._rate_vector(rates, n.shape[0])
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
        r = self._rate_vector(rates, so.shape[0] - 1)
        if not np.any(r != target):
            return pcm, so
        out_len = self.num_resampled_array(np.diff(so), r)
        oo = offsets(out_len)
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
        opts = _lib.options(PitchOpts, DEFAULT_PITCH, kw, "pitch", _PITCH_ALIAS)
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
        return int(self.lib.mfa_pitch_workspace_bytes(self.ctx, len(ns), int(ns.sum()), int(nf.sum()), max_len(sample_off),
                                                      max_len(frame_off)))

    def pitch_raw(self, pcm: torch.Tensor, sample_off: np.ndarray, frame_off: Optional[np.ndarray] = None):
        """pcm: int16 [ΣN] on device at the pitch options' sample_frequency.  Returns (raw float32 [ΣT, 2] = (POV NCCF, pitch in
        Hz) per frame, frame_off): the tracker's output before ProcessPitch (mfa_pitch_batch).  ``frame_off``, when given,
        must hold the tracker's own frame counts."""
        self._need_pitch()
        assert pcm.dtype == torch.int16 and pcm.is_cuda
        so = np.ascontiguousarray(sample_off, dtype=np.int64)
        fo = self.pitch_frame_offsets(so) if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
        raw = torch.empty((int(fo[-1]), 2), dtype=torch.float32, device=self.device)
        d_so, d_fo = self._dev(so), self._dev(fo)
        check(self.ctx, self.lib.mfa_pitch_batch(self.ctx, _ptr(pcm), _ptr(d_so), _ptr(d_fo), so.ctypes.data, fo.ctypes.data,
                                                 so.shape[0] - 1, max_len(fo), _ptr(raw)), "mfa_pitch_batch")
        return raw, fo

    def pitch_process(self, raw: torch.Tensor, frame_off: np.ndarray, out: Optional[torch.Tensor] = None, col0: int = 0) -> torch.Tensor:
        """ProcessPitch on the raw output: [ΣT, n_pitch_cols], or written into columns col0 … of ``out`` (a wider matrix)."""
        self._need_pitch()
        fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        if out is None:
            out = torch.empty((int(fo[-1]), self.num_pitch_cols), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == int(fo[-1])
        check(self.ctx, self.lib.mfa_pitch_process_batch(self.ctx, _ptr(raw), _ptr(self._dev(fo)), fo.shape[0] - 1, max_len(fo),
                                                         _ptr(out), int(out.shape[1]), int(col0)), "mfa_pitch_process_batch")
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

    # ------------------------------------------------------------------ speech activity (energy VAD, sliding CMVN, selection, runs)
    def _ragged_input(self, x: torch.Tensor, frame_off, what: str, dims: int = 2, dtype=torch.float32):
        """A contiguous device tensor whose rows are exactly the batch's frames, and its offsets (int64, from 0)."""
        if not (x.is_cuda and x.dtype == dtype and x.dim() == dims and x.is_contiguous()):
            raise _lib.MfaHipError(f"{what}: the input must be a contiguous {dtype} tensor of {dims} dimension(s) on the device")
        fo = np.ascontiguousarray(frame_off, dtype=np.int64)
        if fo.ndim != 1 or fo.shape[0] < 1 or fo[0] != 0 or (np.diff(fo) < 0).any() or fo[-1] != x.shape[0]:
            raise _lib.MfaHipError(f"{what}: frame offsets must run from 0 to the {x.shape[0]} rows of the input")
        return fo, fo.shape[0] - 1

    def vad_scan_block_frames(self) -> int:
        """Frames per block of the per-utterance integer scan (mfa_vad_scan_block_frames); one workgroup scans the block sums,
        a thread of it more than one beyond ``vad_scan_totals_threads()`` blocks."""
        return int(self.lib.mfa_vad_scan_block_frames())

    def vad_scan_totals_threads(self) -> int:
        return int(self.lib.mfa_vad_scan_totals_threads())

    def sliding_cmvn_tile_frames(self) -> int:
        return int(self.lib.mfa_sliding_cmvn_tile_frames())

    def segment_scan(self, values: torch.Tensor, frame_off: np.ndarray):
        """The scan the stage rests on, by itself: (exclusive scan of int32 ``values`` inside every utterance, the utterances'
        sums)."""
        fo, n_utt = self._ragged_input(values, frame_off, "scan", 1, torch.int32)
        scan = torch.empty_like(values)
        totals = torch.empty(n_utt, dtype=torch.int32, device=self.device)
        self._launch_scan(values, self._dev(fo), n_utt, int(fo[-1]), scan, totals)
        return scan, totals

    def vad(self, feats: torch.Tensor, frame_off: np.ndarray, **opts):
        """Kaldi's energy VAD on column 0 of ``feats`` (MFCC with use_energy: the log energy).  Options: ``DEFAULT_VAD``.
        Returns (vad float32 [ΣT] of 1.0 / 0.0 — what compute-vad writes —, thresholds float32 [n_utt], voiced counts int32
        [n_utt]).  The reference's adaptive mode is ``energy_threshold=0, energy_mean_scale=1``."""
        o = _lib.options(VadOpts, DEFAULT_VAD, opts, "VAD", _VAD_ALIAS)
        fo, n_utt = self._ragged_input(feats, frame_off, "VAD")
        vad = torch.empty(int(fo[-1]), dtype=torch.float32, device=self.device)
        thr = torch.empty(n_utt, dtype=torch.float32, device=self.device)
        voiced = torch.empty(n_utt, dtype=torch.int32, device=self.device)
        self._launch_vad(feats, self._dev(fo), n_utt, int(fo[-1]), max_len(fo), o, vad, thr, voiced)
        return vad, thr, voiced

    def sliding_cmvn(self, feats: torch.Tensor, frame_off: np.ndarray, dim: Optional[int] = None, **opts) -> torch.Tensor:
        """Kaldi's SlidingWindowCmn (apply-cmvn-sliding) on the first ``dim`` columns (default: all) of every utterance; the
        other columns are copied.  Options: ``DEFAULT_SLIDING_CMVN``.  A new tensor."""
        o = _lib.options(SlidingCmvnOpts, DEFAULT_SLIDING_CMVN, opts, "sliding CMVN")
        fo, n_utt = self._ragged_input(feats, frame_off, "sliding CMVN")
        out = torch.empty_like(feats)
        self._launch_sliding_cmvn(feats, self._dev(fo), n_utt, max_len(fo), int(feats.shape[1]) if dim is None else int(dim), o, out)
        return out

    def select_frames(self, feats: torch.Tensor, frame_off: np.ndarray, vad: Optional[torch.Tensor] = None, subsample_n: int = 1):
        """select-voiced-frames (rows with ``vad`` != 0; None: all) then subsample-feats ``subsample_n`` (rows 0, n, 2n, … of
        what remains).  Returns (features, frame_off) of the rows kept.  One scan, one gather; the host waits once, for
        the new offsets."""
        fo, n_utt = self._ragged_input(feats, frame_off, "frame selection")
        if vad is not None and (not vad.is_cuda or vad.dtype != torch.float32 or vad.dim() != 1 or vad.shape[0] != feats.shape[0]
                                or not vad.is_contiguous()):
            raise _lib.MfaHipError("frame selection: the VAD vector must be a contiguous float32 tensor on the device, one value per row")
        src = torch.empty(int(fo[-1]), dtype=torch.int32, device=self.device)
        d_out_off = torch.empty(n_utt + 1, dtype=torch.int64, device=self.device)
        self._launch_select_count(vad, self._dev(fo), n_utt, int(fo[-1]), int(subsample_n), src, d_out_off)
        out_off = d_out_off.cpu().numpy()
        out = torch.empty((int(out_off[-1]), int(feats.shape[1])), dtype=torch.float32, device=self.device)
        self._launch_select(feats, src, int(out_off[-1]), out)
        return out, out_off

    def vad_runs(self, vad: torch.Tensor, frame_off: np.ndarray, capacity: Optional[int] = None):
        """The maximal runs of voiced frames of every utterance: (run_begin int32 [R], run_end int32 [R] = last frame + 1, both
        relative to the utterance, run_off int64 [n_utt + 1]) as host arrays.  The first call brings room for ``capacity``
        runs (default: a run per 16 frames and one per utterance); when the batch has more it is run again with room for
        all of them, which cannot fall short."""
        fo, n_utt = self._ragged_input(vad, frame_off, "voiced runs", 1)
        total = int(fo[-1])
        cap = min((total + 1) // 2 + n_utt, total // 16 + n_utt) if capacity is None else int(capacity)
        d_fo = self._dev(fo)
        run_off = torch.empty(n_utt + 1, dtype=torch.int64, device=self.device)
        while True:
            begin = torch.empty(cap, dtype=torch.int32, device=self.device)
            end = torch.empty(cap, dtype=torch.int32, device=self.device)
            self._launch_vad_runs(vad, d_fo, n_utt, total, cap, begin, end, run_off)
            ro = run_off.cpu().numpy()
            if int(ro[-1]) <= cap:
                return begin[: int(ro[-1])].cpu().numpy(), end[: int(ro[-1])].cpu().numpy(), ro
            cap = int(ro[-1])


# ---------------------------------------------------------------------- the host twins of the speech-activity stage
# (csrc/vad_host.cpp: the kernels' arithmetic in their order on host arrays; no context, no device — tests and tools)
def _host_offsets(frame_off) -> np.ndarray:
    return np.ascontiguousarray(frame_off, dtype=np.int64)


def _twin(rc: int, what: str) -> None:
    if rc != 0:
        raise _lib.MfaHipError(f"{what}: arguments refused")


def vad_scan_host(values: np.ndarray, frame_off):
    v, fo = np.ascontiguousarray(values, dtype=np.int32), _host_offsets(frame_off)
    scan, totals = np.empty_like(v), np.empty(fo.shape[0] - 1, dtype=np.int32)
    _twin(_lib.lib().mfa_debug_vad_scan_host(v.ctypes.data, fo.ctypes.data, fo.shape[0] - 1, scan.ctypes.data, totals.ctypes.data), "scan twin")
    return scan, totals


def vad_host(feats: np.ndarray, frame_off, **opts):
    x, fo = np.ascontiguousarray(feats, dtype=np.float32), _host_offsets(frame_off)
    o = _lib.options(VadOpts, DEFAULT_VAD, opts, "VAD", _VAD_ALIAS)
    n = fo.shape[0] - 1
    vad, thr, voiced = np.empty(x.shape[0], dtype=np.float32), np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32)
    _twin(_lib.lib().mfa_debug_vad_host(x.ctypes.data, x.shape[1], fo.ctypes.data, n, C.byref(o), vad.ctypes.data, thr.ctypes.data,
                                        voiced.ctypes.data), "VAD twin")
    return vad, thr, voiced


def sliding_cmvn_host(feats: np.ndarray, frame_off, dim: Optional[int] = None, **opts) -> np.ndarray:
    x, fo = np.ascontiguousarray(feats, dtype=np.float32), _host_offsets(frame_off)
    o = _lib.options(SlidingCmvnOpts, DEFAULT_SLIDING_CMVN, opts, "sliding CMVN")
    out = np.empty_like(x)
    _twin(_lib.lib().mfa_debug_sliding_cmvn_host(x.ctypes.data, fo.ctypes.data, fo.shape[0] - 1, x.shape[1] if dim is None else int(dim),
                                                 x.shape[1], C.byref(o), out.ctypes.data), "sliding CMVN twin")
    return out


def select_frames_host(feats: np.ndarray, frame_off, vad: Optional[np.ndarray] = None, subsample_n: int = 1):
    fo = _host_offsets(frame_off)
    v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float32)
    src, out_off = np.empty(int(fo[-1]), dtype=np.int32), np.empty(fo.shape[0], dtype=np.int64)
    _twin(_lib.lib().mfa_debug_select_frames_host(None if v is None else v.ctypes.data, fo.ctypes.data, fo.shape[0] - 1, int(subsample_n),
                                                  src.ctypes.data, out_off.ctypes.data), "selection twin")
    return np.asarray(feats)[src[: int(out_off[-1])]], out_off


def vad_runs_host(vad: np.ndarray, frame_off):
    v, fo = np.ascontiguousarray(vad, dtype=np.float32), _host_offsets(frame_off)
    cap = (int(fo[-1]) + 1) // 2 + fo.shape[0]
    begin, end, run_off = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32), np.empty(fo.shape[0], dtype=np.int64)
    _twin(_lib.lib().mfa_debug_vad_runs_host(v.ctypes.data, fo.ctypes.data, fo.shape[0] - 1, cap, begin.ctypes.data, end.ctypes.data,
                                             run_off.ctypes.data), "runs twin")
    return begin[: int(run_off[-1])], end[: int(run_off[-1])], run_off
