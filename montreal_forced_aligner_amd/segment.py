"""Speech-activity segmentation: `mfa segment` without SpeechBrain — MFCC with energy, Kaldi's energy VAD, the runs of
voiced frames, merged segments (MFA/vad/multiprocessing.py:324-406, MFA/vad/models.py:44-130).

``get_initial_segmentation`` and ``merge_segments`` are specifications of the reference's two functions, restated with
their quirks; ``segments_from_runs`` reaches the same intervals from the device's (first frame, last frame + 1) runs without
visiting a frame — the reference walks 360 000 frames per hour of audio in a Python loop.  ``VadSegmenter`` runs MFCC, VAD and
runs for a whole batch of recordings in one pass over the device.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import ctm as _ctm
from .ctm import CtmInterval

# SegmenterMixin / VadConfigMixin of the reference
DEFAULT_SEGMENTATION = dict(max_segment_length=30.0, min_pause_duration=0.333, min_segment_length=0.333)
DEFAULT_VAD_OPTIONS = dict(energy_threshold=5.5, energy_mean_scale=0.5)


def get_initial_segmentation(frames: np.ndarray, frame_shift: float) -> List[CtmInterval]:
    """One "speech" interval per maximal run of frames with int(f) > 0.  A run begins at its first frame · frame_shift; a run
    followed by a silent frame i ends at (i − 1) · frame_shift — the START of its last voiced frame, so a run of one frame is
    an empty interval —; a run that reaches the end of the file ends at len(frames) · frame_shift."""
    segments: List[CtmInterval] = []
    cur: Optional[CtmInterval] = None
    n = frames.shape[0]
    for i in range(n):
        if int(frames[i]) > 0:
            if cur is None:
                cur = CtmInterval(begin=i * frame_shift, end=0, label="speech")
        elif cur is not None:
            cur.end = (i - 1) * frame_shift
            segments.append(cur)
            cur = None
    if cur is not None:
        cur.end = n * frame_shift
        segments.append(cur)
    return segments


def segments_from_runs(run_begin: Sequence[int], run_end: Sequence[int], n_frames: int, frame_shift: float) -> List[CtmInterval]:
    """``get_initial_segmentation`` from the runs of voiced frames (first frame, last frame + 1) of a vector of ``n_frames``
    frames: the same products of the same integers with ``frame_shift``, so the same floats."""
    out = []
    for b, e in zip(np.asarray(run_begin).tolist(), np.asarray(run_end).tolist()):
        out.append(CtmInterval(begin=b * frame_shift, end=(n_frames if e == n_frames else e - 1) * frame_shift, label="speech"))
    return out


def merge_segments(segments: List[CtmInterval], min_pause_duration: float, max_segment_length: float, min_segment_length: float,
                   snap_boundaries: bool = True) -> List[CtmInterval]:
    """A segment joins the one before it unless the pause between them exceeds ``min_pause_duration`` or the joined segment
    would be longer than ``max_segment_length``.  At a boundary that stays, both sides move half the gap towards each other,
    at most ``min_pause_duration / 4`` each.  Last, only segments with end − begin > ``min_segment_length`` are kept.  (The
    intervals handed in are changed, as the reference changes them.)"""
    merged: List[CtmInterval] = []
    snap = min_pause_duration / 2 if snap_boundaries else 0
    for s in segments:
        if not merged or s.begin > merged[-1].end + min_pause_duration or s.end - merged[-1].begin > max_segment_length:
            if merged and snap:
                gap = s.begin - merged[-1].end
                half = gap / 2 if gap < snap else snap / 2
                merged[-1].end += half
                s.begin -= half
            merged.append(s)
        else:
            merged[-1].end = s.end
    return [x for x in merged if x.end - x.begin > min_segment_length]


def _forced_mfcc(mfcc_options: Optional[dict]) -> Tuple[dict, float]:
    """(the MFCC options under the engine's names with what the segmenter forces, MFA/vad/multiprocessing.py:332-335; the
    frame shift in seconds)."""
    from .kalpy_api import MfccComputer

    opts = dict(mfcc_options or {})
    opts.update(use_energy=True, raw_energy=False, dither=0.0, energy_floor=0.0)
    mc = MfccComputer(**opts)
    return {k: (int(v) if isinstance(v, bool) else v) for k, v in mc._opts.items()}, mc.frame_shift


def _segment_batch(engine, pcms: Sequence[np.ndarray], rates: Sequence[Optional[int]], mfcc_options: dict, vad_options: dict,
                   segmentation_options: dict, adaptive: bool, allow_empty: bool) -> Tuple[List[List[CtmInterval]], np.ndarray]:
    """MFCC, VAD and runs of a batch on the device, the merge on the host.  Returns (segments per recording, frame counts)."""
    eng_opts, frame_shift = _forced_mfcc(mfcc_options)
    vo = dict(DEFAULT_VAD_OPTIONS, **(vad_options or {}))
    if adaptive:      # the threshold is the mean of c0 and the mean scale 0: one code path, energy_threshold 0 and scale 1
        vo.update(energy_threshold=0.0, energy_mean_scale=1.0)
    so_opts = dict(DEFAULT_SEGMENTATION, **(segmentation_options or {}))
    # the MFCC options are state of the engine, shared with whoever aligns on it: the forced set is in force for this call only
    before = engine.mfcc_opts
    engine.configure_mfcc(**eng_opts)
    try:
        d_pcm, so = engine.gather_pcm([np.ascontiguousarray(p, dtype=np.int16) for p in pcms])
        d_pcm, so = engine.resample(d_pcm, so, list(rates))
        feats, fo = engine.mfcc(d_pcm, so)
    finally:
        engine.configure_mfcc(**({} if before is None else {f: getattr(before, f) for f, _ in before._fields_}))
    vad, _thr, _cnt = engine.vad(feats, fo, **vo)
    begin, end, run_off = engine.vad_runs(vad, fo)
    out = []
    for k in range(len(pcms)):
        a, b = int(run_off[k]), int(run_off[k + 1])
        initial = segments_from_runs(begin[a:b], end[a:b], int(fo[k + 1] - fo[k]), frame_shift)
        out.append(merge_segments(initial, so_opts["min_pause_duration"], so_opts["max_segment_length"],
                                  so_opts["min_segment_length"] if allow_empty else 0.02))
    return out, np.diff(fo)


def segment_utterance_vad(engine, pcm: np.ndarray, sample_rate: Optional[int], mfcc_options: Optional[dict] = None,
                          vad_options: Optional[dict] = None, segmentation_options: Optional[dict] = None, adaptive: bool = True,
                          allow_empty: bool = True, begin: float = 0.0) -> List[CtmInterval]:
    """The reference's ``segment_utterance_vad`` for one recording (int16 mono at ``sample_rate``; None: the model's rate):
    "speech" intervals in seconds, shifted by ``begin``.  MFCCs are computed with use_energy, raw_energy False, no dither and
    energy_floor 0 whatever ``mfcc_options`` says.  ``adaptive``: the threshold is the mean of c0 (a float64 mean here; numpy's
    float32 pairwise mean, which the reference takes, can differ from it in the last bit)."""
    segs, _ = _segment_batch(engine, [pcm], [sample_rate], mfcc_options, vad_options, segmentation_options, adaptive, allow_empty)
    for s in segs[0]:
        s.begin += begin
        s.end += begin
    return segs[0]


class VadSegmenter:
    """``VadSegmenter(engine, **options)`` with the reference's option names and defaults (SegmenterMixin: max_segment_length 30,
    min_pause_duration 0.333, min_segment_length 0.333; VadConfigMixin: energy_threshold 5.5, energy_mean_scale 0.5); other
    keywords are MFCC options under MFA's names."""

    def __init__(self, engine, max_segment_length: float = 30.0, min_pause_duration: float = 0.333, min_segment_length: float = 0.333,
                 energy_threshold: float = 5.5, energy_mean_scale: float = 0.5, adaptive: bool = True, allow_empty: bool = True,
                 **mfcc_options):
        self.engine = engine
        self.segmentation_options = dict(max_segment_length=max_segment_length, min_pause_duration=min_pause_duration,
                                         min_segment_length=min_segment_length)
        self.vad_options = dict(energy_threshold=energy_threshold, energy_mean_scale=energy_mean_scale)
        self.adaptive, self.allow_empty = adaptive, allow_empty
        self.mfcc_options = mfcc_options
        self.recordings: List[Tuple[str, np.ndarray, Optional[int]]] = []
        self.segments: Dict[str, List[CtmInterval]] = {}

    def segment(self, recordings: Sequence[Tuple[str, np.ndarray, Optional[int]]]) -> Dict[str, List[CtmInterval]]:
        """(name, int16 mono samples, their rate in Hz or None) per recording → its "speech" intervals.  The whole batch goes
        through the resampler (when rates differ from the model's), the MFCC, the VAD and the runs in one pass."""
        recordings = [(str(n), np.ascontiguousarray(p, dtype=np.int16), r) for n, p, r in recordings]
        segs, _ = _segment_batch(self.engine, [p for _, p, _ in recordings], [r for _, _, r in recordings], self.mfcc_options,
                                 self.vad_options, self.segmentation_options, self.adaptive, self.allow_empty)
        self.recordings = recordings
        self.segments = {n: s for (n, _, _), s in zip(recordings, segs)}
        return self.segments

    def _rate(self, rate: Optional[int]) -> int:
        return self.engine.model_rate() if rate is None else int(rate)

    def export_files(self, output_directory, output_format: str = "long_textgrid") -> List[Path]:
        """One TextGrid per recording of the last ``segment`` call (tier of the recording's name, intervals labelled "speech")."""
        out_dir = Path(output_directory)
        out_dir.mkdir(parents=True, exist_ok=True)
        frame_shift = _forced_mfcc(self.mfcc_options)[1]
        paths = []
        for name, pcm, rate in self.recordings:
            path = out_dir / (name + (".TextGrid" if output_format.endswith("textgrid") else "." + output_format))
            data = {name: {"segments": [CtmInterval(s.begin, s.end, s.label) for s in self.segments[name]]}}
            _ctm.export_textgrid(data, path, pcm.shape[0] / self._rate(rate), frame_shift, output_format)
            paths.append(path)
        return paths

    def utterances(self) -> Iterator:
        """The segments of the last ``segment`` call as ``CorpusUtterance`` slices of their recordings (text empty: the
        transcriber's or the user's to fill), in the form ``CorpusAligner.align`` takes for segmented audio."""
        from .aligner import CorpusUtterance

        for name, pcm, rate in self.recordings:
            sr = self._rate(rate)
            for k, s in enumerate(self.segments[name]):
                a, b = max(int(round(s.begin * sr)), 0), min(int(round(s.end * sr)), pcm.shape[0])
                yield CorpusUtterance(f"{name}-{k}", name, pcm[a:b], "", begin=a / sr, file_name=name,
                                      file_duration=pcm.shape[0] / sr, sample_rate=rate)
