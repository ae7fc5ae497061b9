"""Host-side mirror of the kalpy objects MFA's alignment path calls — same names, argument meaning and
error behaviour, backed by libmfa_hip.so instead of Kaldi.

With these in place ``align_utterance_online``-style code (MFA/online/alignment.py:29-123) runs unchanged:

    graph_compiler = TrainingGraphCompiler(model_path, tree_path, lexicon_compiler)
    utterance.generate_mfccs(mfcc_computer); cmvn = CmvnComputer().compute_cmvn_from_features([utterance.mfccs])
    utterance.apply_cmvn(cmvn); feats = utterance.generate_features(mfcc_computer, None, lda_mat=…, fmllr_trans=…)
    fst = graph_compiler.compile_fst(text)
    aligner = GmmAligner(model_path, beam=10, retry_beam=40, transition_scale=1.0, acoustic_scale=0.1, self_loop_scale=0.1)
    alignment = aligner.align_utterance(fst, feats)          # None when the utterance cannot be aligned
    ctm = lexicon_compiler.phones_to_pronunciations(alignment.words, alignment.generate_ctm(tm, phone_table, shift), …)

Matrices cross this API as numpy arrays (kalpy: FloatMatrix/DoubleMatrix).  Every numeric step runs on the GPU through
the C ABI; a missing library or GPU raises ``MfaHipError`` — there is no CPU path.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from . import ctm as _ctm
from . import graph as _graph
from . import kaldi_io
from . import model as _model
from .graph import LexiconCompiler as _LexiconCompiler
from .graph import Pronunciation as KalpyPronunciation  # noqa: F401  (name used by the reference)
from .ragged import offsets

logger = logging.getLogger("kalpy.align")      # the reference's per-job logger name (MFA/utils.py:1435-1476)

_ENGINE = None


def get_engine(device: int = 0):
    """One engine per process (the reference: one aligner object per worker, never shared across processes)."""
    global _ENGINE
    if _ENGINE is None:
        from .engine import AlignmentEngine

        _ENGINE = AlignmentEngine(device)
    return _ENGINE


# ------------------------------------------------------------------------------------------------ audio / features
def _model_rate() -> int:
    """The rate audio is brought to: the engine's configured ``sample_frequency``, or the default before an engine exists."""
    if _ENGINE is not None and _ENGINE.mfcc_opts is not None:
        return _ENGINE.model_rate()
    from .engine import DEFAULT_MFCC

    return int(DEFAULT_MFCC["sample_frequency"])


def _to_model_rate(eng, pcm: np.ndarray, rate: int) -> np.ndarray:
    import torch

    d = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.int16).copy()).to(eng.device)
    out, _ = eng.resample(d, np.array([0, pcm.shape[0]], dtype=np.int64), [rate])
    return out.cpu().numpy()


class Segment:
    """``Segment(path, begin, end, channel)`` — PCM16 wav at any rate from 1 to 384 kHz.  ``sample_rate`` is the file's rate
    (known once the file has been read)."""

    def __init__(self, file_path, begin: Optional[float] = None, end: Optional[float] = None, channel: int = 0):
        self.file_path = str(file_path)
        self.begin, self.end, self.channel = begin, end, channel or 0
        self.sample_rate: Optional[int] = None

    def load_native(self) -> Tuple[np.ndarray, int]:
        """(samples of the segment at the file's own rate, that rate): ``begin`` / ``end`` cut at the native rate."""
        pcm, sr = kaldi_io.read_wav_pcm16(self.file_path)
        self.sample_rate = int(sr)
        x = pcm[min(self.channel, pcm.shape[0] - 1)]
        b = 0 if self.begin is None else int(round(self.begin * sr))
        e = x.shape[0] if self.end is None else int(round(self.end * sr))
        return np.ascontiguousarray(x[b:e]), int(sr)

    def load_audio(self) -> np.ndarray:
        """The segment at the model's rate, as the reference's ``librosa.load(sr=16000)`` hands it over
        (MFA/db_polars.py:1992): a file at another rate is cut at its own rate, then converted on the device
        (Kaldi's LinearResample, include/mfa_hip.h — not librosa's resampler, which is outside the parity domain)."""
        x, sr = self.load_native()
        if sr == _model_rate():
            return x
        return _to_model_rate(get_engine(), x, sr)


class MfccComputer:
    """``MfccComputer(**mfcc_options)`` with MFA's option names (MFA/corpus/features.py:780-820)."""

    # (allow_downsample / allow_upsample are options of this object, not of the kernel: see ``_load``)
    _MAP = dict(sample_frequency="sample_frequency", frame_length="frame_length_ms", frame_shift="frame_shift_ms",
                preemphasis_coefficient="preemphasis", low_frequency="low_frequency", high_frequency="high_frequency",
                cepstral_lifter="cepstral_lifter", energy_floor="energy_floor", num_mel_bins="num_mel_bins",
                num_coefficients="num_coefficients", snip_edges="snip_edges", remove_dc_offset="remove_dc_offset",
                use_energy="use_energy", raw_energy="raw_energy")

    def __init__(self, **options):
        self.parameters = dict(options)
        dither = options.get("dither", 0.0)
        if dither not in (0, 0.0, None):
            raise ValueError("dither must be 0: dithered features are random and outside the parity domain")
        self._opts = {self._MAP[k]: v for k, v in options.items() if k in self._MAP and v is not None}
        self.frame_shift = float(options.get("frame_shift", 10)) / 1000.0
        # Kaldi's defaults are False (a wave at another rate is an error); MFA passes True for both (MFA/corpus/features.py:605-607)
        self.allow_downsample = bool(options.get("allow_downsample", False))
        self.allow_upsample = bool(options.get("allow_upsample", False))

    def _configure(self):
        eng = get_engine()
        eng.configure_mfcc(**{k: (int(v) if isinstance(v, bool) else v) for k, v in self._opts.items()})
        return eng

    def _load(self, segment: Union[Segment, np.ndarray]) -> Tuple[np.ndarray, Optional[int]]:
        """(samples, their rate or None for an array, which is taken to be at the model's rate).  A file the options do not
        allow to be converted is refused here, on the host (Kaldi: "Waveform and config sample Frequency mismatch")."""
        if not isinstance(segment, Segment):
            return np.ascontiguousarray(segment, dtype=np.int16), None
        pcm, sr = segment.load_native()
        from .engine import DEFAULT_MFCC

        target = float(self._opts.get("sample_frequency", DEFAULT_MFCC["sample_frequency"]))
        if sr > target and not self.allow_downsample:
            raise kaldi_io.KaldiFormatError(f"{segment.file_path}: {sr} Hz audio, the features are configured for "
                                            f"{target:g} Hz and allow_downsample is False")
        if sr < target and not self.allow_upsample:
            raise kaldi_io.KaldiFormatError(f"{segment.file_path}: {sr} Hz audio, the features are configured for "
                                            f"{target:g} Hz and allow_upsample is False")
        return pcm, (None if sr == target else sr)

    def compute_mfccs(self, segment: Union[Segment, np.ndarray]) -> np.ndarray:
        import torch

        pcm, rate = self._load(segment)          # (refusals come before any device work)
        eng = self._configure()
        d, so = torch.from_numpy(pcm.copy()).to(eng.device), np.array([0, pcm.shape[0]], dtype=np.int64)
        if rate is not None:
            d, so = eng.resample(d, so, [rate])
        out, _ = eng.mfcc(d, so)
        return out.cpu().numpy()

    def compute_mfccs_for_export(self, segment, compress: bool = True):
        """``compress=True``: the matrix wrapped so that ``kaldi_io.write_ark_entry`` stores it as a Kaldi CompressedMatrix
        (what MfccFunction writes, MFA/corpus/features.py:235); ``compress=False``: the float32 matrix (FineTuneFunction)."""
        m = self.compute_mfccs(segment)
        return CompressedFeatures(m) if compress else m

    def export_feats(self, file_name, segments: Iterable[Tuple[str, Union["Segment", np.ndarray]]], write_scp: bool = True,
                     compress: bool = True, batch_size: int = 256) -> None:
        """``feats.*.ark`` (+ ``.scp``) for (key, segment) pairs, MFCCs computed in device batches (MfccFunction._run)."""
        import torch

        ark = Path(file_name)
        scp = ark.with_suffix(".scp") if write_scp else None
        lines = []
        eng = None
        with open(ark, "wb") as f:
            batch: List[Tuple[str, np.ndarray, Optional[int]]] = []

            def flush():
                nonlocal eng
                if not batch:
                    return
                if eng is None:
                    eng = self._configure()
                so = offsets([len(x) for _, x, _ in batch])
                d = torch.from_numpy(np.concatenate([x for _, x, _ in batch])).to(eng.device)
                d, so = eng.resample(d, so, [r for _, _, r in batch])       # the whole batch in one call (a launch per rate)
                out, fo = eng.mfcc(d, so)
                if compress:          # headers and bytes from the device codec: a quarter of the float bytes come back
                    nc = int(out.shape[1])
                    glob, colhdr, data = (t.cpu().numpy() for t in eng.compress(out, fo))
                    for i, (key, _, _) in enumerate(batch):
                        f.write(key.encode("utf8") + b" ")
                        off = f.tell()
                        f.write(b"\0B")
                        rows = int(fo[i + 1] - fo[i])
                        kaldi_io.write_compressed_parts(f, glob[i], colhdr[i], data[fo[i] * nc: fo[i + 1] * nc], rows, nc)
                        lines.append(f"{key} {ark}:{off}\n")
                else:
                    out = out.cpu().numpy()
                    for i, (key, _, _) in enumerate(batch):
                        off = kaldi_io.write_ark_entry(f, key, out[fo[i]: fo[i + 1]], "matrix")
                        lines.append(f"{key} {ark}:{off}\n")
                batch.clear()

            for key, seg in segments:
                pcm, rate = self._load(seg)
                batch.append((key, pcm, rate))
                if len(batch) >= batch_size:
                    flush()
            flush()
        if scp is not None:
            scp.write_text("".join(lines), encoding="utf8")


class PitchComputer:
    """``PitchComputer(**pitch_options)`` with kalpy's option names (MFA/corpus/features.py:687-688; MFA/models.py:551-576):
    Kaldi's ComputeKaldiPitch + ProcessPitch on the device (include/mfa_hip.h, "Pitch and voicing").  Options not given take
    Kaldi's defaults (max_f0 400, snip_edges True, POV and normalised log-pitch and DELTA-pitch on) — MFA names every flag;
    ``add_delta_pitch=True`` is refused: Kaldi adds Gaussian noise to delta-pitch, which has no parity domain.
    Like MfccComputer, every call puts this object's options in force on the process's engine (``get_engine()``; nothing is
    rebuilt when they already are): an aligner that shares that engine must use the same pitch options."""

    _KALDI = dict(max_f0=400.0, snip_edges=True, add_pov_feature=True, add_normalized_log_pitch=True, add_delta_pitch=True,
                  add_raw_log_pitch=False)

    def __init__(self, **options):
        from .engine import DEFAULT_PITCH, _PITCH_ALIAS

        self.parameters = dict(options)
        opts = dict(self._KALDI)
        for k, v in options.items():
            if v is None:
                continue
            if _PITCH_ALIAS.get(k, k) not in DEFAULT_PITCH:
                raise KeyError(f"unknown pitch option {k!r}")
            opts[k] = v
        if opts["add_delta_pitch"]:
            raise ValueError("add_delta_pitch must be False: Kaldi adds Gaussian noise to delta-pitch, which is outside the parity domain")
        self._opts = {k: (int(v) if isinstance(v, bool) else v) for k, v in opts.items()}
        self.frame_shift = float(options.get("frame_shift", 10)) / 1000.0
        self.sample_frequency = float(options.get("sample_frequency", DEFAULT_PITCH["sample_frequency"]))

    def _configure(self):
        eng = get_engine()
        eng.configure_pitch(**self._opts)
        return eng

    def _pcm(self, eng, segment: Union[Segment, np.ndarray]):
        """(device int16 samples at the options' rate, sample offsets): a file at another rate goes through the device
        resampler first, as it does ahead of the MFCC — which the engine must then be configured for at the same rate."""
        import torch

        if not isinstance(segment, Segment):
            pcm, rate = np.ascontiguousarray(segment, dtype=np.int16), None
        else:
            pcm, sr = segment.load_native()
            rate = None if sr == self.sample_frequency else sr
        d, so = torch.from_numpy(pcm.copy()).to(eng.device), np.array([0, pcm.shape[0]], dtype=np.int64)
        if rate is not None:
            if float(eng.model_rate()) != self.sample_frequency:
                raise kaldi_io.KaldiFormatError(f"{segment.file_path}: {rate} Hz audio would be converted to the MFCC's "
                                                f"{eng.model_rate()} Hz, the pitch options name {self.sample_frequency:g} Hz")
            d, so = eng.resample(d, so, [rate])
        return d, so

    def compute_pitch(self, segment: Union[Segment, np.ndarray]) -> np.ndarray:
        """float32 [T, columns]: POV feature, normalised log-pitch, raw log-pitch, each if its flag is set."""
        eng = self._configure()
        d, so = self._pcm(eng, segment)
        return eng.pitch(d, so).cpu().numpy()

    def compute_pitch_for_export(self, segment, compress: bool = True):
        m = self.compute_pitch(segment)
        return CompressedFeatures(m) if compress else m


def paste_feats(mats: Sequence[np.ndarray], tolerance: int = 0) -> np.ndarray:
    """Kaldi paste-feats: the matrices side by side, cut to the shortest when their row counts differ by at most
    ``tolerance``; a larger difference raises."""
    rows = [int(m.shape[0]) for m in mats]
    if max(rows) - min(rows) > tolerance:
        raise kaldi_io.KaldiFormatError(f"paste_feats: row counts {rows} differ by more than {tolerance}")
    return np.concatenate([np.asarray(m, dtype=np.float32)[: min(rows)] for m in mats], axis=1)


class CompressedFeatures(np.ndarray):
    """A float32 matrix tagged for 8-bit storage: ``FeatureArchive``/``write_features`` write it as Kaldi "CM"."""

    def __new__(cls, m):
        return np.asarray(m, dtype=np.float32).view(cls)


class CmvnComputer:
    def compute_cmvn_from_features(self, feats: Sequence[np.ndarray]) -> np.ndarray:
        """Kaldi layout float64 [2, dim+1]: sums + count / sums of squares."""
        import torch

        eng = get_engine()
        frame_off = offsets([f.shape[0] for f in feats])
        d = torch.from_numpy(np.concatenate(feats).astype(np.float32)).to(eng.device)
        return eng.cmvn_stats(d, frame_off, np.zeros(len(feats), dtype=np.int32), 1).cpu().numpy()[0]


    def export_cmvn(self, file_name, feature_archive, spk2utt: Dict[str, Sequence[str]], write_scp: bool = True) -> None:
        """Per-speaker statistics → ``cmvn.ark`` (+ ``.scp``) of float64 [2, dim+1] matrices keyed by speaker
        (calc_cmvn, MFA/corpus/acoustic_corpus.py:1315-1367).  ``feature_archive``: (utt key, matrix) pairs or a dict."""
        feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
        entries = []
        for spk in sorted(spk2utt):
            mats = [np.asarray(feats[u]) for u in spk2utt[spk] if u in feats]
            if mats:
                entries.append((str(spk), self.compute_cmvn_from_features(mats)))
        ark = Path(file_name)
        kaldi_io.write_table(ark, entries, "matrix", ark.with_suffix(".scp") if write_scp else None)


# apply-cmvn-sliding as the reference's speaker-task archive runs it (FinalFeatureFunction, MFA/corpus/features.py:284-342)
SLIDING_CMVN_ARCHIVE = dict(cmn_window=300, center=1, norm_vars=0)


class VadComputer:
    """``VadComputer(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6)``: Kaldi's
    energy VAD (compute-vad) on column 0 of a feature matrix, on the device."""

    def __init__(self, energy_threshold: float = 5.0, energy_mean_scale: float = 0.5, frames_context: int = 0,
                 proportion_threshold: float = 0.6):
        self.options = dict(energy_threshold=float(energy_threshold), energy_mean_scale=float(energy_mean_scale),
                            frames_context=int(frames_context), proportion_threshold=float(proportion_threshold))

    def compute_vad(self, feats: np.ndarray) -> np.ndarray:
        """float32 [T] of 1.0 / 0.0, one per frame."""
        return self._batch([np.asarray(feats)])[0]

    def _batch(self, mats: Sequence[np.ndarray]) -> List[np.ndarray]:
        import torch

        eng = get_engine()
        fo = offsets([m.shape[0] for m in mats])
        d = torch.from_numpy(np.ascontiguousarray(np.concatenate(mats), dtype=np.float32)).to(eng.device)
        vad = eng.vad(d, fo, **self.options)[0].cpu().numpy()
        return [vad[fo[i]: fo[i + 1]].copy() for i in range(len(mats))]

    def export_vad(self, file_name, feature_archive, write_scp: bool = False, callback=None, batch_size: int = 256) -> None:
        """``vad.ark`` (+ ``.scp``) of float vectors keyed by utterance for (utt key, matrix) pairs; an utterance without
        frames is skipped, as compute-vad skips it.  ``callback(n)`` after every batch of n utterances."""
        ark = Path(file_name)
        entries, batch = [], []

        def flush():
            entries.extend(zip([k for k, _ in batch], self._batch([m for _, m in batch])))
            if callback is not None:
                callback(len(batch))
            batch.clear()

        for key, m in (feature_archive.items() if isinstance(feature_archive, dict) else feature_archive):
            if np.asarray(m).shape[0] == 0:
                logger.warning("Empty feature matrix for utterance %s", key)
                continue
            batch.append((key, np.asarray(m)))
            if len(batch) >= batch_size:
                flush()
        if batch:
            flush()
        kaldi_io.write_table(ark, entries, "vector", ark.with_suffix(".scp") if write_scp else None)


class FeatureArchive:
    """``FeatureArchive(scp, utt2spk=, cmvn_file_name=, lda_mat_file_name=, transform_file_name=, deltas=, …)``: iterable of
    (utt_id, final feature matrix) — Job.construct_feature_archive's chain (MFA/db.py:2101-2136): base features from the
    scp (compressed or not) → sliding-window CMVN (``use_sliding_cmvn``: cmn_window 300, centred) or else per-speaker CMVN →
    Δ+ΔΔ or splice(±3)+LDA → per-speaker fMLLR → the voiced frames of ``vad_file_name`` → every ``subsample_n``-th of them.
    An utterance whose VAD vector is missing, of another length than its features, or without a voiced frame is skipped with
    a warning (select-voiced-frames).  Utterances are pushed through the device in batches of ``batch_size``; ``utt2spk`` is
    a dict or a Kaldi utt2spk file.  kalpy and Kaldi being absent where this was written, the order of the last three steps and
    the sliding window's options are restated from their published behaviour, unpinned."""

    def __init__(self, file_name, utt2spk=None, cmvn_file_name=None, lda_mat_file_name=None, transform_file_name=None,
                 vad_file_name=None, deltas: bool = False, splices: bool = False, splice_frames: int = 3, subsample_n: int = 0,
                 use_sliding_cmvn: bool = False, batch_size: int = 256, stages=None):
        if subsample_n < 0:
            raise NotImplementedError("subsample-feats with a negative n (Kaldi's offset form) is not built")
        self.subsample_n = int(subsample_n) or 1
        self.use_sliding_cmvn = bool(use_sliding_cmvn)
        self.vad_read_specifier = vad_file_name
        self._stages = stages        # the stage methods' owner (default: the process's engine); tensors live on its ``device``
        self.file_name = Path(file_name)
        self.utt2spk = self._read_map(utt2spk)
        self.cmvn_read_specifier = cmvn_file_name
        self.lda_mat_file_name = lda_mat_file_name
        self.transform_read_specifier = transform_file_name
        self.use_splices = bool(splices or lda_mat_file_name)
        self.use_deltas = bool(deltas) and not self.use_splices
        self.splice_frames = splice_frames
        self.batch_size = batch_size
        self._entries = kaldi_io.read_scp(self.file_name) if self.file_name.suffix == ".scp" else None
        self._cache: Dict[str, bytes] = {}
        self._cmvn = self._read_table(cmvn_file_name)
        self._trans = self._read_table(transform_file_name)
        self._vad = self._read_table(vad_file_name, "vector")
        self._lda = None if lda_mat_file_name is None else kaldi_io.read_matrix_file(Path(lda_mat_file_name).read_bytes())
        if self._trans is not None and self._lda is None and not self.use_deltas:
            # CMVN-only features are not final features: the reference transforms after the deltas or the LDA (MFA/db.py:2101-2136)
            raise NotImplementedError("transform_file_name needs deltas=True or an LDA matrix: nothing here applies it to CMVN-only features")

    @staticmethod
    def _read_map(m):
        if m is None or isinstance(m, dict):
            return m
        return dict(line.split()[:2] for line in Path(m).read_text(encoding="utf8").splitlines() if line.strip())

    def _read_table(self, name, kind: str = "matrix") -> Optional[Dict[str, np.ndarray]]:
        if name is None:
            return None
        name = Path(name)
        if name.suffix == ".scp":
            return {k: kaldi_io.read_scp_object(self._cache, p, o, kind) for k, p, o in kaldi_io.read_scp(name)}
        return dict(kaldi_io.read_ark(name.read_bytes(), kind))

    def _base(self) -> Iterator[Tuple[str, np.ndarray]]:
        if self._entries is not None:
            for key, path, off in self._entries:
                yield key, kaldi_io.read_scp_object(self._cache, path, off, "matrix")
        else:
            yield from kaldi_io.read_ark(self.file_name.read_bytes(), "matrix")

    def cmvn_rows(self, ids: Dict[str, int], dim: int) -> Optional[np.ndarray]:
        """The CMVN statistics [len(ids), 2, dim + 1] of the speakers ``ids`` (name → row), or None without a CMVN table."""
        if self._cmvn is None:
            return None
        st = np.zeros((len(ids), 2, dim + 1), dtype=np.float64)
        st[:, 0, dim] = 1.0   # a speaker without statistics keeps its features (mean 0 over count 1)
        for s, i in ids.items():
            if s in self._cmvn:
                st[i] = self._cmvn[s]
        return st

    @staticmethod
    def noop_cmvn_rows(n_spk: int, dim: int) -> np.ndarray:
        """Statistics that leave the features as they are: the "mean 0 over count 1" row of ``cmvn_rows`` for every speaker."""
        st = np.zeros((n_spk, 2, dim + 1), dtype=np.float64)
        st[:, 0, dim] = 1.0
        return st

    def base_rows(self) -> Iterator[Tuple[str, np.ndarray, str]]:
        """(utt_id, base feature matrix as stored, speaker name): for a consumer that applies CMVN (``cmvn_rows``) and
        splices (``splice_frames``) on the device itself — ``LdaStatsAccumulator``."""
        for key, m in self._base():
            yield key, m, (self.utt2spk.get(key, key) if self.utt2spk else key)

    def __iter__(self) -> Iterator[Tuple[str, np.ndarray]]:
        import torch

        eng = self._stages if self._stages is not None else get_engine()
        batch: List[Tuple[str, np.ndarray]] = []

        def flush():
            if self._vad is not None:      # select-voiced-frames: such an utterance is skipped with a warning
                kept = []
                for k, m in batch:
                    v = self._vad.get(k)
                    if v is None:
                        logger.warning("No VAD input found for utterance %s", k)
                    elif v.shape[0] != m.shape[0]:
                        logger.warning("Mismatch in number of frames %d for features and VAD %d, for utterance %s", m.shape[0], v.shape[0], k)
                    elif not np.any(v != 0):
                        logger.warning("No features voiced for utterance %s", k)
                    else:
                        kept.append((k, m))
                batch[:] = kept
                if not batch:
                    return []
            spk_names = [self.utt2spk.get(k, k) if self.utt2spk else k for k, _ in batch]
            ids = {s: i for i, s in enumerate(dict.fromkeys(spk_names))}
            u2s = np.array([ids[s] for s in spk_names], dtype=np.int32)
            dim = batch[0][1].shape[1]
            st = self.cmvn_rows(ids, dim)
            if self.use_sliding_cmvn:      # instead of the speakers' CMVN: the feature kernel gets "mean 0 over count 1" rows
                st = None if not (self.use_deltas or self._lda is not None) else self.noop_cmvn_rows(len(ids), dim)
            cm = None if st is None else torch.from_numpy(st).to(eng.device)
            lda = None if self._lda is None else torch.from_numpy(self._lda.astype(np.float32)).to(eng.device)
            fm = None
            if self._trans is not None and (lda is not None or self.use_deltas):
                R = lda.shape[0] if lda is not None else 3 * dim   # the transform follows the LDA or the deltas
                ft = np.tile(np.eye(R, R + 1, dtype=np.float32), (len(ids), 1, 1))
                for s, i in ids.items():
                    if s in self._trans:
                        ft[i] = self._trans[s]
                fm = torch.from_numpy(ft).to(eng.device)
            fo = offsets([m.shape[0] for _, m in batch])
            d = torch.from_numpy(np.concatenate([m for _, m in batch]).astype(np.float32)).to(eng.device)
            if self.use_sliding_cmvn:
                d = eng.sliding_cmvn(d, fo, **SLIDING_CMVN_ARCHIVE)
            if self.use_splices and lda is None:
                raise NotImplementedError("spliced features without an LDA matrix")
            if not self.use_deltas and lda is None:
                out = d if cm is None else None
                if out is None:   # CMVN only (FinalFeatureFunction's output): Δ kernel's first block is the CMVN-applied base
                    out = eng.features(d, fo, u2s, cm)[:, :dim]
            else:
                out = eng.features(d, fo, u2s, cm, lda=lda, fmllr=fm, splice_context=self.splice_frames)
            if self._vad is not None or self.subsample_n > 1:      # last: voiced frames, then every n-th of them
                vad = None if self._vad is None else \
                    torch.from_numpy(np.concatenate([self._vad[k] for k, _ in batch]).astype(np.float32)).to(eng.device)
                out, fo = eng.select_frames(out.contiguous(), fo, vad, self.subsample_n)
            out = out.cpu().numpy()
            res = [(k, out[fo[i]: fo[i + 1]].copy()) for i, (k, _) in enumerate(batch)]
            batch.clear()
            return res

        for key, m in self._base():
            batch.append((key, m))
            if len(batch) >= self.batch_size:
                yield from flush()
        if batch:
            yield from flush()

    def close(self) -> None:
        self._cache.clear()


class AlignmentArchive:
    """``AlignmentArchive(ali, words_file_name=, likelihood_file_name=)``: iterable of Alignment and ``archive[utt_id]``
    (KeyError when absent) over the arks ``GmmAligner.export_alignments`` writes (MFA/alignment/multiprocessing.py:1856)."""

    def __init__(self, file_name, words_file_name=None, likelihood_file_name=None):
        self._ali = dict(kaldi_io.read_ark(Path(file_name).read_bytes(), "int_vector"))
        self._words = dict(kaldi_io.read_ark(Path(words_file_name).read_bytes(), "int_vector")) if words_file_name else {}
        self._likes = dict(kaldi_io.read_ark(Path(likelihood_file_name).read_bytes(), "vector")) if likelihood_file_name else {}

    def _make(self, key) -> "Alignment":
        pf = self._likes.get(key)
        like = float(np.sum(pf)) if pf is not None else float("nan")
        return Alignment(key, self._ali[key].tolist(), self._words.get(key, np.zeros(0, np.int32)).tolist(), like, pf)

    def __getitem__(self, key) -> "Alignment":
        if key not in self._ali:
            raise KeyError(key)
        return self._make(key)

    def __iter__(self):
        for key in self._ali:
            yield self._make(key)

    def close(self) -> None:
        pass


class Utterance:
    def __init__(self, segment: Segment, transcript: str, cmvn: Optional[np.ndarray] = None, fmllr: Optional[np.ndarray] = None):
        self.segment, self.transcript = segment, transcript
        self.cmvn, self.fmllr = cmvn, fmllr
        self.mfccs: Optional[np.ndarray] = None
        self._cmvn_applied: Optional[np.ndarray] = None

    def generate_mfccs(self, mfcc_computer: MfccComputer) -> None:
        self.mfccs = mfcc_computer.compute_mfccs(self.segment)

    def apply_cmvn(self, cmvn: np.ndarray) -> None:
        self.cmvn = np.asarray(cmvn, dtype=np.float64)

    def generate_features(self, mfcc_computer: MfccComputer, pitch_computer=None, lda_mat: Optional[np.ndarray] = None,
                          fmllr_trans: Optional[np.ndarray] = None, splice_context: int = 3) -> np.ndarray:
        """CMVN → (pitch pasted, when a ``pitch_computer`` is given) → Δ+ΔΔ, or splice+LDA when ``lda_mat`` is given, then
        fMLLR when there is a transform (MFA/alignment/multiprocessing.py:1287-1304).  The CMVN statistics are those of the
        MFCC columns; the pitch columns get zero sums, which the feature kernel's offset −(0 / count) leaves untouched."""
        import torch

        if self.mfccs is None:
            self.generate_mfccs(mfcc_computer)
        eng = get_engine()
        dev = eng.device
        base, cmvn = self.mfccs.astype(np.float32), self.cmvn
        if pitch_computer is not None:
            pitch = pitch_computer.compute_pitch_for_export(self.segment, compress=False)
            base = paste_feats([base, pitch], 1)
            if cmvn is not None:
                dim = self.mfccs.shape[1]
                cmvn = np.concatenate([cmvn[:, :dim], np.zeros((2, pitch.shape[1])), cmvn[:, dim:]], axis=1)
        frame_off = np.array([0, base.shape[0]], dtype=np.int64)
        d = torch.from_numpy(base).to(dev)
        cm = None if cmvn is None else torch.from_numpy(np.ascontiguousarray(cmvn)[None].copy()).to(dev)
        u2s = np.zeros(1, dtype=np.int32)
        lda = None if lda_mat is None else torch.from_numpy(np.asarray(lda_mat, dtype=np.float32)).to(dev)
        fm = fmllr_trans if fmllr_trans is not None else self.fmllr
        fm = None if fm is None else torch.from_numpy(np.asarray(fm, dtype=np.float32)[None].copy()).to(dev)
        return eng.features(d, frame_off, u2s, cm, lda=lda, fmllr=fm, splice_context=splice_context).cpu().numpy()


# ------------------------------------------------------------------------------------------------ lexicon / graphs
class LexiconCompiler(_LexiconCompiler):
    def phones_to_pronunciations(self, words, intervals, transcription: bool = False, text: Optional[str] = None):
        return _ctm.phones_to_pronunciations(self, words, intervals, transcription, text)


def _read_model(path_or_bytes) -> Tuple[_model.TransitionModel, _model.DiagGmmModel]:
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
    return _model.load_model_bytes(bytes(data))


def read_transition_model(path):
    return _read_model(path)[0]


def read_gmm_model(path):
    return _read_model(path)


class TrainingGraphCompiler(_graph.TrainingGraphCompiler):
    """``TrainingGraphCompiler(model_path, tree_path, lexicon_compiler, use_g2p=False, batch_size=…)``."""

    def __init__(self, model_path, tree_path, lexicon_compiler, use_g2p: bool = False, batch_size: int = 500):
        tm = model_path if isinstance(model_path, _model.TransitionModel) else _read_model(model_path)[0]
        tree = tree_path if isinstance(tree_path, kaldi_io.ContextDependency) else kaldi_io.read_tree(Path(tree_path).read_bytes())
        super().__init__(tm, tree, lexicon_compiler, use_g2p, batch_size)

    def export_graphs(self, file_name, records: Iterable[Tuple[str, str]], write_scp: bool = False, callback=None,
                      interjection_words=None) -> None:
        """Writes ``fsts.*.ark`` (key + OpenFst VectorFst<StdArc> binary per utterance).  ``records``:
        ``(key, text)`` pairs, or the utterance dicts CompileTrainGraphsFunction passes (``kaldi_id`` plus
        ``normalized_text`` / ``normalized_character_text`` with ``use_g2p``; MFA/alignment/multiprocessing.py:547-571).
        ``interjection_words`` belong to the transcript-verification workflow (``:512-536``; empty for alignment) and are
        refused when non-empty rather than ignored."""
        if interjection_words:
            raise NotImplementedError("interjection words (transcript verification) are not part of the alignment path")
        text_column = "normalized_character_text" if self.use_g2p else "normalized_text"
        with open(file_name, "wb") as f:
            chunk: List[Tuple[str, str]] = []

            def flush():
                for (key, _t), fst in zip(chunk, self.compile_fsts([t for _k, t in chunk])):   # native, batch_size at a time
                    kaldi_io.write_ark_entry(f, key, fst, "fst")
                    if callback:
                        callback(key)
                chunk.clear()

            for rec in records:
                chunk.append((rec["kaldi_id"], rec[text_column]) if isinstance(rec, dict) else tuple(rec))
                if len(chunk) >= max(1, int(self.batch_size)):
                    flush()
            flush()


class FstArchive:
    """``FstArchive(path)`` — the training-graph table ``fsts.*.ark`` AlignFunction opens (MFA/alignment/multiprocessing.py:
    828): iterable of ``(key, Fst)`` in file order, ``archive[key]`` for random access (KeyError when absent)."""

    def __init__(self, file_name):
        self.file_name = str(file_name)
        self._index: Optional[Dict[str, kaldi_io.Fst]] = None

    def __iter__(self):
        return kaldi_io.read_ark(Path(self.file_name).read_bytes(), "fst")

    def __getitem__(self, key: str) -> kaldi_io.Fst:
        if self._index is None:
            self._index = dict(iter(self))
        return self._index[key]

    def close(self) -> None:
        self._index = None


# ------------------------------------------------------------------------------------------------ alignment
@dataclass
class Alignment:
    utterance_id: Optional[str]
    alignment: List[int]
    words: List[int]
    likelihood: float
    per_frame_likelihoods: Optional[np.ndarray] = None
    status: int = 0                 # 0 aligned with the first beam, 1 with the retry beam (include/mfa_hip.h)

    def generate_ctm(self, transition_model, phone_table, frame_shift: float = 0.01):
        return _ctm.generate_ctm(self.alignment, transition_model, phone_table, frame_shift)


class GmmAligner:
    """``GmmAligner(model_path, beam=, retry_beam=, transition_scale=, acoustic_scale=, self_loop_scale=,
    disambiguation_symbols=)`` (MFA/alignment/multiprocessing.py:814; MFA/online/alignment.py:97-104)."""

    def __init__(self, acoustic_model_path, beam: float = 10, retry_beam: float = 40, transition_scale: float = 1.0,
                 acoustic_scale: float = 0.1, self_loop_scale: float = 0.1, disambiguation_symbols=None,
                 careful: bool = False):
        if careful:
            raise NotImplementedError("careful alignment is not implemented")
        # (AlignFunction._run tests `.endswith(".alimdl")` on it, MFA/alignment/multiprocessing.py:842)
        self.acoustic_model_path = acoustic_model_path if isinstance(acoustic_model_path, (bytes, bytearray)) else str(acoustic_model_path)
        self.transition_model, self.acoustic_model = _read_model(acoustic_model_path)
        self.beam, self.retry_beam = float(beam), float(retry_beam)
        if self.retry_beam != 0 and self.retry_beam <= self.beam:
            self.retry_beam = 4 * self.beam  # MFA/alignment/mixins.py:91-92
        self.transition_scale, self.acoustic_scale, self.self_loop_scale = transition_scale, acoustic_scale, self_loop_scale
        self.disambiguation_symbols = sorted(disambiguation_symbols or [])
        self._scaled = self.transition_model.scaled_log_probs(transition_scale, self_loop_scale)
        self._loaded = False

    def boost_silence(self, silence_weight: float, silence_phones: Sequence[int]) -> None:
        self.acoustic_model.boost_silence(silence_weight, _model.pdfs_of_phones(self.transition_model, silence_phones))
        self._loaded = False

    def _engine(self):
        eng = get_engine()
        if not self._loaded or eng.gmm is not self.acoustic_model:
            eng.load_gmm(self.acoustic_model)
            self._loaded = True
        return eng

    def align_utterances(self, fsts: Sequence[kaldi_io.Fst], feats: Sequence[np.ndarray], utterance_ids=None) -> List[Optional[Alignment]]:
        """Batched form of ``align_utterance``: one device launch per stage for the whole list."""
        import torch
        from .engine import redo_capacity

        eng = self._engine()
        general = [k for k, f in enumerate(fsts) if eng.needs_general_decoder(f)]
        if general and len(general) < len(fsts):       # mixed batch: the two decoders take their own utterances
            fast = [k for k in range(len(fsts)) if k not in set(general)]
            out: List[Optional[Alignment]] = [None] * len(fsts)
            for part in (fast, general):
                ids = [utterance_ids[k] for k in part] if utterance_ids else None
                for k, r in zip(part, self.align_utterances([fsts[k] for k in part], [feats[k] for k in part], ids)):
                    out[k] = r
            return out
        frame_off = offsets([x.shape[0] for x in feats])
        d_feats = torch.from_numpy(np.concatenate(feats).astype(np.float32)).to(eng.device)
        if general:
            # graphs with epsilon input arcs (kalpy-compiled fsts.*.ark) or very wide states: FasterDecoder as Kaldi runs
            # it, ProcessNonemitting included (mfa_align_general_batch)
            graphs = eng.pack_graphs_general([_graph.add_transition_probs(f, self._scaled) for f in fsts], self.transition_model)
            res = eng.align_general(graphs, d_feats, frame_off, beam=self.beam, retry_beam=self.retry_beam,
                                    acoustic_scale=self.acoustic_scale, want_frame_likes=True)
            res = {k: res[k].cpu().numpy() for k in self._RESULT_KEYS}
            return self._collect(res, frame_off, len(fsts), utterance_ids)
        scaled_fsts = [_graph.add_transition_probs(f, self._scaled) for f in fsts]
        graphs = eng.pack_graphs(scaled_fsts, self.transition_model)
        # features in, alignments out — the decodable is evaluated lazily, as Kaldi's is: per window of frames only the
        # pdfs that arcs near the live tokens can emit are scored (mfa_align_features_batch)
        res = eng.align_features(graphs, d_feats, frame_off, beam=self.beam, retry_beam=self.retry_beam,
                                 acoustic_scale=self.acoustic_scale, want_frame_likes=True)
        res = {k: res[k].cpu().numpy() for k in self._RESULT_KEYS}      # (not the score scratch: ΣT·P floats)
        # token / back-pointer capacity overflows (status 3 / 4) are decoded again, as in the corpus pipeline
        redo_capacity(eng, scaled_fsts, self.transition_model, d_feats, frame_off, res,
                      lambda g, f, fo, mt, bp: eng.align_features(g, f, fo, beam=self.beam, retry_beam=self.retry_beam,
                                                                  acoustic_scale=self.acoustic_scale, max_tokens=mt,
                                                                  bp_tokens_per_frame=bp, want_frame_likes=True),
                      self.beam, self.retry_beam, self.acoustic_scale)
        return self._collect(res, frame_off, len(fsts), utterance_ids)

    _RESULT_KEYS = ("ali", "words", "n_words", "like", "status", "frame_like")

    @staticmethod
    def _collect(res, frame_off, n, utterance_ids) -> List[Optional[Alignment]]:
        out: List[Optional[Alignment]] = []
        for u in range(n):
            st = int(res["status"][u])
            if st not in (0, 1):
                # the reference returns None and lets the caller count the failure (statuses beyond "no final token"
                # concern this utterance only, never the rest of the batch; they are logged with their code)
                if st != 2:
                    logger.warning("utterance %s: %s", utterance_ids[u] if utterance_ids else u, _lib.status_reason(st))
                out.append(None)
                continue
            a, b = int(frame_off[u]), int(frame_off[u + 1])
            nw = int(res["n_words"][u])
            out.append(Alignment(utterance_ids[u] if utterance_ids else None, res["ali"][a:b].tolist(),
                                 res["words"][a: a + nw].tolist(), float(res["like"][u]), res["frame_like"][a:b].copy(), st))
        return out

    def align_utterance(self, training_graph: kaldi_io.Fst, features: np.ndarray, utterance_id: Optional[str] = None):
        return self.align_utterances([training_graph], [features], [utterance_id])[0]

    def export_alignments(self, file_name, training_graph_archive, feature_archive, word_file_name=None,
                          likelihood_file_name=None, callback=None, batch_size: int = 256) -> None:
        """``training_graph_archive`` / ``feature_archive``: iterables of (key, Fst) / (key, matrix) with equal key order
        (kalpy: FstArchive, FeatureArchive).  Writes Kaldi int32-vector / float-vector arks keyed by utterance."""
        fa = open(file_name, "wb")
        fw = open(word_file_name, "wb") if word_file_name else None
        fl = open(likelihood_file_name, "wb") if likelihood_file_name else None
        try:
            feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
            batch: List[Tuple[str, kaldi_io.Fst]] = []

            def flush():
                if not batch:
                    return
                keys = [k for k, _ in batch]
                res = self.align_utterances([f for _, f in batch], [feats[k] for k in keys], keys)
                for key, al in zip(keys, res):
                    if al is not None:
                        kaldi_io.write_ark_entry(fa, key, np.asarray(al.alignment, dtype=np.int32), "int_vector")
                        if fw:
                            kaldi_io.write_ark_entry(fw, key, np.asarray(al.words, dtype=np.int32), "int_vector")
                        if fl:
                            kaldi_io.write_ark_entry(fl, key, al.per_frame_likelihoods.astype(np.float32), "vector")
                    if callback:
                        callback((key, al.likelihood if al is not None else None))
                batch.clear()

            for key, fst in training_graph_archive:
                if key not in feats:
                    continue
                batch.append((key, fst))
                if len(batch) >= batch_size:
                    flush()
            flush()
        finally:
            for f in (fa, fw, fl):
                if f:
                    f.close()


# ------------------------------------------------------------------------------------------------ statistics / adaptation
class AccumAmDiagGmm:
    """``_kalpy.gmm.AccumAmDiagGmm`` as MFA/alignment/adapting.py uses it: ``init(acoustic_model)``, ``Add(scale, other)``,
    ``TotLogLike()``, ``TotCount()``.  ``stats`` is the ``engine.GmmStats`` behind it (its transition-id counts are the
    accumulator's ``transition_accs``)."""

    def __init__(self):
        self.stats = None

    def init(self, acoustic_model, n_tids: int = 1) -> None:
        from .engine import GmmStats
        self.stats = GmmStats.zeros(acoustic_model.num_gauss, acoustic_model.dim, n_tids)

    def Add(self, scale: float, other: "AccumAmDiagGmm") -> None:
        if float(scale) != 1.0:
            raise NotImplementedError("AccumAmDiagGmm.Add: only scale 1.0")
        o = other.stats
        if self.stats.tid_count.shape != o.tid_count.shape:          # (init() does not know the transition model)
            self.stats.tid_count = np.zeros_like(o.tid_count)
        self.stats += o

    def TotLogLike(self) -> float:
        return float(self.stats.tot_like)

    def TotCount(self) -> float:
        return float(self.stats.tot_count)


def IsmoothStatsAmDiagGmmFromModel(acoustic_model, tau: float, gmm_accs: AccumAmDiagGmm) -> None:
    """In place, as the reference calls it (MFA/alignment/adapting.py:117)."""
    from . import adapt
    gmm_accs.stats = adapt.ismooth_from_model(adapt.raw_from_soa(acoustic_model), gmm_accs.stats, tau)


class GmmStatsAccumulator:
    """``kalpy.gmm.train.GmmStatsAccumulator(model_path)``: ``accumulate_stats(feature_archive, alignment_archive,
    callback=None)`` over (key, matrix) features and ``Alignment`` objects, then ``gmm_accs`` / ``transition_accs``
    (MFA/alignment/multiprocessing.py:40, :652-666).  Utterances are batched onto the device (``engine.gmm_statistics``)."""

    def __init__(self, acoustic_model_path, batch_frames: int = 500_000):
        self.acoustic_model_path = acoustic_model_path
        self.transition_model, self.acoustic_model = _read_model(acoustic_model_path)
        self.gmm_accs = AccumAmDiagGmm()
        self.gmm_accs.init(self.acoustic_model, self.transition_model.num_transition_ids + 1)
        self.batch_frames = int(batch_frames)

    @property
    def transition_accs(self) -> np.ndarray:
        """Counts per transition-id as float64 (kalpy: a DoubleVector), index 0 unused."""
        return self.gmm_accs.stats.tid_count.astype(np.float64)

    def accumulate_stats(self, feature_archive, alignment_archive, callback=None) -> None:
        import torch
        from .engine import gmm_statistics

        eng = get_engine()
        if eng.gmm is not self.acoustic_model:
            eng.load_gmm(self.acoustic_model)
        feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
        rows, alis, total = [], [], 0

        def flush():
            nonlocal rows, alis, total
            if rows:
                gmm_statistics(eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device),
                               torch.from_numpy(np.concatenate(alis).astype(np.int32)).to(eng.device), self.transition_model,
                               into=self.gmm_accs.stats)
            rows, alis, total = [], [], 0

        for al in alignment_archive:
            x = feats.get(al.utterance_id)
            if x is None:
                continue
            a = np.asarray(al.alignment, dtype=np.int32)
            if a.shape[0] != x.shape[0]:
                logger.warning("utterance %s: %d alignment entries for %d frames, skipped", al.utterance_id, a.shape[0], x.shape[0])
                continue
            rows.append(np.asarray(x)); alis.append(a); total += a.shape[0]
            if callback:
                callback(al.utterance_id)
            if total >= self.batch_frames:
                flush()
        flush()


class TwoFeatsStatsAccumulator(GmmStatsAccumulator):
    """The accumulation of the reference's SAT alignment model (``AccStatsTwoFeatsFunction``, MFA/acoustic_modeling/sat.py:46-130;
    Kaldi gmm-acc-stats-twofeats): ``accumulate_stats(feature_archive, si_feature_archive, alignment_archive, callback=None)``
    — posteriors from ``feature_archive`` (the speaker-adapted features), sums from ``si_feature_archive`` (the same frames,
    unadapted) —, then ``gmm_accs`` / ``transition_accs``.  Batching and the skip rule are ``GmmStatsAccumulator``'s; an
    utterance missing from either archive, or with different frame counts in the two, is skipped as well."""

    def accumulate_stats(self, feature_archive, si_feature_archive, alignment_archive, callback=None) -> None:
        import torch
        from .engine import gmm_statistics_twofeats

        eng = get_engine()
        if eng.gmm is not self.acoustic_model:
            eng.load_gmm(self.acoustic_model)
        feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
        si_feats = dict(si_feature_archive) if not isinstance(si_feature_archive, dict) else si_feature_archive
        rows, si_rows, alis, total = [], [], [], 0

        def flush():
            nonlocal rows, si_rows, alis, total
            if rows:
                gmm_statistics_twofeats(eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device),
                                        torch.from_numpy(np.concatenate(si_rows).astype(np.float32)).to(eng.device),
                                        torch.from_numpy(np.concatenate(alis).astype(np.int32)).to(eng.device), self.transition_model,
                                        into=self.gmm_accs.stats)
            rows, si_rows, alis, total = [], [], [], 0

        for al in alignment_archive:
            x, y = feats.get(al.utterance_id), si_feats.get(al.utterance_id)
            if x is None or y is None:
                continue
            a = np.asarray(al.alignment, dtype=np.int32)
            if a.shape[0] != x.shape[0] or np.shape(y) != np.shape(x):
                logger.warning("utterance %s: %d alignment entries for features %s and %s, skipped", al.utterance_id, a.shape[0],
                               np.shape(x), np.shape(y))
                continue
            rows.append(np.asarray(x)); si_rows.append(np.asarray(y)); alis.append(a); total += a.shape[0]
            if callback:
                callback(al.utterance_id)
            if total >= self.batch_frames:
                flush()
        flush()


# ------------------------------------------------------------------------------------------------ LDA
class LdaEstimateOptions:
    """``_kalpy.transform.LdaEstimateOptions``: ``dim`` 40, ``allow_large_dim`` False, ``remove_offset`` False."""

    def __init__(self, dim: int = 40, allow_large_dim: bool = False, remove_offset: bool = False):
        self.dim, self.allow_large_dim, self.remove_offset = int(dim), bool(allow_large_dim), bool(remove_offset)


class LdaEstimate:
    """``_kalpy.transform.LdaEstimate`` as MFA/acoustic_modeling/lda.py:340-351 uses it: ``Add(other)`` and
    ``estimate(options) -> (lda_mat, full_mat)``.  ``stats`` is the ``stats.LdaStats`` behind it (None until frames arrive)."""

    def __init__(self, stats=None):
        self.stats = stats

    def Add(self, other: "LdaEstimate") -> None:
        if other.stats is None:
            return
        if self.stats is None:
            self.stats = other.stats.copy()
        else:
            self.stats += other.stats

    def estimate(self, options: Optional[LdaEstimateOptions] = None):
        from .lda import estimate_lda
        if self.stats is None:
            raise ValueError("LdaEstimate.estimate: no statistics were accumulated")
        o = options or LdaEstimateOptions()
        return estimate_lda(self.stats, dim=o.dim, allow_large_dim=o.allow_large_dim, remove_offset=o.remove_offset)


class LdaStatsAccumulator:
    """``kalpy.feat.lda.LdaStatsAccumulator(model_path, silence_phones, rand_prune=…)``: ``accumulate_stats(feature_archive,
    alignment_archive, callback=None)`` then ``.lda`` (MFA/acoustic_modeling/lda.py:106-119).  The archive is the reference's
    ``FeatureArchive(feats, deltas=False, splices=True, splice_frames=…)``: it is not iterated (spliced rows are never made);
    the accumulator takes its base rows, CMVN table and splice width and the statistics kernel splices
    (``stats.lda_statistics``).  Classes are the model's pdfs, ``silence_phones`` weigh 0.  ``rand_prune`` defaults to the
    reference's 4.0; the draws are keyed by ``seed`` and the utterance's position in the alignment archive."""

    def __init__(self, acoustic_model_path, silence_phones: Sequence[int] = (), rand_prune: float = 4.0, seed: int = 0,
                 batch_frames: int = 500_000):
        self.acoustic_model_path = acoustic_model_path
        self.transition_model, self.acoustic_model = _read_model(acoustic_model_path)
        self.silence_phones, self.rand_prune, self.seed = list(silence_phones), float(rand_prune), int(seed)
        self.batch_frames = int(batch_frames)
        self.lda = LdaEstimate()

    def accumulate_stats(self, feature_archive, alignment_archive, callback=None) -> None:
        import torch
        from .stats import lda_statistics, silence_weights

        eng = get_engine()
        tm = self.transition_model
        weights = silence_weights(tm, self.silence_phones, 0.0)
        base = {key: (m, spk) for key, m, spk in feature_archive.base_rows()}
        ctx = int(feature_archive.splice_frames)
        rows, alis, spks, keys, total = [], [], [], [], 0

        def flush():
            nonlocal rows, alis, spks, keys, total
            if rows:
                ids = {s: i for i, s in enumerate(dict.fromkeys(spks))}
                u2s = np.array([ids[s] for s in spks], dtype=np.int32)
                st = feature_archive.cmvn_rows(ids, rows[0].shape[1])
                self.lda.stats = lda_statistics(
                    eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device), offsets([m.shape[0] for m in rows]),
                    u2s if st is not None else None, None if st is None else torch.from_numpy(st).to(eng.device),
                    torch.from_numpy(np.concatenate(alis).astype(np.int32)).to(eng.device), tm, splice_context=ctx, weights=weights,
                    rand_prune=self.rand_prune, utt_keys=np.asarray(keys, dtype=np.uint32), seed=self.seed, into=self.lda.stats)
            rows, alis, spks, keys, total = [], [], [], [], 0

        for position, al in enumerate(alignment_archive):
            got = base.get(al.utterance_id)
            if got is None:
                continue
            x, spk = got
            a = np.asarray(al.alignment, dtype=np.int32)
            if a.shape[0] != x.shape[0]:
                logger.warning("utterance %s: %d alignment entries for %d frames, skipped", al.utterance_id, a.shape[0], x.shape[0])
                continue
            rows.append(np.asarray(x)); alis.append(a); spks.append(spk); keys.append(position); total += a.shape[0]
            if callback:
                callback(al.utterance_id)
            if total >= self.batch_frames:
                flush()
        flush()


# ------------------------------------------------------------------------------------------------ MLLT
class MlltAccs:
    """``_kalpy.transform.MlltAccs`` as MFA/acoustic_modeling/lda.py:399-410 uses it: ``Add(other)`` and ``update() -> (mat,
    objf_impr, count)``.  ``stats`` is the ``stats.MlltStats`` behind it (None until frames arrive) — per-Gaussian full second
    moments, contracted with ``acoustic_model``'s inverse variances at ``update`` (``mllt.mllt_accs``)."""

    def __init__(self, acoustic_model=None, stats=None):
        self.acoustic_model, self.stats = acoustic_model, stats

    def Add(self, other: "MlltAccs") -> None:
        if other.stats is None:
            return
        if self.acoustic_model is None:
            self.acoustic_model = other.acoustic_model
        if self.stats is None:
            self.stats = other.stats.copy()
        else:
            self.stats += other.stats

    def update(self, num_sweeps: int = 200):
        from . import mllt
        if self.stats is None:
            raise ValueError("MlltAccs.update: no statistics were accumulated")
        mat, objf_impr, count, _trace = mllt.estimate_mllt(*mllt.mllt_accs(self.stats, self.acoustic_model), num_sweeps=num_sweeps)
        return mat, objf_impr, count


class MlltStatsAccumulator:
    """``kalpy.feat.lda.MlltStatsAccumulator(model_path, silence_phones, rand_prune=…)``: ``accumulate_stats(feature_archive,
    alignment_archive, callback=None)`` over (key, matrix) final features and ``Alignment`` objects, then ``.mllt_accs``
    (MFA/acoustic_modeling/lda.py:174-180).  Utterances are batched onto the device (``stats.mllt_statistics``), the
    accumulators stay there over the batches; ``silence_phones`` weigh 0.  ``rand_prune`` is accepted and ignored: the prune
    exists to make the reference's D³ accumulation per frame and Gaussian affordable, this formulation (per-Gaussian second
    moments, D² per pair) does not have that cost, and a nonzero value changes nothing."""

    def __init__(self, acoustic_model_path, silence_phones: Sequence[int] = (), rand_prune: float = 0.0, batch_frames: int = 500_000):
        self.acoustic_model_path = acoustic_model_path
        self.transition_model, self.acoustic_model = _read_model(acoustic_model_path)
        self.silence_phones, self.rand_prune = list(silence_phones), float(rand_prune)
        self.batch_frames = int(batch_frames)
        self.mllt_accs = MlltAccs(self.acoustic_model)

    def accumulate_stats(self, feature_archive, alignment_archive, callback=None) -> None:
        import torch
        from .stats import mllt_statistics, silence_weights

        eng = get_engine()
        if eng.gmm is not self.acoustic_model:
            eng.load_gmm(self.acoustic_model)
        tm = self.transition_model
        weights = silence_weights(tm, self.silence_phones, 0.0)
        feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
        rows, alis, total = [], [], 0

        def flush():
            nonlocal rows, alis, total
            if rows:
                self.mllt_accs.stats = mllt_statistics(
                    eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device),
                    torch.from_numpy(np.concatenate(alis).astype(np.int32)).to(eng.device), tm, weights, into=self.mllt_accs.stats)
            rows, alis, total = [], [], 0

        for al in alignment_archive:
            x = feats.get(al.utterance_id)
            if x is None:
                continue
            a = np.asarray(al.alignment, dtype=np.int32)
            if a.shape[0] != x.shape[0]:
                logger.warning("utterance %s: %d alignment entries for %d frames, skipped", al.utterance_id, a.shape[0], x.shape[0])
                continue
            rows.append(np.asarray(x)); alis.append(a); total += a.shape[0]
            if callback:
                callback(al.utterance_id)
            if total >= self.batch_frames:
                flush()
        flush()


def compose_transforms(a: np.ndarray, b: np.ndarray, b_is_affine: bool = False) -> np.ndarray:
    """``_kalpy.transform.compose_transforms(mat, prev, False)`` (MFA/acoustic_modeling/lda.py:420): ``mllt.compose_transforms``."""
    from . import mllt
    return mllt.compose_transforms(a, b, b_is_affine)


# ------------------------------------------------------------------------------------------------ flat-start training
def read_topology(path_or_bytes) -> kaldi_io.HmmTopology:
    """``kalpy.gmm.utils.read_topology``: a binary ``topo`` file."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
    r = kaldi_io.BinaryReader(bytes(data))
    r.expect_binary_header()
    return kaldi_io.read_topology(r)


def read_tree(path_or_bytes) -> kaldi_io.ContextDependency:
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else Path(path_or_bytes).read_bytes()
    return kaldi_io.read_tree(bytes(data))


def gmm_init_mono(topo, feats: Sequence[np.ndarray], shared_phones, model_path, tree_path) -> None:
    """``_kalpy.gmm.gmm_init_mono(topo, feats, shared_phones, model_path, tree_path)`` (MFA/acoustic_modeling/monophone.py:324):
    the flat-start model — one Gaussian per (phone set, pdf-class) at the global mean and variance of ``feats``, a list of
    feature matrices — and its tree, written to the two paths (``mle.init_mono``).  ``shared_phones``: lists of phone ids."""
    from . import adapt, mle

    feats = [np.asarray(x, dtype=np.float64) for x in feats if len(x)]
    if not feats:
        raise ValueError("gmm_init_mono: no features")
    raw_tm, raw_am, tree = mle.init_mono(topo, feats[0].shape[1], shared_phones)
    n = sum(x.shape[0] for x in feats)
    mean = sum(x.sum(axis=0) for x in feats) / n
    var = np.maximum(sum((x * x).sum(axis=0) for x in feats) / n - mean * mean, mle.MIN_VARIANCE)
    iv = (1.0 / var).astype(np.float32)[None]
    mi = mean.astype(np.float32)[None] * iv
    gc = adapt.gconsts(np.ones(1, np.float32), mi, iv)
    for p in range(raw_am.num_pdfs):
        raw_am.gconsts[p], raw_am.means_invvars[p], raw_am.inv_vars[p] = gc.copy(), mi.copy(), iv.copy()
    with open(model_path, "wb") as f:
        kaldi_io.write_model(f, raw_tm, raw_am)
    with open(tree_path, "wb") as f:
        kaldi_io.write_tree(f, tree)


def gmm_align_equal(fst: kaldi_io.Fst, feats: np.ndarray, seed: int = 0, key: int = 0):
    """``_kalpy.gmm.gmm_align_equal(decode_fst, feats)`` (MFA/acoustic_modeling/monophone.py:108): (alignment, words) of a
    random path with the frames spread evenly over its self-loops, on the device (mfa_align_equal_batch; the batch entry's
    result for utterance key ``key``), or (None, None) when the utterance cannot be aligned.  ``words``: the output labels
    along a path of the graph that spells the alignment."""
    from . import equal_align as _equal

    eng = get_engine()
    n_frames = int(np.asarray(feats).shape[0])
    ali, status = _equal.equal_align(eng, _equal.pack_bare(eng, [fst]), np.array([0, n_frames], dtype=np.int64), [key], seed)
    if int(status.cpu()[0]) != 0:
        return None, None
    ali = ali.cpu().numpy()
    return ali.tolist(), _equal.path_words(fst, ali)


# ------------------------------------------------------------------------------------------------ the triphone stage
class TreeStatsAccumulator:
    """``kalpy.gmm.train.TreeStatsAccumulator(model_path, context_independent_symbols=…)``: ``accumulate_stats(feature_archive,
    alignment_archive, callback=None)`` over (key, matrix) final features and ``Alignment`` objects, then ``.tree_stats``
    (MFA/acoustic_modeling/triphone.py:181-187) — a ``stats.TreeStats``, which adds (``+=``) as the reference's per-job
    dicts are merged.  Utterances are batched onto the device (``stats.tree_statistics``), the batches merged on the host in
    order.  ``skipped`` counts the utterances whose alignment does not split into phones."""

    def __init__(self, acoustic_model_path, context_independent_symbols: Sequence[int] = (), context_width: int = 3,
                 central_position: int = 1, batch_frames: int = 500_000):
        if (int(context_width), int(central_position)) != (3, 1):
            raise ValueError(f"TreeStatsAccumulator: context width {context_width} with central position {central_position}: only 3 and 1")
        self.acoustic_model_path = acoustic_model_path
        self.transition_model, self.acoustic_model = _read_model(acoustic_model_path)
        self.context_independent_symbols = [int(p) for p in context_independent_symbols]
        self.batch_frames = int(batch_frames)
        self.tree_stats = None
        self.skipped = 0

    def accumulate_stats(self, feature_archive, alignment_archive, callback=None) -> None:
        import torch
        from .stats import tree_statistics

        eng = get_engine()
        tm = self.transition_model
        feats = dict(feature_archive) if not isinstance(feature_archive, dict) else feature_archive
        rows, alis, total = [], [], 0

        def flush():
            nonlocal rows, alis, total
            if rows:
                fo = np.concatenate([[0], np.cumsum([a.shape[0] for a in alis])]).astype(np.int64)
                st, _frame_event, skipped = tree_statistics(
                    eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device), fo,
                    torch.from_numpy(np.concatenate(alis).astype(np.int32)).to(eng.device), tm, self.context_independent_symbols)
                self.skipped += skipped
                if self.tree_stats is None:
                    self.tree_stats = st
                else:
                    self.tree_stats += st
            rows, alis, total = [], [], 0

        for al in alignment_archive:
            x = feats.get(al.utterance_id)
            if x is None:
                continue
            a = np.asarray(al.alignment, dtype=np.int32)
            if a.shape[0] != x.shape[0]:
                logger.warning("utterance %s: %d alignment entries for %d frames, skipped", al.utterance_id, a.shape[0], x.shape[0])
                continue
            rows.append(np.asarray(x)); alis.append(a); total += a.shape[0]
            if callback:
                callback(al.utterance_id)
            if total >= self.batch_frames:
                flush()
        flush()


def automatically_obtain_questions(tree_stats, phone_sets, pdf_classes=(1,), position: int = 1):
    """``_kalpy.tree.automatically_obtain_questions(tree_stats, phone_sets, [1], 1)`` (MFA/acoustic_modeling/triphone.py:402):
    ``tree.automatic_questions`` — bottom-up clustering, not Kaldi's seeded top-down one."""
    from . import tree as _tree
    return _tree.automatic_questions(tree_stats, phone_sets, tuple(pdf_classes), int(position))


def read_roots(path) -> List[Tuple[List[int], bool, bool]]:
    """The reference's ``roots.int`` (MFA/dictionary/mixins.py:845-879): lines of ``shared|not-shared split|not-split`` and
    phone ids, as ``tree.build_tree`` takes them."""
    roots = []
    for line in Path(path).read_text().splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] not in ("shared", "not-shared") or len(f) < 3 or f[1] not in ("split", "not-split"):
            raise ValueError(f"roots file {path}: bad line {line!r}")
        roots.append(([int(p) for p in f[2:]], f[0] == "shared", f[1] == "split"))
    return roots


def build_tree(topo, questions, tree_stats, roots_path, tree_path, max_leaves: int = 1000, cluster_thresh: float = -1.0):
    """``_kalpy.tree.build_tree(topo, questions, tree_stats, roots_int_path, tree_path, max_leaves=, cluster_thresh=)``
    (MFA/acoustic_modeling/triphone.py:417): ``tree.build_tree`` on the roots file, the tree written to ``tree_path``.  Also
    returns the record of splits and merges."""
    from . import tree as _tree
    t, record = _tree.build_tree(topo, questions, tree_stats, read_roots(roots_path), max_leaves=int(max_leaves),
                                 cluster_thresh=float(cluster_thresh))
    with open(tree_path, "wb") as f:
        kaldi_io.write_tree(f, t)
    return record


def gmm_init_model(topo, tree, tree_stats, model_path, mixup: int = 0, mixdown: int = 0, var_floor: float = 0.01) -> None:
    """``_kalpy.gmm.gmm_init_model(topo, tree, tree_stats, model_path, mixup=, mixdown=)`` (MFA/acoustic_modeling/triphone.py:
    455): ``tree.init_model`` written to ``model_path``; with ``mixup`` above the number of leaves, ``mle.mix_up`` to that
    many Gaussians on the leaves' frame counts.  ``mixdown`` is not built."""
    from . import mle
    from . import tree as _tree

    if mixdown:
        raise NotImplementedError("gmm_init_model: mixdown is not built")
    raw_tm, raw_am = _tree.init_model(topo, tree, tree_stats, var_floor=var_floor)
    if mixup and int(mixup) > raw_am.num_pdfs:
        leaf = _tree.event_leaves(tree, tree_stats)
        occ = np.bincount(leaf[leaf >= 0], weights=tree_stats.count[leaf >= 0].astype(np.float64), minlength=raw_am.num_pdfs)
        raw_am, _targets = mle.mix_up(raw_am, occ, int(mixup))
    with open(model_path, "wb") as f:
        kaldi_io.write_model(f, raw_tm, raw_am)


def gmm_init_model_from_previous(*args, **kwargs):
    """``_kalpy.gmm.gmm_init_model_from_previous`` (two-level trees): not built."""
    raise NotImplementedError("gmm_init_model_from_previous is not built")


def convert_alignments(old_transition_model, new_transition_model, tree, alignment) -> List[int]:
    """``_kalpy.hmm.convert_alignments(old_transition_model, new_transition_model, tree, alignment)`` (MFA/acoustic_modeling/
    triphone.py:112): one utterance's transition-ids on the new model and tree — the same phones, states and arcs, the pdfs of
    the windows the alignment itself spells (``tree.convert_table`` over the host twin of the tree statistics).  Raises when
    the alignment does not split into phones."""
    from . import tree as _tree
    from .stats import tree_statistics_host

    a = np.asarray(alignment, dtype=np.int32)
    st, frame_event, skipped = tree_statistics_host(np.zeros((a.shape[0], 1), np.float32), np.array([0, a.shape[0]], dtype=np.int64),
                                                    a, old_transition_model, ())
    if skipped:
        raise ValueError("convert_alignments: the alignment does not split into phones")
    table = _tree.convert_table(old_transition_model, new_transition_model, tree, st)
    return _tree.convert_alignments(table, _tree.local_of_tid(old_transition_model), frame_event, a).tolist()


def write_gmm_model(path, transition_model, acoustic_model) -> None:
    """``kalpy.gmm.utils.write_gmm_model(path, transition_model, acoustic_model)`` for the objects ``read_gmm_model``
    returns (the mixture weights are the model's own when it was read from a file)."""
    from . import adapt
    raw_tm = kaldi_io.RawTransitionModel(transition_model.raw.topo, transition_model.raw.tuples,
                                         transition_model.log_probs.astype(np.float32))
    with open(path, "wb") as f:
        kaldi_io.write_model(f, raw_tm, adapt.raw_from_soa(acoustic_model))


HierarchicalCtm = _ctm.HierarchicalCtm
CtmInterval = _ctm.CtmInterval
WordCtmInterval = _ctm.WordCtmInterval


# ------------------------------------------------------------------------------------------------ diagonal UBM
class MleDiagGmmOptions:
    """``_kalpy.gmm.MleDiagGmmOptions``: Kaldi's defaults."""

    def __init__(self, min_gaussian_weight: float = 1.0e-5, min_gaussian_occupancy: float = 10.0, min_variance: float = 0.001,
                 remove_low_count_gaussians: bool = True):
        self.min_gaussian_weight, self.min_gaussian_occupancy = min_gaussian_weight, min_gaussian_occupancy
        self.min_variance, self.remove_low_count_gaussians = min_variance, remove_low_count_gaussians


class AccumDiagGmm:
    """``_kalpy.gmm.AccumDiagGmm`` as MFA/ivector/trainer.py:329-336 uses it: ``Resize(model, flags)``, ``Add(scale, other)``.
    ``stats`` is the one-pdf ``GmmStats`` behind it."""

    def __init__(self, stats=None):
        self.stats = stats

    def Resize(self, model: "DiagGmm", flags=None) -> None:
        from .stats import GmmStats
        self.stats = GmmStats.zeros(model.NumGauss(), model.Dim(), 1)

    def Add(self, scale: float, other: "AccumDiagGmm") -> None:
        if float(scale) != 1.0:
            raise NotImplementedError("AccumDiagGmm.Add: only scale 1.0")
        self.stats += other.stats


class DiagGmm:
    """kalpy's ``DiagGmm`` as the reference's UBM stage calls it (MFA/ivector/trainer.py:292-305, :330-346,
    MFA/ivector/multiprocessing.py:110-124): ``DiagGmm(num_gauss, dim)``, ``init_from_random_frames(feats)``,
    ``train_one_iter(feats, options, iteration, num_threads)``, ``Split(n, perturb_factor)``, ``NumGauss()``,
    ``gaussian_selection(feats, n)``, ``mle_update(accs, remove_low_count_gaussians=)``.  ``ubm`` is the ``ubm.DiagUbm``
    behind it; the E-steps run on the process's engine."""

    def __init__(self, num_gauss: int = 0, dim: int = 0, ubm=None, seed: int = 0):
        self.ubm = ubm
        self._num_gauss, self._dim = int(num_gauss), int(dim)
        self._rng = np.random.default_rng(seed)

    @classmethod
    def read(cls, path) -> "DiagGmm":
        from .ubm import DiagUbm
        return cls(ubm=DiagUbm.read(path))

    def write(self, path) -> None:
        self.ubm.write(path)

    def NumGauss(self) -> int:
        return self.ubm.num_gauss if self.ubm is not None else self._num_gauss

    def Dim(self) -> int:
        return self.ubm.dim if self.ubm is not None else self._dim

    def init_from_random_frames(self, feats) -> None:
        from . import ubm as _ubm
        self.ubm = _ubm.init_from_random_frames(np.asarray(feats), self._num_gauss, self._rng)

    def _device(self, feats):
        import torch
        eng = get_engine()
        return eng, torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).to(eng.device)

    def train_one_iter(self, feats, options: Optional[MleDiagGmmOptions] = None, iteration: int = 0, num_threads: int = 1) -> float:
        """One dense EM iteration on ``feats`` (gmm-global-init-from-feats' TrainOneIter).  Returns the average log-likelihood
        per frame under the model it started from."""
        from . import ubm as _ubm
        from .stats import ubm_statistics
        o = options or MleDiagGmmOptions()
        eng, x = self._device(feats)
        st = ubm_statistics(eng, x, self.ubm)
        self.ubm = _ubm.update(self.ubm, st, o.remove_low_count_gaussians, o.min_gaussian_weight,
                               min_gaussian_occupancy=o.min_gaussian_occupancy, min_variance=o.min_variance)[0]
        return st.loglike_per_frame

    def Split(self, target_components: int, perturb_factor: float = 0.1) -> None:
        from . import ubm as _ubm
        self.ubm = _ubm.split(self.ubm, int(target_components), perturb_factor, self._rng)

    def gaussian_selection(self, feats, num_gselect: int):
        """(per frame the list of its best Gaussians, best first; the frames' summed log-likelihood over them)."""
        from .stats import gaussian_selection
        eng, x = self._device(feats)
        gs, ll = gaussian_selection(eng, x, self.ubm, int(num_gselect))
        return gs.cpu().numpy().tolist(), float(ll.double().sum().item())

    def mle_update(self, gmm_accs: AccumDiagGmm, remove_low_count_gaussians: bool = True, min_gaussian_weight: float = 1.0e-4):
        from . import ubm as _ubm
        self.ubm, updated, removed, floored = _ubm.update(self.ubm, gmm_accs.stats, remove_low_count_gaussians, min_gaussian_weight)
        return updated, removed, floored


class GselectArchive:
    """``GselectArchive(path)``: iterable of (utt_id, list of per-frame lists) and ``archive[utt_id]`` over an
    Int32VectorVector ark (Kaldi gmm-gselect's output).  ``GselectArchive.write(path, entries)`` writes one."""

    def __init__(self, file_name):
        self.file_name = Path(file_name)
        self._table: Optional[Dict[str, List[np.ndarray]]] = None

    @staticmethod
    def write(file_name, entries) -> None:
        kaldi_io.write_table(file_name, ((k, [np.asarray(row, dtype=np.int32) for row in v]) for k, v in entries), "int_vector_vector")

    def _load(self) -> Dict[str, List[np.ndarray]]:
        if self._table is None:
            self._table = dict(kaldi_io.read_ark(self.file_name.read_bytes(), "int_vector_vector"))
        return self._table

    def __iter__(self):
        return ((k, [r.tolist() for r in v]) for k, v in self._load().items())

    def __getitem__(self, key: str):
        return [r.tolist() for r in self._load()[key]]

    def matrix(self, key: str) -> np.ndarray:
        """The utterance's lists as int32 [frames, n]; lists shorter than the longest are padded with −1 (no Gaussian)."""
        rows = self._load()[key]
        n = max((r.shape[0] for r in rows), default=0)
        out = np.full((len(rows), n), -1, dtype=np.int32)
        for i, r in enumerate(rows):
            out[i, : r.shape[0]] = r
        return out

    def __contains__(self, key) -> bool:
        return key in self._load()

    def close(self) -> None:
        self._table = None


class GlobalGmmStatsAccumulator:
    """``GlobalGmmStatsAccumulator(model_path)``: ``accumulate_stats(feature_archive, gselect_archive, callback=None)`` over
    (key, matrix) features and a ``GselectArchive``, then ``gmm_accs`` (MFA/ivector/multiprocessing.py:271-280; Kaldi
    gmm-global-acc-stats --gselect).  Utterances are batched onto the device (``stats.ubm_statistics``); one without a
    selection, or whose selection has another number of frames, is skipped with a warning."""

    def __init__(self, model_path, batch_frames: int = 500_000):
        self.model_path = model_path
        self.model = DiagGmm.read(model_path)
        self.gmm_accs = AccumDiagGmm()
        self.gmm_accs.Resize(self.model)
        self.batch_frames = int(batch_frames)

    def accumulate_stats(self, feature_archive, gselect_archive: GselectArchive, callback=None) -> None:
        import torch
        from .stats import ubm_statistics

        eng = get_engine()
        rows, sels, total = [], [], 0

        def flush():
            nonlocal rows, sels, total
            if rows:
                n = max(s.shape[1] for s in sels)
                sel = np.concatenate([np.pad(s, ((0, 0), (0, n - s.shape[1])), constant_values=-1) for s in sels])
                ubm_statistics(eng, torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(eng.device), self.model.ubm,
                               torch.from_numpy(sel).to(eng.device), into=self.gmm_accs.stats)
            rows, sels, total = [], [], 0

        for key, x in feature_archive:
            if key not in gselect_archive:
                logger.warning("No gselect information for utterance %s", key)
                continue
            g = gselect_archive.matrix(key)
            if g.shape[0] != x.shape[0]:
                logger.warning("utterance %s: gselect of %d frames for %d feature frames, skipped", key, g.shape[0], x.shape[0])
                continue
            rows.append(np.asarray(x)); sels.append(g); total += g.shape[0]
            if callback:
                callback(key)
            if total >= self.batch_frames:
                flush()
        flush()


# ---- i-vector extractor ------------------------------------------------------------------------------------------------------
def _generate_post(self, feats, num_post: int = 20, min_post: float = 0.025):
    """kalpy's ``DiagGmm.generate_post``: per frame the (Gaussian, posterior) pairs of its ``num_post`` best Gaussians after
    gauss-to-post's pruning at ``min_post`` (scale 1), in the selection's order (MFA/ivector/multiprocessing.py:166-173)."""
    from .stats import gaussian_selection, prune_posteriors, ubm_statistics
    eng, x = self._device(feats)
    gs, _ll = gaussian_selection(eng, x, self.ubm, int(num_post))
    _st, post = ubm_statistics(eng, x, self.ubm, gs, want_post=True)
    post = prune_posteriors(eng, post, float(min_post), 1.0, inplace=True)
    g, p = gs.cpu().numpy(), post.cpu().numpy()
    return [[(int(i), float(v)) for i, v in zip(gr, pr) if v != 0.0] for gr, pr in zip(g, p)]


DiagGmm.generate_post = _generate_post


def ScalePosterior(scale: float, post):
    """Kaldi's ScalePosterior: every posterior multiplied by ``scale`` in float32 (a new list; a scale of 0 empties the frames)."""
    s = np.float32(scale)
    if s == 0:
        return [[] for _ in post]
    return [[(int(i), float(np.float32(p) * s)) for i, p in frame] for frame in post]


def posterior_matrices(post, n: Optional[int] = None):
    """A Posterior as the device takes it: int32 indices and float32 posteriors [frames, n], short frames padded with (−1, 0)."""
    n = max((len(f) for f in post), default=0) if n is None else n
    n = max(n, 1)
    g = np.full((len(post), n), -1, dtype=np.int32)
    p = np.zeros((len(post), n), dtype=np.float32)
    for t, frame in enumerate(post):
        for j, (i, v) in enumerate(frame):
            g[t, j], p[t, j] = i, v
    return g, p


class PosteriorArchive:
    """``PosteriorArchive(path)``: (utt_id, Posterior) pairs and ``archive[utt_id]`` over a Posterior ark (``kaldi_io``'s
    "posterior" kind).  ``PosteriorArchive.write(path, entries)`` writes one."""

    def __init__(self, file_name):
        self.file_name = Path(file_name)
        self._table = None

    @staticmethod
    def write(file_name, entries) -> None:
        kaldi_io.write_table(file_name, entries, "posterior")

    def _load(self):
        if self._table is None:
            self._table = dict(kaldi_io.read_ark(self.file_name.read_bytes(), "posterior"))
        return self._table

    def __iter__(self):
        return iter(self._load().items())

    def __getitem__(self, key: str):
        return self._load()[key]

    def __contains__(self, key) -> bool:
        return key in self._load()


class IvectorExtractorStatsAccumulator:
    """``IvectorExtractorStatsAccumulator(ie_path)``: ``accumulate_stats(feature_archive, post_reader, callback=None)`` over
    (key, matrix) features and a mapping from key to Posterior (a ``PosteriorArchive`` or a dict), then ``ivector_stats``
    (MFA/ivector/multiprocessing.py:283-331; Kaldi ivector-extractor-acc-stats).  Utterances are batched onto the device
    (``stats.ivector_utterance_statistics``, ``stats.ivector_estep``); one without posteriors, or whose posteriors have another
    number of frames, is skipped with a warning."""

    def __init__(self, ie_path, batch_frames: int = 500_000):
        from .ivector import IvectorExtractorModel, IvectorStats
        self.ie_path = ie_path
        self.model = IvectorExtractorModel.read(ie_path)
        self.ivector_stats = IvectorStats.zeros(self.model.num_gauss, self.model.dim, self.model.ivector_dim)
        self.batch_frames = int(batch_frames)

    def accumulate_stats(self, feature_archive, post_reader, callback=None) -> None:
        import torch
        from .stats import ivector_estep, ivector_utterance_statistics

        eng = get_engine()
        rows, posts, total = [], [], 0

        def flush():
            nonlocal rows, posts, total
            if rows:
                n = max(max((len(f) for f in p), default=0) for p in posts)
                mats = [posterior_matrices(p, n) for p in posts]
                off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
                dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
                S = dev(self.ivector_stats.S)
                gamma, X, S = ivector_utterance_statistics(eng, dev(np.concatenate(rows).astype(np.float32)), off,
                                                           dev(np.concatenate([m[0] for m in mats])),
                                                           dev(np.concatenate([m[1] for m in mats])), self.model.num_gauss, S=S)
                ivector_estep(eng, self.model, gamma, X, into=self.ivector_stats)
                self.ivector_stats.S = S.cpu().numpy()
            rows, posts, total = [], [], 0

        for key, x in feature_archive:
            if key not in post_reader:
                logger.warning("No posteriors for utterance %s", key)
                continue
            post = post_reader[key]
            if len(post) != x.shape[0]:
                logger.warning("utterance %s: posteriors of %d frames for %d feature frames, skipped", key, len(post), x.shape[0])
                continue
            rows.append(np.asarray(x)); posts.append(post); total += x.shape[0]
            if callback:
                callback(key)
            if total >= self.batch_frames:
                flush()
        flush()


class IvectorExtractor:
    """``IvectorExtractor(dubm_path, ie_path, acoustic_weight=, max_count=, num_gselect=, min_post=)`` with
    ``extract_ivector(feats)`` and ``export_ivectors(ark_path, feature_archive, write_scp=, callback=)``, as
    ExtractIvectorsFunction drives kalpy's (MFA/corpus/features.py:956-1015; Kaldi ivector-extract): selection and softmax
    under the UBM, pruning with scale ``acoustic_weight``, the utterance statistics with ``max_count``, the E-step without
    accumulators.  The vector handed out is μ with ``prior_offset`` subtracted from element 0, float32; the ark is a
    float-vector table."""

    def __init__(self, dubm_path, ie_path, acoustic_weight: float = 1.0, max_count: float = 0.0, num_gselect: int = 20,
                 min_post: float = 0.025, batch_frames: int = 500_000):
        from .ivector import IvectorExtractorModel
        from .ubm import DiagUbm
        self.ubm = DiagUbm.read(dubm_path)
        self.model = IvectorExtractorModel.read(ie_path)
        if self.ubm.num_gauss != self.model.num_gauss or self.ubm.dim != self.model.dim:
            raise ValueError("IvectorExtractor: the UBM and the extractor do not fit together")
        self.acoustic_weight, self.max_count = float(acoustic_weight), float(max_count)
        self.num_gselect, self.min_post, self.batch_frames = int(num_gselect), float(min_post), int(batch_frames)

    def _extract(self, mats) -> np.ndarray:
        """i-vectors [utterances, R] of the feature matrices ``mats`` as one device batch."""
        import torch
        from .stats import gaussian_selection, ivector_estep, ivector_utterance_statistics, prune_posteriors, ubm_statistics
        eng = get_engine()
        off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(mats), dtype=np.float32)).to(eng.device)
        gs, _ll = gaussian_selection(eng, x, self.ubm, self.num_gselect)
        _st, post = ubm_statistics(eng, x, self.ubm, gs, want_post=True)
        post = prune_posteriors(eng, post, self.min_post, self.acoustic_weight, inplace=True)
        gamma, X, _ = ivector_utterance_statistics(eng, x, off, gs, post, self.ubm.num_gauss, max_count=self.max_count)
        mean = ivector_estep(eng, self.model, gamma, X)[0].cpu().numpy()
        mean[:, 0] -= self.model.prior_offset
        return mean.astype(np.float32)

    def extract_ivector(self, feats) -> np.ndarray:
        feats = np.asarray(feats)
        if feats.ndim != 2 or feats.shape[0] == 0:
            raise ValueError("extract_ivector: an utterance without frames")
        return self._extract([feats])[0]

    def export_ivectors(self, file_name, feature_archive, write_scp: bool = False, callback=None) -> None:
        entries, keys, mats, total = [], [], [], 0

        def flush():
            nonlocal keys, mats, total
            if mats:
                entries.extend(zip(keys, self._extract(mats)))
            keys, mats, total = [], [], 0

        for key, x in feature_archive:
            x = np.asarray(x)
            if x.shape[0] == 0:
                logger.warning("utterance %s has no frames, skipped", key)
                continue
            keys.append(key); mats.append(x); total += x.shape[0]
            if callback:
                callback(key)
            if total >= self.batch_frames:
                flush()
        flush()
        file_name = Path(file_name)
        kaldi_io.write_table(file_name, entries, "vector", file_name.with_suffix(".scp") if write_scp else None)


# ------------------------------------------------------------------------------------------------ PLDA (kalpy.ivector)
def ivector_normalize_length(ivector) -> np.ndarray:
    """``_kalpy.ivector.ivector_normalize_length``: the vector (or every row) scaled to norm √D.  kalpy's works in place on a
    Kaldi vector; a numpy array given here is changed in place too, and returned."""
    from .plda import normalize_length
    out = normalize_length(ivector)
    if isinstance(ivector, np.ndarray) and ivector.dtype == np.float64:
        ivector[...] = out
        return ivector
    return out


def ivector_subtract_mean(ivectors) -> np.ndarray:
    """``_kalpy.ivector.ivector_subtract_mean``: the vectors with their mean taken off, as rows [n, D].  A list of numpy
    vectors is also updated in place, as kalpy updates its list of Kaldi vectors."""
    from .plda import subtract_mean
    out = subtract_mean(np.stack([np.asarray(v, dtype=np.float64) for v in ivectors]))
    if isinstance(ivectors, list):
        for v, row in zip(ivectors, out):
            if isinstance(v, np.ndarray) and v.dtype == np.float64:
                v[...] = row
    return out


class Plda:
    """kalpy's ``Plda`` as the reference uses it (MFA/corpus/ivector_corpus.py:316-452, MFA/diarization/multiprocessing.py):
    ``transform_ivector``, ``log_likelihood`` and the distances built on it, one pair at a time on the host — and the batched
    forms that replace the reference's per-pair Python calls (``pairwise``, ``log_likelihood_distance_vectorized``) on the
    device.  ``distance`` is defined here as −LLR (kalpy's own mapping of the ratio to a distance is not among this project's
    references: INTEGRATION.md)."""

    def __init__(self, model=None):
        self.model = model

    @classmethod
    def read(cls, path) -> "Plda":
        from .plda import PldaModel
        return cls(PldaModel.read(path))

    def write(self, path, binary: bool = True) -> None:
        self.model.write(path, binary)

    def Dim(self) -> int:
        return self.model.dim

    def transform_ivector(self, ivector, num_examples: int = 1, normalize_length: bool = True, simple_length_norm: bool = False):
        return self.model.transform_ivector(np.asarray(ivector, dtype=np.float64), num_examples, normalize_length, simple_length_norm)

    def transform_ivectors(self, ivectors, num_examples=None, normalize_length: bool = True, simple_length_norm: bool = False) -> np.ndarray:
        """Rows [n, D] on the device (``stats.plda_transform``); numpy out."""
        from .stats import plda_transform
        return plda_transform(get_engine(), self.model, ivectors, num_examples, normalize_length, simple_length_norm).cpu().numpy()

    def log_likelihood(self, train_ivector, num_train_examples: int, test_ivector) -> float:
        """The log-likelihood ratio of one pair of transformed vectors, on the host: the direct form, the specification."""
        return float(self.model.log_likelihood_ratio(train_ivector, num_train_examples, test_ivector))

    def distance(self, train_ivector, test_ivector, num_train_examples: int = 1) -> float:
        return -self.log_likelihood(train_ivector, num_train_examples, test_ivector)

    def log_likelihood_distance_vectorized(self, train_ivectors, test_ivector, num_train_examples=None) -> np.ndarray:
        """One test vector against every train vector: −LLR [n_train], on the device."""
        return -self.pairwise(np.atleast_2d(test_ivector), train_ivectors, num_train_examples)[0]

    def pairwise(self, test_ivectors, train_ivectors=None, num_train_examples=None) -> np.ndarray:
        """The matrix [test, train] of log-likelihood ratios on the device (``stats.plda_scores``): what the reference builds
        through ``pairwise_distances(metric=plda.log_likelihood)``.  ``train_ivectors`` None: the test vectors themselves."""
        from .stats import plda_scores
        train = test_ivectors if train_ivectors is None else train_ivectors
        return plda_scores(get_engine(), self.model, test_ivectors, train, num_train_examples)

    def nearest(self, test_ivectors, k: int, train_ivectors=None, num_train_examples=None):
        """The k best train vectors of every test vector (indices, LLRs), no matrix stored (``stats.plda_knn``): what the
        reference's ``NearestNeighbors(metric=<callable>)`` is asked for.  ``train_ivectors`` None: the test vectors, each
        without itself."""
        from .stats import plda_knn
        same = train_ivectors is None
        idx, score = plda_knn(get_engine(), self.model, test_ivectors, test_ivectors if same else train_ivectors, k, num_train_examples,
                              exclude_diagonal=same)
        return idx.cpu().numpy(), score.cpu().numpy()


class PldaStats:
    """kalpy's ``PldaStats``: ``AddSamples(weight, group)``, ``Sort()``, ``Dim()``."""

    def __init__(self):
        from .plda import PldaStats as _Stats
        self.stats = _Stats()

    def AddSamples(self, weight: float, group) -> None:
        self.stats.add_samples(float(weight), np.asarray(group, dtype=np.float64))

    def Sort(self) -> None:
        self.stats.sort()

    def Dim(self) -> int:
        return self.stats.dim


@dataclass
class PldaEstimationConfig:
    num_em_iters: int = 10


class PldaEstimator:
    """``PldaEstimator(stats).Estimate(config, plda)`` fills ``plda`` (a ``Plda``), as compute_plda calls it
    (MFA/corpus/ivector_corpus.py:277-281)."""

    def __init__(self, stats: PldaStats):
        self.stats = stats

    def Estimate(self, config: PldaEstimationConfig, plda: Plda) -> None:
        from .plda import estimate_plda
        plda.model = estimate_plda(self.stats.stats, config.num_em_iters)


@dataclass
class PldaUnsupervisedAdaptorConfig:
    mean_diff_scale: float = 1.0
    within_covar_scale: float = 0.3
    between_covar_scale: float = 0.7


class PldaUnsupervisedAdaptor:
    """``AddStats(weight, ivector)`` then ``UpdatePlda(config, plda)``, which changes ``plda`` in place, as adapt_plda calls
    them (MFA/corpus/ivector_corpus.py:123-139)."""

    def __init__(self):
        self._vectors: List[Tuple[float, np.ndarray]] = []

    def AddStats(self, weight: float, ivector) -> None:
        self._vectors.append((float(weight), np.array(ivector, dtype=np.float64)))

    def UpdatePlda(self, config: PldaUnsupervisedAdaptorConfig, plda: Plda) -> None:
        from .plda import PldaUnsupervisedAdaptor as _Adaptor
        ad = _Adaptor(config.mean_diff_scale, config.within_covar_scale, config.between_covar_scale)
        for w, v in self._vectors:
            ad.add_stats(w, v)
        plda.model = ad.update_plda(plda.model)


class PldaScorer:
    """``PldaScorer(plda_path)`` as PldaClassificationFunction uses kalpy's (MFA/diarization/multiprocessing.py):
    ``load_speaker_ivectors`` prepares the speakers as ``collect_speaker_ivectors`` does (length norm, subtract mean, length
    norm, the transform with each speaker's utterance count); ``classify_speaker`` returns (speaker index, LLR) of one
    utterance vector, ``classify_speakers`` of a batch, both through the device's fused best-column sweep.  ``backend="host"``
    runs the same chain on the host twins (tests)."""

    def __init__(self, plda_path, backend: str = "device"):
        self.plda = plda_path if isinstance(plda_path, Plda) else Plda.read(plda_path)
        self.backend = backend
        self.speaker_ids: List[str] = []
        self.speaker_ivectors: Optional[np.ndarray] = None      # transformed, [speakers, D]
        self.num_speaker_examples: Optional[np.ndarray] = None

    def _transform(self, x, n=None) -> np.ndarray:
        from . import stats as _stats
        if self.backend == "host":
            return _stats.plda_transform_host(self.plda.model, x, n)
        return _stats.plda_transform(get_engine(), self.plda.model, x, n).cpu().numpy()

    def load_speaker_ivectors(self, train_ivector_path, num_utts_path=None) -> None:
        """``train_ivector_path``: a vector ark of per-speaker mean i-vectors, or (key, vector) pairs; ``num_utts_path``: the text
        file "speaker count" per line, or a mapping; missing: 1 each."""
        from .plda import normalize_length, subtract_mean
        if isinstance(train_ivector_path, (str, Path)):
            entries = list(kaldi_io.read_ark(Path(train_ivector_path).read_bytes(), "vector"))
        else:
            entries = list(train_ivector_path)
        if isinstance(num_utts_path, (str, Path)):
            counts = {a: int(b) for a, b in (line.split() for line in Path(num_utts_path).read_text().splitlines() if line.strip())}
        else:
            counts = dict(num_utts_path or {})
        self.speaker_ids = [str(k) for k, _ in entries]
        x = np.stack([np.asarray(v, dtype=np.float64) for _, v in entries])
        x = normalize_length(subtract_mean(normalize_length(x)))
        self.num_speaker_examples = np.array([counts.get(k, 1) for k in self.speaker_ids], dtype=np.int32)
        self.speaker_ivectors = self._transform(x, self.num_speaker_examples)

    def classify_speakers(self, ivectors, transformed: bool = False):
        """(speaker index int32 [n], LLR float64 [n]) of utterance vectors [n, D]; not yet in the model's space unless
        ``transformed``.  −1 for a vector without a finite score."""
        from . import stats as _stats
        if self.speaker_ivectors is None:
            raise RuntimeError("PldaScorer: load_speaker_ivectors first")
        x = np.atleast_2d(np.asarray(ivectors, dtype=np.float64))
        if not transformed:
            x = self._transform(x)
        if self.backend == "host":
            return _stats.plda_classify_host(self.plda.model, x, self.speaker_ivectors, self.num_speaker_examples)
        idx, score = _stats.plda_classify(get_engine(), self.plda.model, x, self.speaker_ivectors, self.num_speaker_examples)
        return idx.cpu().numpy(), score.cpu().numpy()

    def classify_speaker(self, ivector, transformed: bool = False):
        idx, score = self.classify_speakers(np.atleast_2d(ivector), transformed)
        return int(idx[0]), float(score[0])


# ------------------------------------------------------------------------------------------------ speaker clustering
from .cluster import ClusterType, DistanceMetric  # noqa: E402  (the reference's montreal_forced_aligner.data enums)


def cluster_matrix(ivectors: np.ndarray, cluster_type: ClusterType, metric: DistanceMetric = DistanceMetric.euclidean, strict=True,
                   no_visuals=False, working_directory=None, **kwargs) -> np.ndarray:
    """The reference's ``cluster_matrix`` (MFA/diarization/multiprocessing.py) under its signature, on the process's engine:
    ``kwargs`` carry ``distance_threshold``, ``plda`` (a ``Plda``) and ``min_cluster_size`` as there.  ``ClusterType.dbscan`` only
    (``cluster.cluster_matrix``); nothing is drawn, so ``no_visuals`` and ``working_directory`` are accepted and unused."""
    from . import cluster as _cluster
    known = {k: kwargs.pop(k) for k in ("distance_threshold", "plda", "min_cluster_size", "backend") if k in kwargs}
    if kwargs:
        raise TypeError(f"cluster_matrix: unexpected keyword arguments {sorted(kwargs)}")
    backend = known.get("backend", "device")
    return _cluster.cluster_matrix(ivectors, cluster_type, metric, strict=strict, engine=get_engine() if backend == "device" else None, **known)


def hdbscan_matrix(ivectors: np.ndarray, metric: DistanceMetric = DistanceMetric.cosine, strict=True, no_visuals=False,
                   working_directory=None, **kwargs) -> np.ndarray:
    """The ``ClusterType.hdbscan`` branch of the reference's ``cluster_matrix`` on the process's engine (``cluster.hdbscan_matrix``):
    ``kwargs`` carry ``distance_threshold``, ``plda``, ``min_cluster_size`` and ``min_samples``.  ``cluster_matrix`` itself still
    refuses ``ClusterType.hdbscan``; nothing is drawn."""
    from . import cluster as _cluster
    known = {k: kwargs.pop(k) for k in ("distance_threshold", "plda", "min_cluster_size", "min_samples", "backend") if k in kwargs}
    if kwargs:
        raise TypeError(f"hdbscan_matrix: unexpected keyword arguments {sorted(kwargs)}")
    backend = known.get("backend", "device")
    return _cluster.hdbscan_matrix(ivectors, metric, strict=strict, engine=get_engine() if backend == "device" else None, **known)


def cluster_vectors(ivectors: np.ndarray, cluster_type: ClusterType, metric: DistanceMetric = DistanceMetric.cosine, strict=True,
                    no_visuals=False, working_directory=None, **kwargs):
    """The reference's ``cluster_matrix`` to its end on the process's engine (``cluster.cluster_vectors``): (labels, the silhouette
    score it logs), for ``ClusterType.dbscan`` and ``ClusterType.hdbscan``.  ``kwargs`` carry ``distance_threshold``, ``plda``,
    ``min_cluster_size`` and, for hdbscan, ``min_samples``; nothing is drawn."""
    from . import cluster as _cluster
    known = {k: kwargs.pop(k) for k in ("distance_threshold", "plda", "min_cluster_size", "min_samples", "backend") if k in kwargs}
    if kwargs:
        raise TypeError(f"cluster_vectors: unexpected keyword arguments {sorted(kwargs)}")
    backend = known.get("backend", "device")
    return _cluster.cluster_vectors(ivectors, cluster_type, metric, strict=strict, engine=get_engine() if backend == "device" else None, **known)


def silhouette_samples(X: np.ndarray, labels, metric="euclidean", plda=None, noise: str = "cluster", backend: str = "device") -> np.ndarray:
    """``sklearn.metrics.silhouette_samples(X, labels, metric=metric)`` on the process's engine (``cluster.silhouette_samples``);
    ``metric="plda"`` with ``plda=`` takes the place of the reference's callable ``plda.distance``."""
    from . import cluster as _cluster
    return _cluster.silhouette_samples(X, labels, metric, plda, noise, backend, get_engine() if backend == "device" else None)


def silhouette_score(X: np.ndarray, labels, metric="euclidean", plda=None, noise: str = "cluster", backend: str = "device") -> float:
    """``sklearn.metrics.silhouette_score(X, labels, metric=metric)`` (MFA/diarization/multiprocessing.py:452) on the process's engine."""
    from . import cluster as _cluster
    return _cluster.silhouette_score(X, labels, metric, plda, noise, backend, get_engine() if backend == "device" else None)
