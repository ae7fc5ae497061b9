"""Corpus-level driver: the fan-out / fan-in of ``AlignMixin.align_utterances`` (MFA/alignment/mixins.py:282-380) and the
two-pass flow of ``CorpusAligner.align`` (MFA/alignment/base.py:510-539) over the device pipeline, ending in the interval
and TextGrid layer (MFA/alignment/multiprocessing.py:1733-1751, MFA/textgrid.py:463-572).

The reference fans utterances out to worker processes that each walk Kaldi table files one utterance at a time; here a
rank takes the speakers ``sharding.assign_speakers`` gives it, cuts its utterances into length-bucketed ragged batches and
pushes each batch through MFCC → CMVN → features → scores → Viterbi entirely in HBM.  Per-speaker CMVN needs every
utterance of a speaker, so statistics are accumulated over the whole shard first (a cheap pass: MFCC + statistics
kernels), exactly like ``calc_cmvn`` runs before alignment in the reference.

A failed utterance yields ``None`` and is counted, never raised (MFA/alignment/mixins.py:308-314); the reason is kept in
``CorpusAligner.failure_reasons``.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ctm as _ctm
from . import _lib
from . import fmllr as _fmllr
from . import graph as _graph
from . import sharding
from . import adapt as _adapt
from . import kaldi_io
from .engine import AlignmentEngine, GmmStats, fmllr_statistics, gmm_statistics, gmm_statistics_twofeats, redo_capacity
from .model import DiagGmmModel, TransitionModel
from .stats import LdaStats, MlltStats, TreeStats, lda_statistics, mllt_statistics, silence_weights, tree_statistics
from .staging import StagingRing


@dataclass
class CorpusUtterance:
    utt_id: str
    speaker: str
    pcm: np.ndarray                 # int16 mono at ``sample_rate``
    text: str
    begin: float = 0.0              # position inside its sound file (for TextGrid export)
    file_name: Optional[str] = None
    file_duration: Optional[float] = None
    sample_rate: Optional[int] = None   # Hz of ``pcm``; None: the model's rate.  Other rates are converted on the device


class UtteranceResult:
    """One aligned utterance.  ``alignment`` / ``words`` are views of the batch arrays the device handed back; ``ctm`` — the
    ``HierarchicalCtm`` of MFA/alignment/multiprocessing.py:1733-1751 — is built from the batch's interval arrays the first
    time it is asked for (``CorpusAligner.export_textgrids`` writes files from the arrays and never asks)."""

    __slots__ = ("utt_id", "speaker", "alignment", "words", "likelihood", "num_frames", "_ctm", "_lazy")

    def __init__(self, utt_id: str, speaker: str, alignment: np.ndarray, words: np.ndarray, likelihood: float, num_frames: int,
                 ctm: Optional[_ctm.HierarchicalCtm] = None):
        self.utt_id, self.speaker, self.alignment, self.words = utt_id, speaker, alignment, words
        self.likelihood, self.num_frames = likelihood, num_frames          # total; MFA reports likelihood / num_frames
        self._ctm = ctm
        self._lazy = None            # (IntervalBatch, index, text, begin, end) until the objects are wanted

    @property
    def per_frame_likelihood(self) -> float:
        return self.likelihood / max(1, self.num_frames)

    @property
    def ctm(self) -> Optional[_ctm.HierarchicalCtm]:
        if self._ctm is None and self._lazy is not None:
            batch, k, text, begin, end = self._lazy
            self._ctm = batch.ctm(k, text=text, begin=begin, end=end, likelihood=self.per_frame_likelihood)
            self._lazy = None
        return self._ctm

    @ctm.setter
    def ctm(self, value) -> None:
        self._ctm, self._lazy = value, None

    @property
    def has_intervals(self) -> bool:
        return self._ctm is not None or self._lazy is not None

    def __getstate__(self):          # (rank-to-rank gather: the objects travel, not the batch arrays they would be built from)
        return (self.utt_id, self.speaker, np.array(self.alignment), np.array(self.words), self.likelihood, self.num_frames, self.ctm)

    def __setstate__(self, st):
        self.utt_id, self.speaker, self.alignment, self.words, self.likelihood, self.num_frames, self._ctm = st
        self._lazy = None


@dataclass
class AlignOptions:
    beam: float = 10.0
    retry_beam: float = 40.0
    transition_scale: float = 1.0
    acoustic_scale: float = 0.1
    self_loop_scale: float = 0.1
    boost_silence: float = 1.0
    max_tokens: int = 1024
    bp_tokens_per_frame: int = 256
    batch_frames: int = 2_000_000   # frames per device batch (≈ 2 000 ten-second utterances)
    fmllr_min_count: float = 500.0
    silence_weight: float = 0.0
    # `mfa align` (the corpus path) stores raw MFCCs and the CMVN-applied features as 8-bit Kaldi CompressedMatrix tables
    # (MFA/corpus/features.py:235, :356-365) and therefore aligns features quantised twice; `align_one` / the online path
    # keep float32 (the default here).  True reproduces the corpus path's two quantisations (device codec).
    corpus_compression: bool = False
    # raw MFCCs of a run stay on the device between the CMVN pass and the alignment passes up to this many bytes
    mfcc_cache_bytes: int = 64 << 30


class _BatchOut:
    """What the device handed back for one batch, on the host: ragged arrays in the device layout (utterance k of the batch
    at frame_off[k]; its word ids packed at the same offset)."""

    __slots__ = ("idx", "frame_off", "ali", "words", "n_words", "like", "status", "intervals")

    def __init__(self, idx, frame_off, ali, words, n_words, like, status):
        self.idx, self.frame_off, self.ali, self.words = list(idx), np.asarray(frame_off, dtype=np.int64), ali, words
        self.n_words, self.like, self.status = n_words, like, status
        self.intervals = None          # intervals_native.IntervalBatch once extracted


class CorpusAligner:
    """``CorpusAligner(tm, am, tree, lexicon, lda=None, ali_am=None)`` then ``align(utterances)`` / ``export_textgrids(...)``.

    ``ali_am``: the speaker-independent alignment model of a SAT acoustic model (``final.alimdl``).  When given, the first
    pass runs on it (MFA/alignment/mixins.py:404-410), fMLLR statistics take their posteriors from it and their means and
    variances from ``am`` (MFA/corpus/features.py:503-511), the second pass runs on ``am`` with the transforms, and an
    utterance that fails the second pass keeps its first-pass alignment (MFA/alignment/multiprocessing.py:841-863,
    :1784-1860)."""

    def __init__(self, tm: TransitionModel, am: DiagGmmModel, tree, lexicon, lda: Optional[np.ndarray] = None,
                 options: Optional[AlignOptions] = None, device: int = 0, engine: Optional[AlignmentEngine] = None,
                 mfcc_options: Optional[dict] = None, silence_phones: Sequence[int] = (),
                 ali_am: Optional[DiagGmmModel] = None, lazy: bool = True, pitch_options: Optional[dict] = None,
                 raw_tm: Optional[kaldi_io.RawTransitionModel] = None, raw_am: Optional[kaldi_io.RawAmDiagGmm] = None,
                 raw_ali_am: Optional[kaldi_io.RawAmDiagGmm] = None):
        self.tm, self.tree, self.lexicon = tm, tree, lexicon
        # the models as their files hold them (kaldi_io.read_model): what ``adapt`` updates and ``write_adapted`` writes
        self.raw_tm, self.raw_am, self.raw_ali_am = raw_tm, raw_am, raw_ali_am
        self.adapted: Optional[tuple] = None             # (raw tm, raw am, raw ali_am | None) of the last ``adapt``
        self.adapt_stats: Optional[GmmStats] = None      # its statistics on ``am`` (``adapt_ali_stats``: on ``ali_am``)
        self.adapt_ali_stats: Optional[GmmStats] = None
        self.adapt_loglike: Dict[str, Optional[float]] = {}   # average log-likelihood per frame the reference logs, per model
        self.adapt_counts: Dict[str, tuple] = {}         # Gaussians (updated, kept) per model
        self.lda_stats: Optional[LdaStats] = None        # the statistics of the last ``estimate_lda``
        self.mllt_stats: Optional[MlltStats] = None      # the statistics of the last ``estimate_mllt``
        self.alimdl_stats: Optional[GmmStats] = None     # the statistics of the last ``estimate_alignment_model``
        self.tree_stats: Optional[TreeStats] = None      # the statistics of the last ``tree_statistics``
        self.tree_skipped = 0                            # ... and the utterances it skipped
        self.pronunciation_counts = None                 # pronprob.PronunciationCounts of the last ``pronunciation_statistics``
        self.lda = None if lda is None else np.asarray(lda, dtype=np.float32)
        self.opt = options or AlignOptions()
        self.engine = engine or AlignmentEngine(device)
        self.mfcc_options = dict(mfcc_options or {})
        self.engine.configure_mfcc(**self.mfcc_options)
        # a use_pitch / use_voicing model (model.pitch_options(meta)): pitch columns are pasted after the MFCCs' CMVN in every
        # pass (MFA/alignment/multiprocessing.py:1290-1294).  None: no pitch, the path below is the one without this keyword.
        self.pitch_options = None if pitch_options is None else {k: v for k, v in pitch_options.items() if v is not None}
        self.n_pitch = 0
        if self.pitch_options is not None:
            if float(self.pitch_options.get("sample_frequency", 16000.0)) != self._model_rate():
                raise ValueError("pitch_options and mfcc_options must name the same sample_frequency: pitch runs on the PCM at the model's rate")
            self.engine.configure_pitch(**self.pitch_options)        # (add_delta_pitch and bad f0 bounds are refused here)
            self.n_pitch = self.engine.num_pitch_cols
        self.silence_phones = list(silence_phones)
        self.lazy = bool(lazy)
        # boost_silence scales the weights of the silence pdfs (GmmAligner.boost_silence, MFA/alignment/multiprocessing.py:
        # 803-815) of whichever model a pass aligns with — on COPIES: the caller's models are left as they were
        self.am = self._boosted(am)
        self.ali_am = None if ali_am is None else self._boosted(ali_am)
        if self.ali_am is not None and not np.array_equal(self.ali_am.pdf_offsets, self.am.pdf_offsets):
            raise ValueError("final.alimdl and final.mdl must have the same Gaussians per pdf")
        self._loaded = None
        self._load(self.am)
        self.compiler = _graph.TrainingGraphCompiler(tm, tree, lexicon)
        self.scaled = tm.scaled_log_probs(self.opt.transition_scale, self.opt.self_loop_scale)
        self.frame_shift = float(self.mfcc_options.get("frame_shift_ms", 10.0)) / 1000.0
        self.failed: List[str] = []
        self.failure_reasons: Dict[str, str] = {}
        self.fallback_first_pass: List[str] = []
        self.ctm_failed: List[str] = []          # aligned, but the interval stage raised (alignment kept, ctm None)
        self.transforms: Optional[np.ndarray] = None
        # speakers whose fMLLR estimate was dropped for degenerate statistics (a muted channel: constant features); they keep
        # the transform they came with (identity, or their previous one)
        self.fmllr_rejected: List[str] = []
        self._mfcc_cache: Dict[tuple, tuple] = {}
        self._mfcc_cache_bytes = 0
        self._mfcc_cache_on = False
        self._intervals = None          # intervals_native.IntervalExtractor, built on first use
        self._worker = None             # one worker thread: the next batch's graphs compile under the current batch
        self._graph_pools = StagingRing(self.engine.device, 3)   # staging the batches' graphs compile into (this pipeline's alone)
        self._out_pools = StagingRing(self.engine.device, 3)     # pinned staging for the batches' outputs on their way back

    def _boosted(self, am: DiagGmmModel) -> DiagGmmModel:
        import copy

        if self.opt.boost_silence == 1.0 or not self.silence_phones:
            return am
        from .model import pdfs_of_phones
        am2 = copy.copy(am)
        am2.gconsts = np.array(am.gconsts, dtype=np.float32, copy=True)
        am2.boost_silence(self.opt.boost_silence, pdfs_of_phones(self.tm, self.silence_phones))
        return am2

    def _load(self, am: DiagGmmModel) -> None:
        if self._loaded is not am:
            self.engine.load_gmm(am)
            self._loaded = am

    # ------------------------------------------------------------------ helpers
    def _model_rate(self) -> float:
        return float(self.mfcc_options.get("sample_frequency", 16000.0))

    def _rates(self, utts: Sequence[CorpusUtterance]) -> Optional[List[int]]:
        """Per-utterance sample rates when some utterance is not at the model's rate, else None (nothing to convert)."""
        model = self._model_rate()
        if all(getattr(u, "sample_rate", None) is None or u.sample_rate == model for u in utts):
            return None
        return [int(model) if getattr(u, "sample_rate", None) is None else int(u.sample_rate) for u in utts]

    def audio_seconds(self, u: CorpusUtterance) -> float:
        """Duration of an utterance's audio, by its own rate."""
        rate = getattr(u, "sample_rate", None)
        return len(u.pcm) / (self._model_rate() if rate is None else float(rate))

    def _batches(self, utts: Sequence[CorpusUtterance]) -> List[List[int]]:
        """Length-bucketed batches (BASELINE configs[4]): sort by duration, cut at ``batch_frames``.  Computed once per run
        (``align`` asks three times: graph compilation ahead, the CMVN pass, the alignment passes)."""
        lens = np.fromiter((len(u.pcm) for u in utts), dtype=np.int64, count=len(utts))
        rates = self._rates(utts)
        # (keyed on what the batches are a function of: not the list's identity, which a refilled or a new list can share)
        key = (int(self.opt.batch_frames), lens.tobytes(), None if rates is None else np.asarray(rates, dtype=np.int64).tobytes())
        if getattr(self, "_batches_key", None) == key:
            return self._batches_val
        if rates is not None:          # frames are counted from the lengths the resampler will hand the MFCC
            lens = self.engine.num_resampled_array(lens, rates)
        order = np.argsort(lens, kind="stable")
        frames = self.engine.num_frames_array(lens) if hasattr(self.engine, "num_frames_array") else \
            np.array([self.engine.num_frames(int(n)) for n in lens], dtype=np.int64)
        out, cur, total = [], [], 0
        for i, t in zip(order.tolist(), frames[order].tolist()):
            if cur and total + t > self.opt.batch_frames:
                out.append(cur)
                cur, total = [], 0
            cur.append(i)
            total += t
        if cur:
            out.append(cur)
        self._batches_key, self._batches_val = key, out
        return out

    def _mfcc(self, utts: Sequence[CorpusUtterance], idx: Sequence[int]):
        key = (id(utts), tuple(idx))          # (the list object of the run in progress; the cache only lives inside align())
        hit = self._mfcc_cache.get(key) if self._mfcc_cache_on else None
        if hit is not None:          # the CMVN pass computed them already (and a second alignment pass asks a third time)
            return hit
        # PCM gathered by host threads straight into pinned staging memory, then one asynchronous H2D copy (mfa_gather_pcm)
        pcm, so = self.engine.gather_pcm([utts[i].pcm for i in idx])
        rates = self._rates([utts[i] for i in idx])
        if rates is not None:          # native-rate PCM travels; the conversion to the model's rate runs on the device
            pcm, so = self.engine.resample(pcm, so, rates)
        if self.n_pitch:                     # the base matrix: MFCC columns, then the pitch columns (same rows: the paste rule)
            mfcc, fo = self.engine.base_features(pcm, so)
        else:
            mfcc, fo = self.engine.mfcc(pcm, so)
        if self.opt.corpus_compression:      # feats.*.ark of MfccFunction: compute_mfccs_for_export(seg, compress=True)
            nc = self.engine.num_ceps
            if not self.n_pitch:
                mfcc = self.engine.compress_round_trip(mfcc, fo)
            else:                            # two tables: the MFCCs', and compute_pitch_for_export(seg, compress=True)'s
                once = self.engine.compress_round_trip(mfcc, fo, cols=(0, nc))
                mfcc = self.engine.compress_round_trip(mfcc, fo, cols=(nc, nc + self.n_pitch), out=once)
        size = mfcc.numel() * mfcc.element_size()
        if self._mfcc_cache_on and self._mfcc_cache_bytes + size <= self.opt.mfcc_cache_bytes:   # 52 KB per 10 s utterance: HBM holds millions
            self._mfcc_cache[key] = (mfcc, fo)
            self._mfcc_cache_bytes += size
        return mfcc, fo

    def _final_features(self, mfcc, fo, rows, cmvn, d_lda, fmllr):
        """CMVN → Δ+ΔΔ | splice+LDA(+fMLLR).  With ``corpus_compression`` the CMVN-applied MFCCs take the second trip
        through the 8-bit codec first (FinalFeatureFunction, MFA/corpus/features.py:323-365), on the device; pitch columns,
        pasted after CMVN, have been through the codec once (``_mfcc``) and stay as they are."""
        eng = self.engine
        if not self.opt.corpus_compression:
            return eng.features(mfcc, fo, rows, cmvn, lda=d_lda, fmllr=fmllr)
        # ApplyCmvn (no variance normalisation) fused into the codec launch; with pitch the statistics are zero-padded to
        # the base matrix's width and only the MFCC columns make the trip
        dim = mfcc.shape[1] - self.n_pitch
        twice = eng.compress_round_trip(mfcc, fo, cols=(0, dim), cmvn=cmvn, utt2spk=rows)
        return eng.features(twice, fo, rows, None, lda=d_lda, fmllr=fmllr)

    def speaker_cmvn(self, utts: Sequence[CorpusUtterance]) -> Tuple[Dict[str, int], "object"]:
        """calc_cmvn: float64 [n_spk, 2, dim+1] on the device, and the speaker → row map.  With pitch the statistics are
        those of the MFCC columns alone, zero-padded in the pitch columns (the feature kernel then leaves those untouched)."""
        spk_ids = {s: k for k, s in enumerate(dict.fromkeys(u.speaker for u in utts))}
        # per-batch statistics come from the device kernel (float64, fixed order); batches are added up on the host, in
        # batch order — a few hundred bytes per speaker, and no framework arithmetic on the path
        total = np.zeros((len(spk_ids), 2, self.engine.num_ceps + 1), dtype=np.float64)
        pending = []
        for idx in self._batches(utts):
            mfcc, fo = self._mfcc(utts, idx)
            rows = np.array([spk_ids[utts[i].speaker] for i in idx], dtype=np.int32)
            local, inv = np.unique(rows, return_inverse=True)
            if self.n_pitch:
                mfcc = mfcc[:, : self.engine.num_ceps].contiguous()
            pending.append((local, self.engine.cmvn_stats(mfcc, fo, inv.astype(np.int32), len(local))))
        # read back after the last batch is queued: the next batch's PCM is gathered while this one's copy is on the bus
        for local, st in pending:
            total[local] += st.cpu().numpy()
        stats = torch.from_numpy(total).to(self.engine.device)
        return spk_ids, (self.engine.pad_cmvn_stats(stats, self.n_pitch) if self.n_pitch else stats)

    def _decode(self, graphs, feats, fo, max_tokens, bp_tokens):
        """One device call: scores evaluated lazily for the cells live tokens can reach (default), or the dense matrix."""
        eng, o = self.engine, self.opt
        if self.lazy:
            return eng.align_features(graphs, feats, fo, beam=o.beam, retry_beam=o.retry_beam, acoustic_scale=o.acoustic_scale,
                                      max_tokens=max_tokens, bp_tokens_per_frame=bp_tokens)
        ll, ll_off, ll_cols = eng.score(feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts,
                                        pdf_first_frame=graphs.pdf_first_frame)
        return eng.align(graphs, ll, ll_off, ll_cols, fo, beam=o.beam, retry_beam=o.retry_beam, acoustic_scale=o.acoustic_scale,
                         max_tokens=max_tokens, bp_tokens_per_frame=bp_tokens)

    # ------------------------------------------------------------------ one alignment pass, batch by batch
    def _compile(self, utts, idx_all, pool):
        """Pure host work of a batch, safe on a worker thread (no device call): transcripts → training graphs by the native
        compiler's threads, straight into the batch's pinned staging buffers.  Runs for batch b + 1 while the main thread packs,
        launches and collects batch b (and, for the first batch, while the CMVN pass gathers PCM)."""
        fsts_all = self.compiler.compile_fsts([utts[i].text for i in idx_all], self.scaled, columns=True, alloc=pool.get)
        return dict(idx_all=list(idx_all), fsts_all=fsts_all, pool=pool)

    def _next_graph_pool(self):
        """The staging pool the next batch's graphs compile into: round robin over three sets that nothing but the pipeline
        draws from — batch b + 1 compiles while batch b is launched from its pool and batch b - 1 is still collected from
        its own (the capacity redo packs its graphs again).  The engine's ``next_staging``, which every other packing call
        takes from, cannot move this turn.  Waits until the copies last started from the pool are done (main thread)."""
        return self._graph_pools.next()

    def _submit_compile(self, utts, idx_all):
        from concurrent.futures import ThreadPoolExecutor

        if self._worker is None:
            self._worker = ThreadPoolExecutor(1, thread_name_prefix="mfa-graphs")
        pool = self._next_graph_pool()
        return self._worker.submit(self._compile, utts, idx_all, pool)

    def _prepare(self, utts, comp):
        """Device layout + score plan of a compiled batch (main thread: starts the batch's H2D copies)."""
        eng = self.engine
        idx_all, fsts_all, pool = comp["idx_all"], comp["fsts_all"], comp["pool"]
        prep = dict(idx_all=idx_all, idx=[], fsts=[], gidx=[], gfsts=[], graphs=None)
        if getattr(fsts_all, "arc_pdf", None) is not None and len(fsts_all) and getattr(fsts_all, "max_degree", None) is not None \
                and fsts_all.min_ilabel > 0 and fsts_all.max_degree <= 64 and fsts_all.min_arcs > 0:
            # a batch straight from the native compiler with nothing for the general decoder in it: taken as it is
            prep["idx"], prep["fsts"] = list(idx_all), fsts_all
        else:
            for i, f in zip(idx_all, fsts_all):
                if f.num_arcs == 0 or f.num_states == 0 or np.any(f.arcs["ilabel"] < 0):
                    self.failure_reasons[utts[i].utt_id] = "empty or malformed training graph"   # this utterance only
                elif eng.needs_general_decoder(f):    # epsilon input arcs / a state with more than 64 arcs
                    prep["gidx"].append(i); prep["gfsts"].append(f)
                else:
                    prep["idx"].append(i); prep["fsts"].append(f)
        if prep["idx"]:
            prep["graphs"] = eng.pack_graphs(prep["fsts"], self.tm, pool=pool if prep["fsts"] is fsts_all else None)
        return prep

    def _launch(self, utts, prep, spk_ids, cmvn, d_lda, fmllr):
        """Device side of a batch: features and the alignment call for the utterances the wavefront-parallel decoder takes —
        enqueued, not waited for."""
        if not prep["idx"]:
            return None
        feats, fo, rows = self._batch_features(utts, prep["idx"], spk_ids, cmvn, d_lda, fmllr)
        res = self._decode(prep["graphs"], feats, fo, self.opt.max_tokens, self.opt.bp_tokens_per_frame)
        # outputs start their way back right behind the kernels (asynchronous copies into pinned staging memory, one event):
        # _collect waits for THIS batch only, while the next batch's kernels are already queued behind it.  (No copy to
        # the device starts from these pools, so the ring's wait has nothing to wait for: a set is free once _collect has
        # copied its views out, which happens right after the next batch's launch.)
        pool = self._out_pools.next()
        host = {}
        with torch.cuda.device(self.engine.device):
            for k in ("status", "ali", "words", "n_words", "like"):
                t = res[k]
                view = pool.get("out_" + k, t.numel(), {torch.int32: np.int32, torch.float32: np.float32}[t.dtype])
                torch.from_numpy(view).copy_(t, non_blocking=True)
                host[k] = view
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.engine.device))
        return dict(res=res, feats=feats, fo=fo, rows=rows, host=host, event=ev)

    def _general(self, utts, prep, spk_ids, cmvn, d_lda, fmllr, results, kept, want_feats):
        """FasterDecoder as Kaldi runs it, ProcessNonemitting included (mfa_align_general_batch): the slow, exact path for
        graphs with epsilon input arcs or very wide states."""
        eng, o = self.engine, self.opt
        gidx, gfsts = prep["gidx"], prep["gfsts"]
        feats, fo, rows = self._batch_features(utts, gidx, spk_ids, cmvn, d_lda, fmllr)
        gg = eng.pack_graphs_general(gfsts, self.tm)
        rg = eng.align_general(gg, feats, fo, beam=o.beam, retry_beam=o.retry_beam, acoustic_scale=o.acoustic_scale,
                               bp_tokens_per_frame=max(o.bp_tokens_per_frame, 512))
        out = _BatchOut(gidx, fo, rg["ali"].cpu().numpy(), rg["words"].cpu().numpy(), rg["n_words"].cpu().numpy(),
                        rg["like"].cpu().numpy(), rg["status"].cpu().numpy())
        for k, i in enumerate(gidx):
            if out.status[k] in (0, 1):
                results[i] = (out, k)
            else:
                self.failure_reasons[utts[i].utt_id] = _lib.status_reason(out.status[k])
        if want_feats:
            kept.append((gidx, feats, self._zero_failed(rg["ali"], fo, out.status), fo, rows))

    def _batch_features(self, utts, idx, spk_ids, cmvn, d_lda, fmllr):
        """(final features, frame offsets, speaker rows) of the utterances ``idx`` of a batch."""
        mfcc, fo = self._mfcc(utts, idx)
        rows = np.array([spk_ids[utts[i].speaker] for i in idx], dtype=np.int32)
        return self._final_features(mfcc, fo, rows, cmvn, d_lda, fmllr), fo, rows

    @staticmethod
    def _zero_failed(ali_dev, fo, status):
        """A batch's alignments on the device with the frames of failed utterances zeroed (in a copy): they must not vote in
        the statistics made from them."""
        bad = np.flatnonzero((status != 0) & (status != 1)).tolist()
        if bad:
            ali_dev = ali_dev.clone()
            for k in bad:
                ali_dev[int(fo[k]): int(fo[k + 1])] = 0
        return ali_dev

    def _collect(self, utts, prep, launched, results, kept, want_feats):
        """Results of a launched batch back on the host (this is where the host waits for the device)."""
        eng, o = self.engine, self.opt
        idx, fsts = prep["idx"], prep["fsts"]
        res, feats, fo, rows = launched["res"], launched["feats"], launched["fo"], launched["rows"]
        launched["event"].synchronize()
        # (pinned staging views: copied out here, before the ring of output pools comes round to their set again)
        host = {k: v.copy() for k, v in launched["host"].items()}
        status, ali = host["status"], host["ali"]
        # capacity overflows (status 3 tokens / 4 back-pointers) are decoded again: the merged alignments replace the
        # device's copy when the fMLLR pass will read it
        if redo_capacity(eng, fsts, self.tm, feats, fo, host, self._decode, o.beam, o.retry_beam, o.acoustic_scale) and want_feats:
            res["ali"] = torch.from_numpy(ali).to(eng.device)
        out = _BatchOut(idx, fo, ali, host["words"], host["n_words"], host["like"], status)
        ok = (status == 0) | (status == 1)
        for k in np.flatnonzero(ok).tolist():
            results[idx[k]] = (out, k)
        for k in np.flatnonzero(~ok).tolist():
            if status[k] == 2:
                self.failure_reasons.setdefault(utts[idx[k]].utt_id, _lib.status_reason(2))
            else:
                self.failure_reasons[utts[idx[k]].utt_id] = _lib.status_reason(status[k])
        if want_feats:
            kept.append((idx, feats, self._zero_failed(res["ali"], fo, status), fo, rows))

    def _pass(self, utts, spk_ids, cmvn, fmllr, want_feats=False, first_compile=None):
        """One alignment pass over all batches.  Returns per utterance ``(batch output, index)`` (None where alignment
        failed) and, when asked, what fMLLR estimation needs (features, alignments, frame offsets per batch).  Nothing an
        individual utterance does aborts the pass: unsupported graphs and decoder statuses beyond "failed" are recorded in
        ``failure_reasons`` (the reference logs and continues, MFA/alignment/mixins.py:308-314).

        Software pipeline over batches: the graphs of batch b + 1 compile on a worker thread while the main thread packs,
        launches and collects batch b.  ``first_compile``: the future of batch 0's compilation when the caller started it
        earlier (``_align`` does, under the CMVN pass)."""
        eng = self.engine
        d_lda = None if self.lda is None else torch.from_numpy(self.lda).to(eng.device)
        results: List[Optional[tuple]] = [None] * len(utts)
        kept: List[tuple] = []
        batches = self._batches(utts)
        fut = first_compile if first_compile is not None else (self._submit_compile(utts, batches[0]) if batches else None)
        in_flight = None                      # (prep, launched) of the batch the device is working on
        for b in range(len(batches)):
            comp = fut.result()
            # the next batch's graphs compile on the worker thread from here on — under this batch's packing and launch and
            # the previous batch's collection (its staging pool was last read two batches ago)
            fut = self._submit_compile(utts, batches[b + 1]) if b + 1 < len(batches) else None
            prep = self._prepare(utts, comp)
            launched = self._launch(utts, prep, spk_ids, cmvn, d_lda, fmllr)
            if in_flight is not None:         # collected while the device runs the batch launched just now
                self._collect(utts, in_flight[0], in_flight[1], results, kept, want_feats)
                in_flight = None
            if prep["gidx"]:
                self._general(utts, prep, spk_ids, cmvn, d_lda, fmllr, results, kept, want_feats)
            if launched is not None:
                in_flight = (prep, launched)
        if in_flight is not None:
            self._collect(utts, in_flight[0], in_flight[1], results, kept, want_feats)
        return results, kept

    # ------------------------------------------------------------------ public
    def align(self, utterances: Sequence[CorpusUtterance], speaker_adapted: bool = False, make_ctm: bool = True,
              previous_transforms: Optional[np.ndarray] = None) -> List[Optional[UtteranceResult]]:
        """The reference's flow (MFA/alignment/base.py:510-539): first pass on speaker-independent features — with the
        alignment model when the acoustic model ships one —; with ``speaker_adapted`` (a SAT model, ``uses_speaker_adaptation``
        in MFA) per-speaker fMLLR is estimated from it and a second pass is run with the transforms on ``am``.
        ``previous_transforms`` [n_spk, D, D+1] (speaker rows in first-appearance order): transforms the features already
        carry in the first pass; the new estimate is composed onto them (CalcFmllrFunction's previous_transform_archive)."""
        with self._run():
            return self._align(list(utterances), speaker_adapted, make_ctm, previous_transforms)[0]

    @contextmanager
    def _run(self):
        """The state of one run of ``align`` / ``adapt``: empty failure lists on entry; the cache of raw MFCCs (and of the
        batches) lives inside it and is dropped on the way out, however the run ends."""
        self.failed, self.failure_reasons, self.fallback_first_pass, self.ctm_failed = [], {}, [], []
        self.fmllr_rejected = []
        self._mfcc_cache, self._mfcc_cache_bytes, self._mfcc_cache_on = {}, 0, True
        try:
            yield
        finally:
            self._mfcc_cache, self._mfcc_cache_bytes, self._mfcc_cache_on = {}, 0, False
            self._batches_key = None

    def _align(self, utts, speaker_adapted, make_ctm, previous_transforms, keep_last=False):
        """Returns (results, kept): ``kept`` — with ``keep_last`` — is what the LAST pass left on the device per batch,
        (utterance indices, final features, alignments with failed utterances zeroed, frame offsets, speaker rows)."""
        batches = self._batches(utts)
        first_compile = self._submit_compile(utts, batches[0]) if batches else None     # graphs compile under the CMVN pass
        spk_ids, cmvn = self.speaker_cmvn(utts)
        first_model = self.ali_am if self.ali_am is not None else self.am
        self._load(first_model)
        prev = None if previous_transforms is None else torch.from_numpy(np.asarray(previous_transforms, dtype=np.float32)).to(self.engine.device)
        results, kept = self._pass(utts, spk_ids, cmvn, prev, want_feats=speaker_adapted or keep_last, first_compile=first_compile)
        self.transforms = None if previous_transforms is None else np.asarray(previous_transforms, dtype=np.float32)
        if speaker_adapted:
            # the transform follows either feature branch: the LDA's rows, or Δ+ΔΔ of the cepstra (MFA/db.py:2101-2136)
            D = self.lda.shape[0] if self.lda is not None else 3 * (self.engine.num_ceps + self.n_pitch)
            beta = np.zeros(len(spk_ids)); K = np.zeros((len(spk_ids), D, D + 1)); G = np.zeros((len(spk_ids), D, D + 1, D + 1))
            two_model = self.am if self.ali_am is not None else None
            for idx, feats, ali, fo, rows in kept:
                ids, b, k, g = fmllr_statistics(self.engine, feats, fo, ali, self.tm, rows, self.silence_phones,
                                                self.opt.silence_weight, stats_model=two_model)
                beta[ids] += b; K[ids] += k; G[ids] += g
            W = np.tile(np.eye(D, D + 1, dtype=np.float32), (len(spk_ids), 1, 1))
            names = {row: name for name, row in spk_ids.items()}
            for s in range(len(spk_ids)):
                W[s], _impr, why = _fmllr.estimate_fmllr(beta[s], K[s], G[s], min_count=self.opt.fmllr_min_count)
                if why == _fmllr.DEGENERATE:
                    self.fmllr_rejected.append(names[s])
                if previous_transforms is not None:
                    W[s] = _fmllr.compose_transforms(W[s], previous_transforms[s])
            self.transforms = W
            self._load(self.am)
            first = results
            self.failure_reasons = {}
            results, kept = self._pass(utts, spk_ids, cmvn, torch.from_numpy(W).to(self.engine.device), want_feats=keep_last)
            if self.ali_am is not None:
                # an utterance the second pass lost keeps its first-pass (alignment-model) result:
                # ali_first_pass / words_first_pass / likelihoods_first_pass, MFA/alignment/multiprocessing.py:1784-1860
                for i, (r2, r1) in enumerate(zip(results, first)):
                    if r2 is None and r1 is not None:
                        results[i] = r1
                        self.fallback_first_pass.append(utts[i].utt_id)
                        self.failure_reasons.pop(utts[i].utt_id, None)
        return self._results(utts, results, make_ctm), (kept if keep_last else [])

    # ------------------------------------------------------------------ model adaptation
    def adapt(self, utterances: Sequence[CorpusUtterance], speaker_adapted: bool = False, mapping_tau: float = 20.0,
              update_transitions: bool = True, make_ctm: bool = True) -> List[Optional[UtteranceResult]]:
        """``mfa adapt`` (MFA/alignment/adapting.py): align the corpus as ``align`` does, accumulate GMM statistics from the
        alignments of the last pass on the device (``engine.gmm_statistics``), smooth them towards the old model with
        ``mapping_tau`` frames, re-estimate the means and — with ``update_transitions`` — the transition probabilities, and
        load the new model.  Returns the results of the alignment (made with the OLD model).

        Statistics are formed with the model as its file holds it (``raw_am``, no silence boost: the reference reads
        ``unadapted.mdl`` from disk), on the final features of the last pass — with ``speaker_adapted`` the fMLLR-transformed
        ones.  With ``speaker_adapted`` and an ``ali_am`` the alignment model is adapted from the SAME features and
        alignments: the reference's AccStatsFunction builds its feature archive with Job.construct_feature_archive
        (MFA/db.py:2101-2136), which picks up the ``trans`` table whenever one exists, for either model.  Utterances that
        failed contribute nothing.  Needs the raw models (``raw_tm=``, ``raw_am=`` and, for the alignment model,
        ``raw_ali_am=`` of the constructor).  Afterwards: ``adapted`` (raw tm, am, ali_am), ``adapt_stats`` /
        ``adapt_ali_stats``, ``adapt_loglike`` and ``adapt_counts``; ``write_adapted`` writes the files."""
        if self.raw_tm is None or self.raw_am is None:
            raise ValueError("adapt needs the models as read from their files: CorpusAligner(..., raw_tm=, raw_am=[, raw_ali_am=])")
        both = bool(speaker_adapted) and self.ali_am is not None
        if both and self.raw_ali_am is None:
            raise ValueError("adapt with an alignment model needs raw_ali_am= as well")
        with self._run():
            results, kept = self._align(list(utterances), speaker_adapted, make_ctm, None, keep_last=True)
        n_tids = self.tm.num_transition_ids + 1

        def accumulate(raw):
            model = DiagGmmModel.from_raw(raw)
            self.engine.load_gmm(model)
            self._loaded = model
            st = GmmStats.zeros(model.num_gauss, model.dim, n_tids)
            for _idx, feats, ali, _fo, _rows in kept:
                gmm_statistics(self.engine, feats, ali, self.tm, into=st)
            return st

        self.adapt_stats = accumulate(self.raw_am)
        new_am, up, keep = _adapt.adapt_model(self.raw_am, self.adapt_stats, mapping_tau)
        self.adapt_counts = {"mdl": (up, keep)}
        self.adapt_loglike = {"mdl": self.adapt_stats.loglike_per_frame, "alimdl": None}
        new_ali, self.adapt_ali_stats = None, None
        if both:
            self.adapt_ali_stats = accumulate(self.raw_ali_am)
            new_ali, up, keep = _adapt.adapt_model(self.raw_ali_am, self.adapt_ali_stats, mapping_tau)
            self.adapt_counts["alimdl"] = (up, keep)
            self.adapt_loglike["alimdl"] = self.adapt_ali_stats.loglike_per_frame
        new_tm = _adapt.transition_update(self.raw_tm, self.adapt_stats.tid_count) if update_transitions else self.raw_tm
        self.adapted = (new_tm, new_am, new_ali)
        self._reload(new_tm, new_am, new_ali)
        return results

    # ------------------------------------------------------------------ LDA estimation
    def _lda_accumulate(self, utts, kept, spk_ids, cmvn, splice_context: int, rand_prune: float, seed: int) -> LdaStats:
        """LDA statistics of the alignments ``kept`` (of ``_align(..., keep_last=True)``, inside the same ``_run``) on the
        base features as ``_mfcc`` / ``speaker_cmvn`` make them — with ``corpus_compression`` the twice-compressed
        CMVN-applied rows without CMVN, exactly what ``_final_features`` hands the feature kernel.  Classes are pdfs, silence
        weighs 0 (weight-silence-post 0.0), utterance keys are corpus positions."""
        eng = self.engine
        weights = silence_weights(self.tm, self.silence_phones, 0.0)
        st = None
        for idx, _feats, ali, fo, rows in kept:
            mfcc, fo2 = self._mfcc(utts, idx)
            assert np.array_equal(fo, fo2)
            use_cmvn = cmvn
            if self.opt.corpus_compression:
                mfcc = eng.compress_round_trip(mfcc, fo, cols=(0, mfcc.shape[1] - self.n_pitch), cmvn=cmvn, utt2spk=rows)
                use_cmvn = None
            st = lda_statistics(eng, mfcc, fo, rows, use_cmvn, ali, self.tm, splice_context=splice_context, weights=weights,
                                rand_prune=rand_prune, utt_keys=np.asarray(idx, dtype=np.uint32), seed=seed, into=st)
        if st is None:
            raise ValueError("estimate_lda: no utterances")
        return st

    def estimate_lda(self, utterances: Sequence[CorpusUtterance], dim: int = 40, splice_context: int = 3, rand_prune: float = 0.0,
                     seed: int = 0):
        """The LDA stage's estimate (MFA/acoustic_modeling/lda.py:54-119, 352-373): align with this aligner's model on its
        own features, accumulate LDA statistics of those alignments in the spliced space of the base features on the device
        (``lda_statistics``, batch by batch into one ``LdaStats``, kept as ``lda_stats``) and return
        ``lda.estimate_lda(stats, dim)`` = (lda_mat [dim, S], full [S, S]).  ``rand_prune``: the reference prunes at 4.0
        because its accumulation is slow; here every frame is affordable and the default is 0 (off)."""
        from .lda import estimate_lda as _estimate

        utts = list(utterances)
        with self._run():
            _results, kept = self._align(utts, False, False, None, keep_last=True)
            spk_ids, cmvn = self.speaker_cmvn(utts)            # (from the cached MFCCs: the bits of the alignment pass)
            self.lda_stats = self._lda_accumulate(utts, kept, spk_ids, cmvn, int(splice_context), float(rand_prune), int(seed))
        return _estimate(self.lda_stats, dim=dim)

    # ------------------------------------------------------------------ MLLT estimation
    def _mllt_accumulate(self, kept, raw_am) -> MlltStats:
        """MLLT statistics of the resident features and alignments ``kept`` under ``raw_am`` as its file holds it (no silence
        boost), silence at weight 0.  The accumulators stay on the device over the batches (``MlltStats``)."""
        model = DiagGmmModel.from_raw(raw_am)
        self.engine.load_gmm(model)
        self._loaded = model
        weights = silence_weights(self.tm, self.silence_phones, 0.0)
        st = MlltStats.zeros(model.num_gauss, model.dim)
        for _idx, feats, ali, _fo, _rows in kept:
            mllt_statistics(self.engine, feats, ali, self.tm, weights, into=st)
        return st

    def estimate_mllt(self, utterances: Sequence[CorpusUtterance], num_sweeps: int = 200):
        """The MLLT estimate of the LDA+MLLT stage (MFA/acoustic_modeling/lda.py:122-180, 399-410), the sibling of
        ``estimate_lda``: align with this aligner's model on its own features, keep features and alignments resident,
        accumulate MLLT statistics under ``raw_am`` with silence at weight 0 on the device (``mllt_statistics``, kept as
        ``mllt_stats``) and return ``mllt.estimate_mllt(*mllt.mllt_accs(stats, raw_am))`` = (mat [D, D], objf_impr, count,
        trace).  Needs ``raw_am=`` of the constructor."""
        from . import mllt as _mllt

        if self.raw_am is None:
            raise ValueError("estimate_mllt needs the model as read from its file: CorpusAligner(..., raw_am=)")
        with self._run():
            _results, kept = self._align(list(utterances), False, False, None, keep_last=True)
            self.mllt_stats = self._mllt_accumulate(kept, self.raw_am)
            self._load(self.am)
        beta, G = _mllt.mllt_accs(self.mllt_stats, self.raw_am)
        return _mllt.estimate_mllt(beta, G, num_sweeps=num_sweeps)

    # ------------------------------------------------------------------ alignment model of a speaker-adapted model
    def _twofeats_accumulate(self, utts, kept, spk_ids, cmvn, raw_am, tm: Optional[TransitionModel] = None) -> GmmStats:
        """Two-feature GMM statistics of the resident batches ``kept`` (adapted features and alignments of
        ``_align(..., keep_last=True)``, inside the same ``_run``): posteriors on the resident features, sums of the same
        frames' unadapted features (no transform; the MFCC cache is used), under ``raw_am`` as its file holds it.  ``tm``:
        the transition model of the alignments (default: the aligner's)."""
        model = DiagGmmModel.from_raw(raw_am)
        self.engine.load_gmm(model)
        self._loaded = model
        tm = self.tm if tm is None else tm
        d_lda = None if self.lda is None else torch.from_numpy(self.lda).to(self.engine.device)
        st = GmmStats.zeros(model.num_gauss, model.dim, tm.num_transition_ids + 1)
        for idx, feats, ali, fo, _rows in kept:
            unadapted, fo2, _rows2 = self._batch_features(utts, idx, spk_ids, cmvn, d_lda, None)
            assert np.array_equal(fo, fo2)
            gmm_statistics_twofeats(self.engine, feats, unadapted, ali, tm, into=st)
        return st

    def estimate_alignment_model(self, utterances: Sequence[CorpusUtterance], power: float = 0.25):
        """The alignment model of the SAT stage (MFA/acoustic_modeling/sat.py:46-130, :307-372; Kaldi
        gmm-acc-stats-twofeats + gmm-est), the sibling of ``estimate_lda`` / ``estimate_mllt``: align with
        ``speaker_adapted=True``, keep the last pass's adapted features and alignments resident, accumulate two-feature
        statistics under ``raw_am`` as its file holds it — posteriors on the adapted features, sums of the unadapted ones
        (``gmm_statistics_twofeats``, kept as ``alimdl_stats``) — and return ``train.alignment_model``'s
        (ali_raw_tm, ali_raw_am) with the statistics: (ali_raw_tm, ali_raw_am, stats).  ``power`` is the reference's mix-up
        exponent; there is no mix-up here (``train.alignment_model`` says why), so it changes nothing.  Needs ``raw_tm=``
        and ``raw_am=`` of the constructor."""
        from .train import alignment_model

        if self.raw_tm is None or self.raw_am is None:
            raise ValueError("estimate_alignment_model needs the models as read from their files: CorpusAligner(..., raw_tm=, raw_am=)")
        utts = list(utterances)
        with self._run():
            _results, kept = self._align(utts, True, False, None, keep_last=True)
            spk_ids, cmvn = self.speaker_cmvn(utts)            # (from the cached MFCCs: the bits of the alignment passes)
            self.alimdl_stats = self._twofeats_accumulate(utts, kept, spk_ids, cmvn, self.raw_am)
            self._load(self.am)
        ali_raw_tm, ali_raw_am = alignment_model(self.raw_tm, self.raw_am, self.alimdl_stats)
        return ali_raw_tm, ali_raw_am, self.alimdl_stats

    # ------------------------------------------------------------------ tree statistics
    def _tree_accumulate(self, kept, ci_phones: Sequence[int]):
        """Tree statistics of the resident features and alignments ``kept`` (of ``_align(..., keep_last=True)``): the device
        call per batch (``stats.tree_statistics``), the batches merged on the host in batch order.  Returns (``TreeStats`` of
        all batches or None, per batch (its ``TreeStats``, ``frame_event`` on the device), utterances skipped)."""
        total, batches, skipped = None, [], 0
        for _idx, feats, ali, fo, _rows in kept:
            st, frame_event, n = tree_statistics(self.engine, feats, fo, ali, self.tm, ci_phones)
            batches.append((st, frame_event))
            skipped += n
            if total is None:
                total = st.copy()
            else:
                total += st
        return total, batches, skipped

    def tree_statistics(self, utterances: Sequence[CorpusUtterance], ci_phones: Optional[Sequence[int]] = None) -> TreeStats:
        """The tree statistics of the triphone stage (MFA/acoustic_modeling/triphone.py, ``TreeStatsFunction``): align with this
        aligner's model on its own features, keep features and alignments resident, accumulate per (left, centre, right,
        pdf-class) on the device.  ``ci_phones``: the context-independent phones (default: the silence phones).  Kept as
        ``tree_stats``; ``tree_skipped`` counts the utterances whose alignment did not end a phone."""
        ci = self.silence_phones if ci_phones is None else list(ci_phones)
        with self._run():
            _results, kept = self._align(list(utterances), False, False, None, keep_last=True)
            self.tree_stats, _batches, self.tree_skipped = self._tree_accumulate(kept, ci)
        if self.tree_stats is None:
            raise ValueError("tree_statistics: no utterances")
        return self.tree_stats

    # ------------------------------------------------------------------ pronunciation probabilities
    def pronunciation_statistics(self, utterances: Sequence[CorpusUtterance], speaker_adapted: bool = False):
        """The counts of the pronunciation-probability stage (GeneratePronunciationsFunction, MFA/alignment/multiprocessing.py:
        1476-1570): ``align`` with the interval stage on, then ``pronprob.count_from_intervals`` over every batch's interval
        arrays — the tables ``pronprob.count_from_ctm`` gives over the ``ctm`` objects of the same alignment, without building
        one.  An utterance counts in the batch its result comes from (with an alignment model: the first pass's when the
        second lost it); one that failed, or whose interval stage failed, counts nowhere.  Kept as ``pronunciation_counts``."""
        from . import pronprob

        with self._run():
            results = self._align(list(utterances), speaker_adapted, True, None)[0]
        ex = self._extractor()
        index = pronprob.PronunciationIndex(self.lexicon)
        chosen: Dict[int, tuple] = {}                     # per batch: its interval arrays and the utterances that count in it
        by_object = []                                    # (an utterance only the Python interval stage could take: its ctm)
        for r in results:
            if r is not None and r._lazy is not None:
                batch, k = r._lazy[0], r._lazy[1]
                chosen.setdefault(id(batch), (batch, np.zeros(batch.n_utt, dtype=bool)))[1][k] = True
            elif r is not None and r._ctm is not None:
                by_object.append(r._ctm)
        del results
        counts = pronprob.count_from_ctm(self.lexicon, by_object, index)
        for batch, select in chosen.values():
            counts += pronprob.count_from_intervals(ex, batch, select, index)
        self.pronunciation_counts = counts
        return counts

    def train_dictionary(self, utterances: Sequence[CorpusUtterance], speaker_adapted: bool = False):
        """``mfa train_dictionary`` on this aligner's model (DictionaryTrainer, MFA/alignment/pretrained.py:561-613):
        ``pronunciation_statistics`` then ``pronprob.estimate`` — (a new ``LexiconCompiler`` with the re-estimated records,
        the four silence numbers).  The aligner keeps the lexicon it has; ``pronprob.write_dictionary`` /
        ``write_silence_info`` write the result."""
        from . import pronprob

        return pronprob.estimate(self.lexicon, self.pronunciation_statistics(utterances, speaker_adapted))

    def _reload(self, raw_tm, raw_am, raw_ali_am) -> None:
        """Make the adapted models the aligner's own: transition model (graphs, scaled probabilities), boosted copies, device."""
        self.raw_tm, self.raw_am = raw_tm, raw_am
        self.tm = TransitionModel(raw_tm)
        self.am = self._boosted(DiagGmmModel.from_raw(raw_am))
        if raw_ali_am is not None:
            self.raw_ali_am = raw_ali_am
            self.ali_am = self._boosted(DiagGmmModel.from_raw(raw_ali_am))
        self.compiler = _graph.TrainingGraphCompiler(self.tm, self.tree, self.lexicon)
        self.scaled = self.tm.scaled_log_probs(self.opt.transition_scale, self.opt.self_loop_scale)
        self._intervals = None
        self._load(self.am)

    def write_adapted(self, directory) -> List[Path]:
        """``final.mdl`` and, when the alignment model was adapted, ``final.alimdl`` of the last ``adapt``."""
        if self.adapted is None:
            raise ValueError("write_adapted: adapt has not been run")
        out_dir = Path(directory)
        out_dir.mkdir(parents=True, exist_ok=True)
        tm, am, ali = self.adapted
        written = []
        for name, model in (("final.mdl", am), ("final.alimdl", ali)):
            if model is not None:
                with open(out_dir / name, "wb") as f:
                    kaldi_io.write_model(f, tm, model)
                written.append(out_dir / name)
        return written

    def _extractor(self):
        if self._intervals is None:
            from . import intervals_native
            self._intervals = intervals_native.IntervalExtractor(self.tm, self.lexicon, self.frame_shift)
        return self._intervals

    def _results(self, utts, results, make_ctm) -> List[Optional[UtteranceResult]]:
        """Per-utterance results from the batch outputs.  With ``make_ctm`` the interval stage — generate_ctm →
        phones_to_pronunciations → update_utterance_boundaries → fix_unk_words, MFA/alignment/multiprocessing.py:1733-1751 —
        runs once per batch over the arrays (intervals_native); the ``HierarchicalCtm`` objects are built when a caller asks
        an ``UtteranceResult`` for its ``ctm``.  Per utterance, as the reference's extraction loop: an alignment the stage
        cannot take concerns this utterance only (:1739-1770 catches, logs and continues)."""
        if make_ctm:
            ex = self._extractor()
            for bo in {id(r[0]): r[0] for r in results if r is not None}.values():
                if bo.intervals is None:
                    bo.intervals = ex.extract(bo.frame_off, bo.ali, bo.words, bo.n_words, bo.status)
        out: List[Optional[UtteranceResult]] = []
        for u, r in zip(utts, results):
            if r is None:
                self.failed.append(u.utt_id)
                self.failure_reasons.setdefault(u.utt_id, "no alignment")
                out.append(None)
                continue
            bo, k = r
            a, b = int(bo.frame_off[k]), int(bo.frame_off[k + 1])
            ur = UtteranceResult(u.utt_id, u.speaker, bo.ali[a:b], bo.words[a: a + int(bo.n_words[k])], float(bo.like[k]), b - a)
            if make_ctm:
                end = u.begin + self.audio_seconds(u)
                if bo.intervals.err[k] == 0:
                    ur._lazy = (bo.intervals, k, u.text, u.begin, end)
                else:
                    try:                    # the Python specification on this utterance: it raises the specific error
                        ur.ctm = bo.intervals.ctm(k, text=u.text, begin=u.begin, end=end, likelihood=ur.per_frame_likelihood)
                    except Exception as e:  # noqa: BLE001
                        self.failure_reasons[u.utt_id] = f"interval extraction failed: {e}"
                        self.ctm_failed.append(u.utt_id)
            out.append(ur)
        return out

    def export_textgrids(self, utterances: Sequence[CorpusUtterance], results: Sequence[Optional[UtteranceResult]], output_directory,
                         output_format: str = "long_textgrid", cleanup_silence: bool = True) -> List[Path]:
        """One file per sound file, one (words, phones) tier pair per speaker (export_textgrid, MFA/textgrid.py:463-572).

        Files whose utterances still carry their interval arrays (the results of ``align``) are written from those arrays
        by the native writer — byte for byte what ``ctm.export_textgrid`` writes (tests/test_intervals_native_cpu.py);
        anything else (results whose ``ctm`` a caller set or changed, a file the native writer declines) goes through the
        Python objects."""
        out_dir = Path(output_directory)
        out_dir.mkdir(parents=True, exist_ok=True)
        ext = {"long_textgrid": ".TextGrid", "short_textgrid": ".TextGrid", "json": ".json", "csv": ".csv"}[output_format]
        per_file: Dict[str, dict] = {}
        for n, (u, r) in enumerate(zip(utterances, results)):
            if r is None or not r.has_intervals:
                continue
            name = u.file_name or u.utt_id
            f = per_file.get(name)
            if f is None:
                f = per_file[name] = dict(name=name, duration=0.0, speakers={}, native=True)
            end = u.begin + self.audio_seconds(u)
            f["duration"] = max(f["duration"], u.file_duration or end)
            f["speakers"].setdefault(u.speaker, []).append(n)
            if r._lazy is None:
                f["native"] = False
        written: List[Path] = []
        slow = [f for f in per_file.values() if not f["native"]]
        fast = [f for f in per_file.values() if f["native"]]
        if fast:
            from . import intervals_native
            # the interval arrays of the batches involved, laid end to end: utterance (batch, k) becomes base[batch] + k
            batches, base = {}, {}
            for f in fast:
                for ns in f["speakers"].values():
                    for n in ns:
                        b = results[n]._lazy[0]
                        if id(b) not in batches:
                            base[id(b)] = sum(x.n_utt for x in batches.values())
                            batches[id(b)] = b
            merged = intervals_native.IntervalBatch.concat(list(batches.values()))
            total = merged.n_utt
            ub_l, ue_l = [0.0] * total, [0.0] * total          # (plain lists: per-element numpy stores cost more than the loop)
            texts: List[Optional[str]] = [None] * total
            files = []
            for f in fast:
                spk = []
                for name, ns in f["speakers"].items():
                    ids = []
                    for n in ns:
                        b, k, text, begin, end = results[n]._lazy
                        m = base[id(b)] + k
                        ub_l[m] = begin; ue_l[m] = end; texts[m] = text
                        ids.append(m)
                    spk.append((name, ids))
                files.append(dict(duration=f["duration"], speakers=spk))
            ub, ue = np.asarray(ub_l, dtype=np.float64), np.asarray(ue_l, dtype=np.float64)
            paths = [str(out_dir / (f["name"] + ext)) for f in fast]
            _none, codes = self._extractor().write_files(merged, files, ub, ue, merged.relabels(texts), output_format, cleanup_silence,
                                                          paths=paths)          # text AND files by the library's threads
            for f, path, code in zip(fast, paths, codes):
                if code == 0:
                    written.append(Path(path))
                elif code == 1:
                    slow.append(f)          # the Python writer raises the reference's error for this file
        sil = self.lexicon.silence_word
        for f in slow:
            speakers = {}
            for name, ns in f["speakers"].items():
                tiers = speakers.setdefault(name, {"words": [], "phones": []})
                for n in ns:
                    for w in results[n].ctm.word_intervals:
                        if cleanup_silence and w.label == sil:
                            continue
                        tiers["words"].append(_ctm.CtmInterval(w.begin, w.end, w.label))
                        tiers["phones"].extend(w.phones)
                tiers["words"].sort(); tiers["phones"].sort()
            path = out_dir / (f["name"] + ext)
            _ctm.export_textgrid(speakers, path, f["duration"], self.frame_shift, output_format)
            if path.exists():
                written.append(path)
        order = {name: k for k, name in enumerate(per_file)}
        written.sort(key=lambda p_: order.get(p_.name[: -len(ext)], 0))
        return written


def align_sharded(aligner_factory, utterances: Sequence[CorpusUtterance], rank: int, world_size: int, **kw):
    """One process per GPU: this rank aligns the speakers ``sharding.assign_speakers`` gives it (weights = audio seconds)
    and every rank receives all results (host-side object gather; no collective on the data path)."""
    spk_index = {s: k for k, s in enumerate(dict.fromkeys(u.speaker for u in utterances))}
    aligner = aligner_factory()
    # (samples weigh the same as seconds while every utterance is at the model's rate; with rates of their own, seconds)
    if all(getattr(u, "sample_rate", None) is None for u in utterances):
        weights = [len(u.pcm) for u in utterances]
    else:
        weights = [aligner.audio_seconds(u) for u in utterances]
    rank_of = sharding.assign_speakers([spk_index[u.speaker] for u in utterances], world_size, weights=weights)
    mine = sharding.local_indices(rank_of, rank)
    local = aligner.align([utterances[i] for i in mine], **kw)
    gathered = sharding.gather_results({int(i): r for i, r in zip(mine, local)}, world_size)
    return [gathered.get(i) for i in range(len(utterances))]
