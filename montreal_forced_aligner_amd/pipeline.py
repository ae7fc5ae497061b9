"""``Pipeline``, the unit bench.py times.  It uses the engine's ``device``, ``gmm``, ``mfcc_opts``, ``num_ceps``,
``frame_offsets``, ``_dev``, ``_align_outputs`` and ``_launch_*``; what it reports about itself is in ``pipeline_report``."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ._lib import AlignOpts, ScorePlan
from .packing import PackedGraphs
from .pipeline_report import PipelineReport
from .ragged import _speaker_groups, offsets
from .stats import check_delta_fmllr


class Pipeline(PipelineReport):
    """A fixed-shape batch whose inputs, offsets, graphs and output buffers all live in HBM, so that one ``step()`` is
    nothing but the five kernel launches of the hot path (MFCC → CMVN stats → features → GMM scores → Viterbi).

    This is the unit bench.py times and the shape a corpus aligner would feed: build once per batch shape, refill the
    PCM/graph tensors, call ``step()``.
    """

    def __init__(self, engine, pcm: torch.Tensor, sample_off: np.ndarray, utt2spk: np.ndarray,
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

    def score_and_decode(self) -> None:
        """features + graphs → alignments, scores evaluated lazily per window (mfa_align_features_batch)."""
        if self._plan is None:
            self._plan = self.graphs.plan()
        self.e._launch_align_features(self.graphs, self.gstruct, self._plan, self.feats, self.d_frame_off, self.max_frames,
                                      self.total_frames, self.opts, self.window, self.loglikes, self.d_ll_off, self.d_ll_cols,
                                      self._out)

    # ---- host side of the boundary: alignments land in (pinned) host memory
    def host_output_buffers(self, pinned: bool = True) -> Dict[str, torch.Tensor]:
        return {k: torch.empty(getattr(self, k).shape, dtype=getattr(self, k).dtype, pin_memory=pinned)
                for k in ("ali", "words", "n_words", "like", "status")}

    def outputs_to_host(self, host: Dict[str, torch.Tensor]) -> None:
        """Asynchronous D2H of ali / words / n_words / like / status on the engine's stream."""
        for name, dst in host.items():
            dst.copy_(getattr(self, name), non_blocking=True)
