"""Flat-start monophone training: the reference's ``MonophoneTrainer`` (MFA/acoustic_modeling/monophone.py; loop in
MFA/acoustic_modeling/base.py:769-833) over the device pipeline.  A corpus, a lexicon and a topology in — no model, no
labels — ``final.mdl`` and ``tree`` out.

  iteration 0   equal alignments (mfa_align_equal_batch) → GMM statistics → the flat-start model: every pdf at the global
                mean and variance (the statistics summed over all pdfs: a one-Gaussian pdf's posterior is 1 whatever its
                parameters), then transition update + ``mle_update(min_gaussian_occupancy=3)`` + mix-up to the current target
  iteration i   realign when scheduled (with ``initial_beam`` at iteration 1) → statistics → ``adapt.transition_update`` →
                ``mle.mle_update`` → ``mle.mix_up`` to the current target; the target grows by ``gaussian_increment`` while
                i <= ``final_gaussian_iteration``

The device is driven through a backend of three calls — ``equal_align``, ``align``, ``accumulate`` — so that the same loop
runs on the host twins in tests.  ``DeviceBackend`` is ``CorpusAligner``'s machinery: features, CMVN and graphs as ``align``
makes them, ``_align(..., keep_last=True)`` for features and alignments that stay on the device, ``gmm_statistics(into=)``.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import adapt as _adapt
from . import kaldi_io, mle
from .model import DiagGmmModel, TransitionModel
from .stats import GmmStats


def realignment_iterations(num_iterations: int) -> List[int]:
    """MonophoneTrainer.compute_calculated_properties: every iteration of the first quarter, every second of the second,
    every third afterwards."""
    out = [0]
    for i in range(1, num_iterations):
        if i <= int(num_iterations / 4):
            out.append(i)
        elif i <= int(num_iterations * 2 / 4):
            if i - out[-1] > 1:
                out.append(i)
        elif i - out[-1] > 2:
            out.append(i)
    return out


class DeviceBackend:
    """The three calls on the device, through a ``CorpusAligner`` built on first use.  Features and alignments of the last
    alignment stay on the device, per batch, between the calls."""

    def __init__(self, utterances, lexicon, options=None, mfcc_options: Optional[dict] = None, silence_phones: Sequence[int] = (),
                 device: int = 0, engine=None):
        from .aligner import AlignOptions

        self.utts = list(utterances)
        self.lexicon, self.opt = lexicon, options or AlignOptions()
        self.mfcc_options, self.silence_phones = dict(mfcc_options or {}), list(silence_phones)
        self.device, self.engine = device, engine
        self.al = None
        self.kept: List[tuple] = []          # per batch (utterance indices, features, alignments, frame offsets, speaker rows)
        self.dim = 3 * int(self.mfcc_options.get("num_coefficients", 13))

    def _aligner(self, raw_tm, raw_am, tree):
        from .aligner import CorpusAligner

        if self.al is None:
            self.al = CorpusAligner(TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am), tree, self.lexicon, options=self.opt,
                                    device=self.device, engine=self.engine, mfcc_options=self.mfcc_options,
                                    silence_phones=self.silence_phones, raw_tm=raw_tm, raw_am=raw_am)
            self.engine = self.al.engine
        else:
            self.al._reload(raw_tm, raw_am, None)
        return self.al

    def equal_align(self, raw_tm, raw_am, tree, seed: int) -> int:
        from .equal_align import equal_align

        al = self._aligner(raw_tm, raw_am, tree)
        self.kept, failed = [], 0
        with al._run():
            spk_ids, cmvn = al.speaker_cmvn(self.utts)
            for idx in al._batches(self.utts):
                fsts = al.compiler.compile_fsts([self.utts[i].text for i in idx], al.scaled, columns=True)
                graphs = al.engine.pack_graphs(fsts, al.tm)
                feats, fo, rows = al._batch_features(self.utts, idx, spk_ids, cmvn, None, None)
                # the key is the utterance's position in the corpus: its path does not depend on how batches are cut
                ali, status = equal_align(al.engine, graphs, fo, np.asarray(idx, dtype=np.uint32), seed)
                failed += int((status != 0).sum().item())
                self.kept.append((list(idx), feats, ali, fo, rows))
        return failed

    def align(self, raw_tm, raw_am, tree, beam: float) -> int:
        al = self._aligner(raw_tm, raw_am, tree)
        usual = al.opt.beam
        al.opt.beam = float(beam)
        try:
            with al._run():
                results, self.kept = al._align(self.utts, False, False, None, keep_last=True)
        finally:
            al.opt.beam = usual
        return sum(r is None for r in results)

    def accumulate(self, raw_tm, raw_am) -> GmmStats:
        """Statistics of the resident alignments under the model as its file would hold it (no silence boost)."""
        from .stats import gmm_statistics

        al = self.al
        model = DiagGmmModel.from_raw(raw_am)
        al.engine.load_gmm(model)
        al._loaded = model
        tm = TransitionModel(raw_tm)
        st = GmmStats.zeros(model.num_gauss, model.dim, tm.num_transition_ids + 1)
        for _idx, feats, ali, _fo, _rows in self.kept:
            gmm_statistics(al.engine, feats, ali, tm, into=st)
        return st

    def alignments(self) -> List[np.ndarray]:
        """The resident alignments on the host, by utterance (zeros where an utterance failed)."""
        out: List[Optional[np.ndarray]] = [None] * len(self.utts)
        for idx, _feats, ali, fo, _rows in self.kept:
            a = ali.cpu().numpy()
            for k, i in enumerate(idx):
                out[i] = a[int(fo[k]): int(fo[k + 1])]
        return out


class MonophoneTrainer:
    """``MonophoneTrainer(utterances, lexicon, topology).train()`` then ``write(directory)`` / ``aligner()``.

    Options carry the reference's names and defaults (MFA/acoustic_modeling/monophone.py:160-182): ``num_iterations`` 40,
    ``max_gaussians`` 1000, ``power`` 0.25, ``initial_beam`` 6, ``boost_silence`` 1.25 (in ``align_options``).
    ``history``: one dict per iteration — ``loglike`` (average log-likelihood per frame of the statistics, i.e. of the
    model the iteration started from; iteration 0: of the unit-variance model the accumulator ran with), ``gaussians`` after
    the update, ``failed`` utterances of the alignment in force, ``realigned``, ``mixed_up``, ``target``, ``updated``,
    ``removed``, ``floored``.  Refused with a message: a feature dimension above 48 and a mix-up target above 128 Gaussians in
    a pdf (the statistics kernel's limits), topologies ``graph`` refuses."""

    def __init__(self, utterances=None, lexicon=None, topology: Optional[kaldi_io.HmmTopology] = None, num_iterations: int = 40,
                 max_gaussians: int = 1000, power: float = 0.25, initial_beam: float = 6.0, align_options=None, seed: int = 1234,
                 shared_phones: Optional[Sequence[Sequence[int]]] = None, silence_phones: Sequence[int] = (),
                 mfcc_options: Optional[dict] = None, device: int = 0, engine=None, backend=None):
        from .aligner import AlignOptions

        if topology is None or lexicon is None:
            raise ValueError("MonophoneTrainer needs a lexicon and a topology")
        if num_iterations < 1:
            raise ValueError("num_iterations must be at least 1")
        self.lexicon, self.topology = lexicon, topology
        self.num_iterations, self.max_gaussians, self.power = int(num_iterations), int(max_gaussians), float(power)
        self.initial_beam, self.seed = float(initial_beam), int(seed)
        self.opt = align_options or AlignOptions(boost_silence=1.25)
        self.silence_phones, self.mfcc_options = list(silence_phones), dict(mfcc_options or {})
        self.backend = backend if backend is not None else DeviceBackend(utterances, lexicon, self.opt, self.mfcc_options,
                                                                          self.silence_phones, device, engine)
        self.raw_tm, self.raw_am, self.tree = mle.init_mono(topology, self.backend.dim, shared_phones)
        self.initial_gaussians = self.raw_am.num_pdfs
        self.final_gaussian_iteration = self.num_iterations - 10
        self.realignment_iterations = realignment_iterations(self.num_iterations)
        self.current_gaussians = self.initial_gaussians
        self.rng = np.random.default_rng(self.seed)
        self.history: List[Dict] = []
        self.initial_stats: Optional[GmmStats] = None      # iteration 0's statistics (of the equal alignments)
        self.iteration = 0

    @property
    def gaussian_increment(self) -> int:
        """BaseTrainer.gaussian_increment (MFA/acoustic_modeling/base.py:451-453); 0 when no iteration may add Gaussians."""
        if self.final_gaussian_iteration <= 0:
            return 0
        return int((self.max_gaussians - self.initial_gaussians) / self.final_gaussian_iteration)

    @property
    def num_gaussians(self) -> int:
        return int(sum(w.shape[0] for w in self.raw_am.weights))

    def _update(self, stats: GmmStats, failed: int, realigned: bool, **mle_options) -> None:
        """Transition update, Gaussian update and mix-up to the current target from one iteration's statistics."""
        loglike, before = stats.loglike_per_frame, self.raw_am
        self.raw_tm = _adapt.transition_update(self.raw_tm, stats.tid_count)
        occ = mle.pdf_occupancies(before, stats)
        self.raw_am, updated, removed, floored = mle.mle_update(before, stats, **mle_options)
        n = self.num_gaussians
        if self.current_gaussians > n:
            self.raw_am, _targets = mle.mix_up(self.raw_am, occ, self.current_gaussians, self.power, rng=self.rng)
        self.history.append(dict(iteration=self.iteration, loglike=loglike, frames=stats.tot_count, gaussians=self.num_gaussians,
                                 failed=int(failed), realigned=bool(realigned), mixed_up=self.num_gaussians > n,
                                 target=self.current_gaussians, updated=updated, removed=removed, floored=floored))

    def _flat_start(self, stats: GmmStats) -> kaldi_io.RawAmDiagGmm:
        """gmm-init-mono's model from the statistics of the equal alignments: every pdf at the global mean and variance."""
        n = float(stats.occ.sum())
        if not n > 0:
            raise ValueError("MonophoneTrainer: no utterance could be aligned equally (transcripts longer than their audio?)")
        mean = stats.mean_acc.sum(axis=0) / n
        var = np.maximum(stats.var_acc.sum(axis=0) / n - mean * mean, mle.MIN_VARIANCE)
        iv = (1.0 / var).astype(np.float32)[None]
        mi = mean.astype(np.float32)[None] * iv
        one = np.ones(1, np.float32)
        gc = _adapt.gconsts(one, mi, iv)
        P = self.raw_am.num_pdfs
        return kaldi_io.RawAmDiagGmm(self.raw_am.dim, [gc.copy() for _ in range(P)], [one.copy() for _ in range(P)],
                                     [mi.copy() for _ in range(P)], [iv.copy() for _ in range(P)])

    def train(self) -> "MonophoneTrainer":
        b = self.backend
        # iteration 0
        self.iteration = 0
        failed = b.equal_align(self.raw_tm, self.raw_am, self.tree, self.seed)
        stats = b.accumulate(self.raw_tm, self.raw_am)
        self.initial_stats = stats.copy()
        self.raw_am = self._flat_start(stats)
        self._update(stats, failed, True, min_gaussian_occupancy=3.0)
        for it in range(1, self.num_iterations + 1):
            self.iteration = it
            realign = it in self.realignment_iterations
            if realign:
                failed = b.align(self.raw_tm, self.raw_am, self.tree, self.initial_beam if it == 1 else self.opt.beam)
            stats = b.accumulate(self.raw_tm, self.raw_am)
            self._update(stats, failed, realign)
            if it <= self.final_gaussian_iteration:
                self.current_gaussians += self.gaussian_increment
        return self

    def write(self, directory) -> List[Path]:
        """``final.mdl`` and ``tree``."""
        out = Path(directory)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "final.mdl", "wb") as f:
            kaldi_io.write_model(f, self.raw_tm, self.raw_am)
        with open(out / "tree", "wb") as f:
            kaldi_io.write_tree(f, self.tree)
        return [out / "final.mdl", out / "tree"]

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the trained model (on the training engine when the device backend ran)."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             mfcc_options=self.mfcc_options, silence_phones=self.silence_phones, raw_tm=self.raw_tm,
                             raw_am=self.raw_am, **kw)
