"""Flat-start monophone training: the reference's ``MonophoneTrainer`` (MFA/acoustic_modeling/monophone.py; loop in
MFA/acoustic_modeling/base.py:769-833) over the device pipeline.  A corpus, a lexicon and a topology in — no model, no
labels — ``final.mdl`` and ``tree`` out.

  iteration 0   equal alignments (mfa_align_equal_batch) → GMM statistics → the flat-start model: every pdf at the global
                mean and variance (the statistics summed over all pdfs: a one-Gaussian pdf's posterior is 1 whatever its
                parameters), then transition update + ``mle_update(min_gaussian_occupancy=3)`` + mix-up to the current target
  iteration i   realign when scheduled (with ``initial_beam`` at iteration 1) → statistics → ``adapt.transition_update`` →
                ``mle.mle_update`` → ``mle.mix_up`` to the current target; the target grows by ``gaussian_increment`` while
                i <= ``final_gaussian_iteration``

``TriphoneTrainer`` (below) builds a tree from the previous model's alignments — tree statistics on the device, questions, tree
and initial model on the host (``tree``) — and trains on it.  ``LdaTrainer`` is the LDA stage, on the tree it is given or on
one it builds the same way: the previous model's alignments → LDA statistics and estimate → one
Gaussian per pdf on the splice + LDA features → the same loop, shared through ``GmmTrainerBase``.  ``SatTrainer`` is the
speaker-adapted stage on either feature path: per-speaker fMLLR under the previous model, a tree on the adapted features, the
same loop with fMLLR re-estimated and composed at ``fmllr_iterations``, and after it the speaker-independent alignment model
(``alignment_model``) from two-feature statistics — posteriors on the adapted features, sums of the unadapted ones —, so that
the stage ends in a ``final.mdl`` + ``final.alimdl`` pair.  ``PronunciationProbabilityTrainer`` (at the end) trains no model: it
aligns with the previous stage's, counts the aligned pronunciations and the silences around them (``pronprob``) and hands the
next stage a lexicon with probabilities.  The speaker path's trainers live in ``speaker_train`` and are re-exported here.

The device is driven through a backend of three calls — ``equal_align``, ``align``, ``accumulate``, and for the tree
``tree_accumulate`` and ``convert_alignments``, for the SAT stage ``align_previous``, ``estimate_transforms`` and
``accumulate_two_feats`` — so that the same loop runs on the host twins in tests.  ``DeviceBackend`` is ``CorpusAligner``'s machinery: features, CMVN and graphs as ``align``
makes them, ``_align(..., keep_last=True)`` for features and alignments that stay on the device, ``gmm_statistics(into=)``.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import adapt as _adapt
from . import kaldi_io, mle
from .model import DiagGmmModel, TransitionModel
from .speaker_train import (DubmTrainer, IvectorDeviceBackend, IvectorHostBackend, IvectorTrainer, UbmDeviceBackend,   # noqa: F401
                            UbmHostBackend)
from .stats import GmmStats, fmllr_statistics, gmm_statistics


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
        self.lda: Optional[np.ndarray] = None     # LdaDeviceBackend sets it: the aligner's features are then splice + LDA
        self.kept: List[tuple] = []          # per batch (utterance indices, features, alignments, frame offsets, speaker rows)
        self.tree_batches: List[tuple] = []  # per batch (its TreeStats, frame_event) of the last ``tree_accumulate``
        self.dim = 3 * int(self.mfcc_options.get("num_coefficients", 13))

    def _aligner(self, raw_tm, raw_am, tree):
        from .aligner import CorpusAligner

        if self.al is None:
            self.al = CorpusAligner(TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am), tree, self.lexicon, lda=self.lda,
                                    options=self.opt, device=self.device, engine=self.engine, mfcc_options=self.mfcc_options,
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
        al = self.al
        model = DiagGmmModel.from_raw(raw_am)
        al.engine.load_gmm(model)
        al._loaded = model
        tm = TransitionModel(raw_tm)
        st = GmmStats.zeros(model.num_gauss, model.dim, tm.num_transition_ids + 1)
        for _idx, feats, ali, _fo, _rows in self.kept:
            gmm_statistics(al.engine, feats, ali, tm, into=st)
        return st

    def tree_accumulate(self, raw_tm, ci_phones: Sequence[int]):
        """Tree statistics of the resident features and alignments (``CorpusAligner._tree_accumulate``): (``TreeStats`` of the
        corpus, utterances skipped).  Every batch's own statistics and ``frame_event`` stay for ``convert_alignments``."""
        stats, self.tree_batches, skipped = self.al._tree_accumulate(self.kept, ci_phones)
        return stats, skipped

    def convert_alignments(self, old_raw_tm, raw_tm, raw_am, tree) -> None:
        """The resident alignments moved onto the new model's transition-ids, in place — a gather through
        ``tree.convert_table`` per batch, on the device — and a new aligner on the new tree; the resident features stay."""
        from . import tree as _tree

        old_tm, new_tm = TransitionModel(old_raw_tm), TransitionModel(raw_tm)
        local = _tree.local_of_tid(old_tm)
        self.kept = [(idx, feats, _tree.convert_alignments(_tree.convert_table(old_tm, new_tm, tree, st), local, fe, ali), fo, rows)
                     for (idx, feats, ali, fo, rows), (st, fe) in zip(self.kept, self.tree_batches)]
        self.tree_batches = []
        self.al = None
        self._aligner(raw_tm, raw_am, tree)

    def alignments(self) -> List[np.ndarray]:
        """The resident alignments on the host, by utterance (zeros where an utterance failed)."""
        out: List[Optional[np.ndarray]] = [None] * len(self.utts)
        for idx, _feats, ali, fo, _rows in self.kept:
            a = ali.cpu().numpy()
            for k, i in enumerate(idx):
                out[i] = a[int(fo[k]): int(fo[k + 1])]
        return out


def previous_models(previous):
    """``previous`` of a stage as (raw_tm, raw_am, tree): the tuple itself, or a trained stage."""
    if hasattr(previous, "raw_tm"):
        return (previous.raw_tm, previous.raw_am, previous.tree)
    return tuple(previous)


def alignment_model(raw_tm, raw_am, stats: GmmStats):
    """The speaker-independent alignment model (``final.alimdl``) of a speaker-adapted model from its two-feature statistics
    (``stats.gmm_statistics_twofeats``: posteriors on the adapted features, sums of the unadapted ones):
    (``adapt.transition_update(raw_tm, stats.tid_count)``, ``mle.mle_update(raw_am, stats,
    remove_low_count_gaussians=False)[0]``).

    There is no mix-up.  The reference passes ``mixup=current_gaussians`` here (MFA/acoustic_modeling/sat.py:352-357), Kaldi's
    ``train_sat.sh`` does not mix up, and ``CorpusAligner`` and ``mfa_fmllr_stats_model`` refuse an alignment model whose
    Gaussians per pdf differ from ``final.mdl``'s: the layout of ``raw_am`` is kept, Gaussian for Gaussian."""
    return _alignment_model(raw_tm, raw_am, stats)[:2]


def _alignment_model(raw_tm, raw_am, stats: GmmStats):
    """``alignment_model`` and the update's counts: (ali_raw_tm, ali_raw_am, Gaussians updated, variances floored)."""
    new_am, updated, _removed, floored = mle.mle_update(raw_am, stats, remove_low_count_gaussians=False)
    return _adapt.transition_update(raw_tm, stats.tid_count), new_am, updated, floored


def default_roots(topology: kaldi_io.HmmTopology, shared_phones, silence_phones: Sequence[int]):
    """The reference's ``roots.int`` (MFA/dictionary/mixins.py:845-879): one root per ``mle.phone_sets`` entry, shared and
    split — the silence phones' not shared and not split."""
    sil = set(int(p) for p in silence_phones)
    return [(s, False, False) if sil & set(s) else (s, True, True) for s in mle.phone_sets(topology, shared_phones)]


def tree_stage(backend, prev_tm, topology, roots, shared_phones, ci_phones, extra_questions, num_leaves: int,
               cluster_threshold: float):
    """Tree statistics of the resident alignments → questions (the automatic ones, then ``extra_questions``) → tree →
    ``init_model`` → the alignments converted in place and a new aligner on the new tree.  Returns (raw_tm, raw_am, tree,
    what the stage's ``history`` entry carries)."""
    from . import tree as _tree

    stats, skipped = backend.tree_accumulate(prev_tm, ci_phones)
    if stats is None or stats.num_events == 0:
        raise ValueError("tree building: the previous model's alignments gave no tree statistics")
    questions = _tree.automatic_questions(stats, mle.phone_sets(topology, shared_phones))
    seen = {tuple(q) for q in questions}
    for q in extra_questions:
        q = sorted(int(p) for p in q)
        if tuple(q) not in seen:
            seen.add(tuple(q))
            questions.append(q)
    roots = list(roots) if roots is not None else default_roots(topology, shared_phones, ci_phones)
    tree, record = _tree.build_tree(topology, questions, stats, roots, max_leaves=num_leaves, cluster_thresh=cluster_threshold)
    raw_tm, raw_am = _tree.init_model(topology, tree, stats)
    backend.convert_alignments(prev_tm, raw_tm, raw_am, tree)
    info = dict(events=stats.num_events, leaves=record["leaves"], skipped=int(skipped), questions=len(questions),
                tree_gain_per_frame=(record["total_gain"] - record["merge_loss"]) / record["frames"])
    return raw_tm, raw_am, tree, dict(info, tree_stats=stats, tree_record=record)


class GmmTrainerBase:
    """What the training stages share: the Gaussian schedule, one iteration's update with its ``history`` entry, the loop
    after iteration 0, and the files.  A stage sets ``backend``, ``raw_tm`` / ``raw_am`` / ``tree``, ``opt``, ``power``,
    ``rng``, ``num_iterations``, ``max_gaussians``, ``initial_gaussians``, ``final_gaussian_iteration``,
    ``realignment_iterations`` and ``current_gaussians``, and runs iteration 0 itself."""

    history: List[Dict]
    iteration = 0

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

    def _iterate(self, failed: int, first_beam: float) -> None:
        """Iterations 1 .. num_iterations (MFA/acoustic_modeling/base.py:769-833): realign when scheduled (iteration 1 with
        ``first_beam``), statistics, update, then the target grows while the iteration is at most ``final_gaussian_iteration``."""
        b = self.backend
        for it in range(1, self.num_iterations + 1):
            self.iteration = it
            realign = it in self.realignment_iterations
            if realign:
                failed = b.align(self.raw_tm, self.raw_am, self.tree, first_beam if it == 1 else self.opt.beam)
            extra = self._before_statistics(it)
            stats = b.accumulate(self.raw_tm, self.raw_am)
            self._update(stats, failed, realign)
            if extra:
                self.history[-1].update(extra)
            if it <= self.final_gaussian_iteration:
                self.current_gaussians += self.gaussian_increment

    def _before_statistics(self, iteration: int) -> Optional[Dict]:
        """A stage's own step between an iteration's realignment and its statistics; what it returns joins the iteration's
        ``history`` entry.  Nothing here."""
        return None

    def write(self, directory) -> List[Path]:
        """``final.mdl`` and ``tree``."""
        out = Path(directory)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "final.mdl", "wb") as f:
            kaldi_io.write_model(f, self.raw_tm, self.raw_am)
        with open(out / "tree", "wb") as f:
            kaldi_io.write_tree(f, self.tree)
        return [out / "final.mdl", out / "tree"]


class MonophoneTrainer(GmmTrainerBase):
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
        self._iterate(failed, self.initial_beam)
        return self

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the trained model (on the training engine when the device backend ran)."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             mfcc_options=self.mfcc_options, silence_phones=self.silence_phones, raw_tm=self.raw_tm,
                             raw_am=self.raw_am, **kw)


# ---- the triphone stage -----------------------------------------------------------------------------------------------------------
class TriphoneTrainer(GmmTrainerBase):
    """The reference's ``TriphoneTrainer`` (MFA/acoustic_modeling/triphone.py): context-dependent models on a tree built here.
    ``TriphoneTrainer(utterances, lexicon, previous=(raw_tm, raw_am, tree)).train()`` then ``write(directory)`` / ``aligner()``;
    ``previous`` may also be the trained stage itself.

      iteration 0   align with ``previous`` → tree statistics of those alignments on the device (``stats.tree_statistics``,
                    context-independent: the silence phones) → ``tree.automatic_questions`` with ``extra_questions`` appended →
                    ``tree.build_tree`` (``roots``; default ``default_roots``) → ``tree.init_model`` → a new aligner on the new
                    tree, the resident features kept → the alignments converted in place (``tree.convert_table``, a gather on
                    the device) → GMM statistics under the initial model, transition update, ``mle_update``
      iteration i   ``GmmTrainerBase._iterate``

    Options carry the reference's names and defaults (triphone.py:213-234): ``num_iterations`` 35, ``num_leaves`` 1000,
    ``max_gaussians`` 10000, ``cluster_threshold`` −1, ``boost_silence`` 1.25 (in ``align_options``), ``power`` 0.25;
    realignment at every tenth iteration, ``final_gaussian_iteration`` = ``num_iterations`` − 10, ``initial_gaussians`` = the
    number of leaves built.  ``history`` as ``MonophoneTrainer``'s; iteration 0's entry also carries ``events``, ``leaves``,
    ``questions``, ``tree_gain_per_frame`` and ``skipped``.  ``tree_stats``, ``tree_record`` and ``questions`` are kept."""

    def __init__(self, utterances=None, lexicon=None, previous=None, roots=None, extra_questions: Sequence[Sequence[int]] = (),
                 num_iterations: int = 35, num_leaves: int = 1000, max_gaussians: int = 10000, cluster_threshold: float = -1.0,
                 power: float = 0.25, align_options=None, seed: int = 1234, min_gaussian_occupancy: float = 3.0,
                 shared_phones: Optional[Sequence[Sequence[int]]] = None, silence_phones: Sequence[int] = (),
                 mfcc_options: Optional[dict] = None, device: int = 0, engine=None, backend=None,
                 context_width: int = 3, central_position: int = 1):
        from .aligner import AlignOptions

        if previous is None or lexicon is None:
            raise ValueError("TriphoneTrainer needs a lexicon and the previous stage's (raw_tm, raw_am, tree)")
        if num_iterations < 1 or num_leaves < 1:
            raise ValueError("num_iterations and num_leaves must be at least 1")
        if (int(context_width), int(central_position)) != (3, 1):
            raise ValueError(f"TriphoneTrainer: context width {context_width} with central position {central_position}: only 3 and 1")
        self.lexicon, self.previous = lexicon, previous_models(previous)
        self.roots, self.extra_questions = roots, [list(q) for q in extra_questions]
        self.num_iterations, self.num_leaves, self.max_gaussians = int(num_iterations), int(num_leaves), int(max_gaussians)
        self.cluster_threshold, self.power, self.seed = float(cluster_threshold), float(power), int(seed)
        self.min_gaussian_occupancy = float(min_gaussian_occupancy)
        self.shared_phones = shared_phones
        self.opt = align_options or AlignOptions(boost_silence=1.25)
        self.silence_phones, self.mfcc_options = list(silence_phones), dict(mfcc_options or {})
        self.backend = backend if backend is not None else DeviceBackend(utterances, lexicon, self.opt, self.mfcc_options,
                                                                          self.silence_phones, device, engine)
        self.raw_tm, self.raw_am, self.tree = self.previous
        self.initial_gaussians = self.raw_am.num_pdfs           # until the tree is built
        self.final_gaussian_iteration = self.num_iterations - 10
        self.realignment_iterations = list(range(10, self.num_iterations, 10))
        self.current_gaussians = self.initial_gaussians
        self.rng = np.random.default_rng(self.seed)
        self.history: List[Dict] = []
        self.initial_stats: Optional[GmmStats] = None
        self.tree_stats = None
        self.tree_record: Optional[Dict] = None
        self.iteration = 0

    def train(self) -> "TriphoneTrainer":
        b = self.backend
        prev_tm, prev_am, prev_tree = self.previous
        self.iteration = 0
        failed = b.align(prev_tm, prev_am, prev_tree, self.opt.beam)
        self.raw_tm, self.raw_am, self.tree, info = tree_stage(b, prev_tm, prev_tm.topo, self.roots, self.shared_phones,
                                                               self.silence_phones, self.extra_questions, self.num_leaves,
                                                               self.cluster_threshold)
        self.tree_stats, self.tree_record = info.pop("tree_stats"), info.pop("tree_record")
        self.initial_gaussians = self.current_gaussians = self.raw_am.num_pdfs
        stats = b.accumulate(self.raw_tm, self.raw_am)
        self.initial_stats = stats.copy()
        self._update(stats, failed, True, min_gaussian_occupancy=self.min_gaussian_occupancy)
        self.history[-1].update(info)
        self._iterate(failed, self.opt.beam)
        return self

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the trained model (on the training engine when the device backend ran)."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             mfcc_options=self.mfcc_options, silence_phones=self.silence_phones, raw_tm=self.raw_tm,
                             raw_am=self.raw_am, **kw)


# ---- the LDA stage ----------------------------------------------------------------------------------------------------------------
class LdaDeviceBackend(DeviceBackend):
    """``LdaTrainer``'s calls on the device: ``DeviceBackend``'s ``align`` / ``accumulate`` / ``alignments`` on splice + LDA
    features, and before them the previous model's alignments, the LDA statistics of those alignments
    (``CorpusAligner._lda_accumulate``) and the same alignments on the new features."""

    def __init__(self, utterances, lexicon, options=None, mfcc_options: Optional[dict] = None, silence_phones: Sequence[int] = (),
                 device: int = 0, engine=None, splice_context: int = 3):
        super().__init__(utterances, lexicon, options, mfcc_options, silence_phones, device, engine)
        self.ctx = int(splice_context)
        self.base_dim = int(self.mfcc_options.get("num_coefficients", 13))
        self.prev_al = None
        self.prev_kept: List[tuple] = []

    def align_previous(self, raw_tm, raw_am, tree, previous_lda, beam: float) -> int:
        from .aligner import CorpusAligner

        al = CorpusAligner(TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am), tree, self.lexicon, lda=previous_lda,
                           options=self.opt, device=self.device, engine=self.engine, mfcc_options=self.mfcc_options,
                           silence_phones=self.silence_phones, raw_tm=raw_tm, raw_am=raw_am)
        self.prev_al, self.engine = al, al.engine
        usual = al.opt.beam
        al.opt.beam = float(beam)
        try:
            with al._run():
                results, self.prev_kept = al._align(self.utts, False, False, None, keep_last=True)
        finally:
            al.opt.beam = usual
        return sum(r is None for r in results)

    def lda_accumulate(self, raw_tm, rand_prune: float, seed: int):
        al = self.prev_al
        with al._run():
            spk_ids, cmvn = al.speaker_cmvn(self.utts)
            return al._lda_accumulate(self.utts, self.prev_kept, spk_ids, cmvn, self.ctx, float(rand_prune), int(seed))

    def set_lda(self, lda: np.ndarray, raw_tm, raw_am, tree) -> None:
        """From here on the features are splice + ``lda``: the aligner is built anew on the model given (of the LDA's
        dimension), and the previous model's alignments stay resident beside their new features."""
        import torch

        self.lda, self.al = np.ascontiguousarray(lda, dtype=np.float32), None
        al = self._aligner(raw_tm, raw_am, tree)
        d_lda = torch.from_numpy(self.lda).to(al.engine.device)
        with al._run():
            spk_ids, cmvn = al.speaker_cmvn(self.utts)
            self.kept = [(idx, al._batch_features(self.utts, idx, spk_ids, cmvn, d_lda, None)[0], ali, fo, rows)
                         for idx, _feats, ali, fo, rows in self.prev_kept]
        self.prev_kept, self.prev_al = [], None

    def mllt_accumulate(self, raw_tm, raw_am):
        """MLLT statistics of the resident alignments under the model as its file would hold it, silence at weight 0
        (``CorpusAligner._mllt_accumulate``: the accumulators stay on the device over the batches)."""
        return self.al._mllt_accumulate(self.kept, raw_am)

    def set_transform(self, lda: np.ndarray) -> None:
        """From here on the features are splice + ``lda`` (the composed matrix, of the same shape): the resident features
        are recomputed from the base features, the alignments stay."""
        import torch

        al = self.al
        self.lda = al.lda = np.ascontiguousarray(lda, dtype=np.float32)
        d_lda = torch.from_numpy(self.lda).to(al.engine.device)
        with al._run():
            spk_ids, cmvn = al.speaker_cmvn(self.utts)
            self.kept = [(idx, al._batch_features(self.utts, idx, spk_ids, cmvn, d_lda, None)[0], ali, fo, rows)
                         for idx, _feats, ali, fo, rows in self.kept]


REFERENCE_MLLT_ITERATIONS = (2, 4, 6, 12)      # LdaTrainer.mllt_iterations of the reference (MFA/acoustic_modeling/lda.py:312)


class LdaTrainer(GmmTrainerBase):
    """The reference's LDA+MLLT ``LdaTrainer`` (MFA/acoustic_modeling/lda.py): on the tree it is given, or — with
    ``num_leaves`` — on a tree it builds itself as the reference's stage does (``_setup_tree``).
    ``LdaTrainer(utterances, lexicon, previous=(raw_tm, raw_am, tree)).train()`` then ``write(directory)``
    (``final.mdl``, ``tree``, ``lda.mat``) / ``aligner()``; ``previous`` may also be the trained stage itself.

      iteration 0   align with ``previous`` on its own features (Δ+ΔΔ, or splice + ``previous_lda``) → LDA statistics of
                    those alignments (classes are pdfs, silence weighs 0) → ``lda.estimate_lda`` → GMM statistics of the same
                    alignments on the splice + LDA features under a one-Gaussian-per-pdf model (the posterior is 1 whatever
                    its parameters) → every pdf at its own mean and variance (floored at ``mle.MIN_VARIANCE``; a pdf not
                    above ``min_gaussian_occupancy`` takes the global ones) → transition update, ``mle_update``, mix-up
                    With ``num_leaves``, after the LDA estimate and before those GMM statistics: tree statistics of the same
                    alignments on the splice + LDA features → questions → tree of at most ``num_leaves`` leaves →
                    ``tree.init_model`` → the alignments converted (``tree_stage``, as ``TriphoneTrainer``'s iteration 0;
                    ``roots``, ``extra_questions``, ``cluster_threshold`` as there).  The default ``num_leaves=None`` leaves
                    the stage exactly as it is without.
      iteration i   ``MonophoneTrainer``'s loop (``GmmTrainerBase._iterate``); at an iteration of ``mllt_iterations``, after the
                    realignment if one is scheduled and before the GMM statistics (MFA/acoustic_modeling/lda.py:372-451):
                    MLLT statistics of the resident alignments (``backend.mllt_accumulate``: per-Gaussian full second
                    moments on the device, silence at weight 0) → ``mllt.mllt_accs`` → ``mllt.estimate_mllt`` → the means
                    moved into the new space (``mllt.transform_means``) → the matrix composed onto ``lda_mat``
                    (``mllt.compose_transforms``) → ``backend.set_transform``: the resident features recomputed, the
                    alignments kept.  The iteration's ``history`` entry gains ``mllt`` = {objf_impr_per_frame, logdet, count}.

    ``mllt_iterations`` defaults to EMPTY, not to the reference's schedule ``REFERENCE_MLLT_ITERATIONS`` = (2, 4, 6, 12): the
    loop without MLLT is what existing callers and tests of this stage run, and an empty schedule reproduces it bit for
    bit; pass ``mllt_iterations=REFERENCE_MLLT_ITERATIONS`` for the reference's stage.  Entries outside
    1..``num_iterations`` are refused.  ``mllt_mats`` keeps every estimated matrix, ``logdet_total`` the sum of their
    log|det|: after an MLLT ``loglike`` is measured in a new space, and only ``loglike + logdet_total`` compares across
    iterations.  ``write`` writes the composed ``lda.mat``.

    Options carry the reference's names and defaults (MFA/acoustic_modeling/lda.py:218-244, triphone.py:213-234, :318-325):
    ``num_iterations`` 35, ``max_gaussians`` 15000, ``power`` 0.25, ``lda_dimension`` 40, ``splice_context`` 3 (both sides),
    ``boost_silence`` 1.0 (in ``align_options``), realignment at every tenth iteration, ``final_gaussian_iteration`` =
    ``num_iterations`` − 10, ``initial_gaussians`` = the number of pdfs (the reference's ``num_leaves``).  ``random_prune``
    defaults to 0, not the reference's 4.0: the reference prunes because its accumulation is slow, and on the device every
    frame is affordable.  ``history`` as ``MonophoneTrainer``'s; ``lda_stats``, ``lda_mat`` [dim, S] and ``lda_full`` [S, S]
    are kept.  Refused with a message: an LDA dimension above the GMM statistics' (48) and a spliced dimension above 128."""

    def __init__(self, utterances=None, lexicon=None, previous=None, previous_lda: Optional[np.ndarray] = None,
                 lda_dimension: int = 40, splice_context: int = 3, num_iterations: int = 35, max_gaussians: int = 15000,
                 power: float = 0.25, random_prune: float = 0.0, align_options=None, seed: int = 1234,
                 min_gaussian_occupancy: float = 3.0, silence_phones: Sequence[int] = (), mfcc_options: Optional[dict] = None,
                 device: int = 0, engine=None, backend=None, mllt_iterations: Sequence[int] = (), mllt_sweeps: int = 200,
                 num_leaves: Optional[int] = None, roots=None, extra_questions: Sequence[Sequence[int]] = (),
                 cluster_threshold: float = -1.0, shared_phones: Optional[Sequence[Sequence[int]]] = None):
        from . import _lib
        from .aligner import AlignOptions

        if previous is None or lexicon is None:
            raise ValueError("LdaTrainer needs a lexicon and the previous stage's (raw_tm, raw_am, tree)")
        if num_iterations < 1:
            raise ValueError("num_iterations must be at least 1")
        self.mllt_iterations = tuple(int(i) for i in mllt_iterations)
        if any(i < 1 or i > int(num_iterations) for i in self.mllt_iterations):
            raise ValueError(f"LdaTrainer: mllt_iterations {self.mllt_iterations} outside 1..{int(num_iterations)}")
        self.mllt_sweeps = int(mllt_sweeps)
        self.mllt_mats: List[np.ndarray] = []
        self.logdet_total = 0.0
        lib = _lib.lib()
        self.lexicon, self.previous = lexicon, previous_models(previous)
        self.num_leaves = None if num_leaves is None else int(num_leaves)
        if self.num_leaves is not None and self.num_leaves < 1:
            raise ValueError("LdaTrainer: num_leaves must be at least 1")
        self.roots, self.extra_questions = roots, [list(q) for q in extra_questions]
        self.cluster_threshold, self.shared_phones = float(cluster_threshold), shared_phones
        self.tree_stats = None
        self.tree_record: Optional[Dict] = None
        self.previous_lda = None if previous_lda is None else np.asarray(previous_lda, dtype=np.float32)
        self.lda_dimension, self.splice_context = int(lda_dimension), int(splice_context)
        if self.lda_dimension < 1 or self.lda_dimension > int(lib.mfa_gmm_acc_max_dim()):
            raise ValueError(f"LdaTrainer: lda_dimension {self.lda_dimension} outside 1..{int(lib.mfa_gmm_acc_max_dim())} "
                             "(the GMM statistics' feature dimension)")
        self.num_iterations, self.max_gaussians, self.power = int(num_iterations), int(max_gaussians), float(power)
        self.random_prune, self.seed = float(random_prune), int(seed)
        self.min_gaussian_occupancy = float(min_gaussian_occupancy)
        self.opt = align_options or AlignOptions(boost_silence=1.0)
        self.silence_phones, self.mfcc_options = list(silence_phones), dict(mfcc_options or {})
        self.backend = backend if backend is not None else LdaDeviceBackend(utterances, lexicon, self.opt, self.mfcc_options,
                                                                             self.silence_phones, device, engine, self.splice_context)
        spliced = (2 * self.splice_context + 1) * int(self.backend.base_dim)
        if self.splice_context < 0 or spliced > int(lib.mfa_lda_acc_max_dim()):
            raise ValueError(f"LdaTrainer: splice context {self.splice_context} on {self.backend.base_dim} base features gives a "
                             f"spliced dimension of {spliced} (the LDA statistics take at most {int(lib.mfa_lda_acc_max_dim())})")
        if self.lda_dimension > spliced:
            raise ValueError(f"LdaTrainer: lda_dimension {self.lda_dimension} above the spliced dimension {spliced}")
        self.raw_tm, self.raw_am, self.tree = self.previous
        self.initial_gaussians = self.raw_am.num_pdfs
        self.final_gaussian_iteration = self.num_iterations - 10
        self.realignment_iterations = list(range(10, self.num_iterations, 10))
        self.current_gaussians = self.initial_gaussians
        self.rng = np.random.default_rng(self.seed)
        self.history: List[Dict] = []
        self.initial_stats: Optional[GmmStats] = None      # iteration 0's statistics (of the previous model's alignments)
        self.lda_stats = None
        self.lda_mat: Optional[np.ndarray] = None
        self.lda_full: Optional[np.ndarray] = None
        self.iteration = 0

    def _unit_model(self, num_pdfs: int) -> kaldi_io.RawAmDiagGmm:
        """One Gaussian per pdf at mean 0, variance 1: what iteration 0's statistics run under."""
        D = self.lda_dimension
        one, mi, iv = np.ones(1, np.float32), np.zeros((1, D), np.float32), np.ones((1, D), np.float32)
        gc = _adapt.gconsts(one, mi, iv)
        return kaldi_io.RawAmDiagGmm(D, [gc.copy() for _ in range(num_pdfs)], [one.copy() for _ in range(num_pdfs)],
                                     [mi.copy() for _ in range(num_pdfs)], [iv.copy() for _ in range(num_pdfs)])

    def _pdf_start(self, stats: GmmStats) -> kaldi_io.RawAmDiagGmm:
        """Every pdf at the mean and variance of its own frames; one not above ``min_gaussian_occupancy`` at the global ones."""
        n = float(stats.occ.sum())
        if not n > 0:
            raise ValueError("LdaTrainer: the previous model aligned no utterance")
        gmean = stats.mean_acc.sum(axis=0) / n
        gvar = np.maximum(stats.var_acc.sum(axis=0) / n - gmean * gmean, mle.MIN_VARIANCE)
        one = np.ones(1, np.float32)
        out = kaldi_io.RawAmDiagGmm(self.lda_dimension, [], [], [], [])
        for p in range(stats.occ.shape[0]):
            mean, var = gmean, gvar
            if stats.occ[p] > self.min_gaussian_occupancy:
                mean = stats.mean_acc[p] / stats.occ[p]
                var = np.maximum(stats.var_acc[p] / stats.occ[p] - mean * mean, mle.MIN_VARIANCE)
            iv = (1.0 / var).astype(np.float32)[None]
            mi = mean.astype(np.float32)[None] * iv
            out.gconsts.append(_adapt.gconsts(one, mi, iv)); out.weights.append(one.copy())
            out.means_invvars.append(mi); out.inv_vars.append(iv)
        return out

    def train(self) -> "LdaTrainer":
        from .lda import estimate_lda

        b = self.backend
        prev_tm, prev_am, tree = self.previous
        self.iteration = 0
        failed = b.align_previous(prev_tm, prev_am, tree, self.previous_lda, self.opt.beam)
        self.lda_stats = b.lda_accumulate(prev_tm, self.random_prune, self.seed)
        self.lda_mat, self.lda_full = estimate_lda(self.lda_stats, dim=self.lda_dimension)
        self.raw_tm, self.tree = prev_tm, tree
        self.raw_am = self._unit_model(prev_am.num_pdfs)
        b.set_lda(self.lda_mat, self.raw_tm, self.raw_am, self.tree)
        info = None
        if self.num_leaves is not None:
            self.raw_tm, _init_am, self.tree, info = tree_stage(b, prev_tm, prev_tm.topo, self.roots, self.shared_phones,
                                                                self.silence_phones, self.extra_questions, self.num_leaves,
                                                                self.cluster_threshold)
            self.tree_stats, self.tree_record = info.pop("tree_stats"), info.pop("tree_record")
            self.raw_am = self._unit_model(_init_am.num_pdfs)
            self.initial_gaussians = self.current_gaussians = self.raw_am.num_pdfs
        stats = b.accumulate(self.raw_tm, self.raw_am)
        self.initial_stats = stats.copy()
        self.raw_am = self._pdf_start(stats)
        self._update(stats, failed, True, min_gaussian_occupancy=self.min_gaussian_occupancy)
        if info:
            self.history[-1].update(info)
        self._iterate(failed, self.opt.beam)
        return self

    def _before_statistics(self, iteration: int) -> Optional[Dict]:
        if iteration not in self.mllt_iterations:
            return None
        from . import mllt

        b = self.backend
        stats = b.mllt_accumulate(self.raw_tm, self.raw_am)
        beta, G = mllt.mllt_accs(stats, self.raw_am)
        mat, impr, count, _trace = mllt.estimate_mllt(beta, G, num_sweeps=self.mllt_sweeps)
        self.raw_am = mllt.transform_means(self.raw_am, mat)
        self.lda_mat = mllt.compose_transforms(mat, self.lda_mat)
        b.set_transform(self.lda_mat)
        logdet = float(np.linalg.slogdet(mat.astype(np.float64))[1])
        self.mllt_mats.append(mat)
        self.logdet_total += logdet
        return dict(mllt=dict(objf_impr_per_frame=impr / count, logdet=logdet, count=count))

    def write(self, directory) -> List[Path]:
        """``final.mdl``, ``tree`` and ``lda.mat`` (with MLLT: the composed matrix)."""
        files = super().write(directory)
        if self.lda_mat is None:
            raise ValueError("LdaTrainer.write: train has not been run")
        with open(Path(directory) / "lda.mat", "wb") as f:
            f.write(b"\0B")
            kaldi_io.write_matrix(f, self.lda_mat)
        return files + [Path(directory) / "lda.mat"]

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the trained model and its LDA matrix (on the training engine when the device backend ran)."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             lda=self.lda_mat, mfcc_options=self.mfcc_options, silence_phones=self.silence_phones,
                             raw_tm=self.raw_tm, raw_am=self.raw_am, **kw)


# ---- the speaker-adapted (SAT) stage ----------------------------------------------------------------------------------------------
FMLLR_MAX_DIM = 41                             # mfa_fmllr_acc_batch's limit (csrc/fmllr.hip)
REFERENCE_FMLLR_ITERATIONS = (2, 4, 6, 12)     # SatTrainer.fmllr_iterations of the reference (MFA/acoustic_modeling/sat.py)


class SatDeviceBackend(DeviceBackend):
    """``SatTrainer``'s calls on the device: ``DeviceBackend``'s on features that carry per-speaker fMLLR transforms.
    ``transforms`` [n_spk, D, D+1] float32 (rows in ``speaker_cmvn``'s order, named by ``speakers``; identity at first) is
    what the resident features carry; ``steps`` keeps every ``estimate_transforms``' own matrices, before composition."""

    def __init__(self, utterances, lexicon, options=None, mfcc_options: Optional[dict] = None, silence_phones: Sequence[int] = (),
                 device: int = 0, engine=None, lda: Optional[np.ndarray] = None):
        super().__init__(utterances, lexicon, options, mfcc_options, silence_phones, device, engine)
        self.lda = None if lda is None else np.ascontiguousarray(lda, dtype=np.float32)
        if self.lda is not None:
            self.dim = int(self.lda.shape[0])
        self.transforms: Optional[np.ndarray] = None
        self.speakers: List[str] = []
        self.steps: List[np.ndarray] = []

    def _speaker_rows(self, al):
        """(speaker → row, CMVN statistics) inside a ``_run``; ``speakers`` by row."""
        spk_ids, cmvn = al.speaker_cmvn(self.utts)
        self.speakers = [name for name, _row in sorted(spk_ids.items(), key=lambda kv: kv[1])]
        return spk_ids, cmvn

    def _aligned(self, al, beam: float, transforms) -> int:
        usual = al.opt.beam
        al.opt.beam = float(beam)
        try:
            with al._run():
                results, self.kept = al._align(self.utts, False, False, transforms, keep_last=True)
                self._speaker_rows(al)
        finally:
            al.opt.beam = usual
        return sum(r is None for r in results)

    def align_previous(self, raw_tm, raw_am, tree, previous_lda, beam: float, previous_transforms: Optional[np.ndarray] = None) -> int:
        """Align with the previous stage's model on its own features — Δ+ΔΔ, or splice + ``previous_lda`` —; with
        ``previous_transforms`` the features carry them and ``transforms`` starts from them, else from the identity.  The
        resident features are the adapted ones."""
        self.lda = None if previous_lda is None else np.ascontiguousarray(previous_lda, dtype=np.float32)
        if self.lda is not None:
            self.dim = int(self.lda.shape[0])
        self.al = None
        al = self._aligner(raw_tm, raw_am, tree)
        prev = None if previous_transforms is None else np.ascontiguousarray(previous_transforms, dtype=np.float32)
        failed = self._aligned(al, beam, prev)
        D, n = self.dim, len(self.speakers)
        if prev is not None and tuple(prev.shape) != (n, D, D + 1):
            raise ValueError(f"previous_transforms of shape {tuple(prev.shape)} for {n} speakers of dimension {D}")
        self.transforms = prev.copy() if prev is not None else np.tile(np.eye(D, D + 1, dtype=np.float32), (n, 1, 1))
        self.steps = []
        return failed

    def estimate_transforms(self, raw_tm, raw_am) -> Dict:
        """Per-speaker fMLLR from the resident adapted features and alignments under the model as its file holds it
        (single-model statistics, ``opt.silence_weight``; ``fmllr.estimate_fmllr(min_count=opt.fmllr_min_count)``), each
        composed onto ``transforms``; the resident features are recomputed with the composed transforms, the alignments
        stay.  Returns speakers (estimated), rejected (names: too few frames, degenerate statistics, no gain), and over the
        estimated speakers objf_impr_per_frame and frames."""
        import torch

        from . import fmllr as _fmllr

        al = self.al
        model = DiagGmmModel.from_raw(raw_am)
        al.engine.load_gmm(model)
        al._loaded = model
        tm = TransitionModel(raw_tm)
        n, D = len(self.speakers), self.dim
        beta, K, G = np.zeros(n), np.zeros((n, D, D + 1)), np.zeros((n, D, D + 1, D + 1))
        for _idx, feats, ali, fo, rows in self.kept:
            ids, b, k, g = fmllr_statistics(al.engine, feats, fo, ali, tm, rows, self.silence_phones, self.opt.silence_weight)
            beta[ids] += b; K[ids] += k; G[ids] += g
        step = np.tile(np.eye(D, D + 1, dtype=np.float32), (n, 1, 1))
        rejected, impr, frames, done = [], 0.0, 0.0, 0
        for s in range(n):
            step[s], gain, why = _fmllr.estimate_fmllr(beta[s], K[s], G[s], min_count=self.opt.fmllr_min_count)
            if why is not None:
                rejected.append(self.speakers[s])
                continue
            done, impr, frames = done + 1, impr + gain, frames + float(beta[s])
            self.transforms[s] = _fmllr.compose_transforms(step[s], self.transforms[s])
        self.steps.append(step)
        d_lda = None if self.lda is None else torch.from_numpy(self.lda).to(al.engine.device)
        d_w = torch.from_numpy(self.transforms).to(al.engine.device)
        with al._run():
            spk_ids, cmvn = self._speaker_rows(al)
            self.kept = [(idx, al._batch_features(self.utts, idx, spk_ids, cmvn, d_lda, d_w)[0], ali, fo, rows)
                         for idx, _feats, ali, fo, rows in self.kept]
        return dict(speakers=done, rejected=rejected, objf_impr_per_frame=impr / frames if frames else 0.0, frames=frames)

    def align(self, raw_tm, raw_am, tree, beam: float) -> int:
        """Realignment on the adapted features: one pass with ``transforms`` in the features."""
        return self._aligned(self._aligner(raw_tm, raw_am, tree), beam, self.transforms)

    def accumulate_two_feats(self, raw_tm, raw_am) -> GmmStats:
        """Two-feature statistics of the resident batches under the model as its file holds it: posteriors on the resident
        adapted features, sums of the same frames' unadapted ones (``CorpusAligner._twofeats_accumulate``)."""
        al = self.al
        with al._run():
            spk_ids, cmvn = self._speaker_rows(al)
            return al._twofeats_accumulate(self.utts, self.kept, spk_ids, cmvn, raw_am, TransitionModel(raw_tm))


class SatTrainer(GmmTrainerBase):
    """The reference's ``SatTrainer`` (MFA/acoustic_modeling/sat.py): a speaker-adapted model on a tree built here, and its
    speaker-independent alignment model.  ``SatTrainer(utterances, lexicon, previous=(raw_tm, raw_am, tree)).train()`` then
    ``write(directory)`` (``final.mdl``, ``tree``, ``final.alimdl``, with an LDA ``lda.mat``) / ``aligner()``.  ``previous`` may
    also be a trained stage: an ``LdaTrainer``'s ``lda_mat`` and a ``SatTrainer``'s ``transforms`` are picked up
    (``previous_lda=`` / ``previous_transforms=`` give them by hand).

      iteration 0   align with ``previous`` on its own features (Δ+ΔΔ, or splice + LDA; with ``previous_transforms`` in them)
                    → unless ``previous_transforms`` was given, per-speaker fMLLR under the previous model
                    (``backend.estimate_transforms``) → tree statistics of the adapted features, questions, tree, initial
                    model, alignments converted (``tree_stage``) → GMM statistics → transition update, ``mle_update``
      iteration i   ``GmmTrainerBase._iterate``; at an iteration of ``fmllr_iterations``, after the realignment if one is
                    scheduled and before the statistics (sat.py:279-297): fMLLR under the current model, composed onto
                    ``transforms``; the resident features are recomputed, the alignments stay
      afterwards    two-feature statistics of the resident batches (``stats.gmm_statistics_twofeats``: posteriors on the
                    adapted features, sums of the unadapted ones) → ``alignment_model`` → ``ali_raw_tm`` / ``ali_raw_am``,
                    with ``alimdl_stats`` and ``history_alimdl`` = {loglike, frames, updated, floored}

    Options carry the reference's names and defaults (sat.py:159-220, triphone.py): ``num_iterations`` 35, ``num_leaves`` 2500,
    ``max_gaussians`` 15000, ``power`` 0.2, ``fmllr_iterations`` (2, 4, 6, 12) — entries outside 1..``num_iterations`` are
    refused —, ``boost_silence`` 1.0 (in ``align_options``), realignment at every tenth iteration,
    ``final_gaussian_iteration`` = ``num_iterations`` − 10.  ``history`` as ``TriphoneTrainer``'s; iteration 0's entry and the
    scheduled iterations' carry ``fmllr`` = {speakers, rejected, objf_impr_per_frame, frames}.  ``transforms`` [n_spk, D, D+1]
    and ``speakers`` (their rows' names) stay on the trainer, ``fmllr_steps`` keeps every estimate before composition.
    Refused with a message: a feature dimension above the GMM statistics' 48, and Δ+ΔΔ features above fMLLR's 41."""

    def __init__(self, utterances=None, lexicon=None, previous=None, previous_lda: Optional[np.ndarray] = None,
                 previous_transforms: Optional[np.ndarray] = None, roots=None, extra_questions: Sequence[Sequence[int]] = (),
                 num_iterations: int = 35, num_leaves: int = 2500, max_gaussians: int = 15000, cluster_threshold: float = -1.0,
                 power: float = 0.2, fmllr_iterations: Sequence[int] = REFERENCE_FMLLR_ITERATIONS, align_options=None,
                 seed: int = 1234, min_gaussian_occupancy: float = 3.0, shared_phones: Optional[Sequence[Sequence[int]]] = None,
                 silence_phones: Sequence[int] = (), mfcc_options: Optional[dict] = None, device: int = 0, engine=None,
                 backend=None):
        from . import _lib
        from .aligner import AlignOptions

        if previous is None or lexicon is None:
            raise ValueError("SatTrainer needs a lexicon and the previous stage's (raw_tm, raw_am, tree)")
        if num_iterations < 1 or num_leaves < 1:
            raise ValueError("num_iterations and num_leaves must be at least 1")
        self.fmllr_iterations = tuple(int(i) for i in fmllr_iterations)
        if any(i < 1 or i > int(num_iterations) for i in self.fmllr_iterations):
            raise ValueError(f"SatTrainer: fmllr_iterations {self.fmllr_iterations} outside 1..{int(num_iterations)}")
        self.lexicon, self.previous = lexicon, previous_models(previous)
        if previous_lda is None:
            previous_lda = getattr(previous, "lda_mat", None)
        if previous_transforms is None:
            previous_transforms = getattr(previous, "transforms", None)
        self.lda_mat = None if previous_lda is None else np.asarray(previous_lda, dtype=np.float32)
        self.previous_transforms = None if previous_transforms is None else np.asarray(previous_transforms, dtype=np.float32)
        self.roots, self.extra_questions = roots, [list(q) for q in extra_questions]
        self.num_iterations, self.num_leaves, self.max_gaussians = int(num_iterations), int(num_leaves), int(max_gaussians)
        self.cluster_threshold, self.power, self.seed = float(cluster_threshold), float(power), int(seed)
        self.min_gaussian_occupancy = float(min_gaussian_occupancy)
        self.shared_phones = shared_phones
        self.opt = align_options or AlignOptions(boost_silence=1.0)
        self.silence_phones, self.mfcc_options = list(silence_phones), dict(mfcc_options or {})
        self.raw_tm, self.raw_am, self.tree = self.previous
        dim, limit = int(self.raw_am.dim), int(_lib.lib().mfa_gmm_acc_max_dim())
        if self.lda_mat is not None and int(self.lda_mat.shape[0]) != dim:
            raise ValueError(f"SatTrainer: an LDA matrix of {self.lda_mat.shape[0]} rows for a previous model of dimension {dim}")
        if dim > limit:
            raise ValueError(f"SatTrainer: feature dimension {dim} above {limit} (the GMM statistics' feature dimension)")
        if self.lda_mat is None and dim > FMLLR_MAX_DIM:
            raise ValueError(f"SatTrainer: Δ+ΔΔ features of dimension {dim} above {FMLLR_MAX_DIM} (the fMLLR statistics' on that path)")
        self.backend = backend if backend is not None else SatDeviceBackend(utterances, lexicon, self.opt, self.mfcc_options,
                                                                             self.silence_phones, device, engine, self.lda_mat)
        self.initial_gaussians = self.raw_am.num_pdfs           # until the tree is built
        self.final_gaussian_iteration = self.num_iterations - 10
        self.realignment_iterations = list(range(10, self.num_iterations, 10))
        self.current_gaussians = self.initial_gaussians
        self.rng = np.random.default_rng(self.seed)
        self.history: List[Dict] = []
        self.initial_stats: Optional[GmmStats] = None
        self.tree_stats = None
        self.tree_record: Optional[Dict] = None
        self.ali_raw_tm = self.ali_raw_am = None
        self.alimdl_stats: Optional[GmmStats] = None
        self.history_alimdl: Optional[Dict] = None
        self.iteration = 0

    @property
    def transforms(self) -> Optional[np.ndarray]:
        return self.backend.transforms

    @property
    def speakers(self) -> List[str]:
        return self.backend.speakers

    @property
    def fmllr_steps(self) -> List[np.ndarray]:
        return self.backend.steps

    def train(self) -> "SatTrainer":
        b = self.backend
        prev_tm, prev_am, prev_tree = self.previous
        self.iteration = 0
        failed = b.align_previous(prev_tm, prev_am, prev_tree, self.lda_mat, self.opt.beam, self.previous_transforms)
        fmllr = None if self.previous_transforms is not None else b.estimate_transforms(prev_tm, prev_am)
        self.raw_tm, self.raw_am, self.tree, info = tree_stage(b, prev_tm, prev_tm.topo, self.roots, self.shared_phones,
                                                               self.silence_phones, self.extra_questions, self.num_leaves,
                                                               self.cluster_threshold)
        self.tree_stats, self.tree_record = info.pop("tree_stats"), info.pop("tree_record")
        self.initial_gaussians = self.current_gaussians = self.raw_am.num_pdfs
        stats = b.accumulate(self.raw_tm, self.raw_am)
        self.initial_stats = stats.copy()
        self._update(stats, failed, True, min_gaussian_occupancy=self.min_gaussian_occupancy)
        self.history[-1].update(info)
        if fmllr is not None:
            self.history[-1]["fmllr"] = fmllr
        self._iterate(failed, self.opt.beam)
        self.finalize_training()
        return self

    def _before_statistics(self, iteration: int) -> Optional[Dict]:
        if iteration not in self.fmllr_iterations:
            return None
        return dict(fmllr=self.backend.estimate_transforms(self.raw_tm, self.raw_am))

    def finalize_training(self) -> None:
        """The alignment model: two-feature statistics of the resident batches under the final model → ``alignment_model``."""
        st = self.backend.accumulate_two_feats(self.raw_tm, self.raw_am)
        self.ali_raw_tm, self.ali_raw_am, updated, floored = _alignment_model(self.raw_tm, self.raw_am, st)
        self.alimdl_stats = st
        self.history_alimdl = dict(loglike=st.loglike_per_frame, frames=st.tot_count, updated=updated, floored=floored)

    def write(self, directory) -> List[Path]:
        """``final.mdl``, ``tree``, ``final.alimdl`` (``ali_raw_tm`` + ``ali_raw_am``) and, with an LDA, ``lda.mat``."""
        if self.ali_raw_am is None:
            raise ValueError("SatTrainer.write: train has not been run")
        files = super().write(directory)
        out = Path(directory)
        with open(out / "final.alimdl", "wb") as f:
            kaldi_io.write_model(f, self.ali_raw_tm, self.ali_raw_am)
        files.append(out / "final.alimdl")
        if self.lda_mat is not None:
            with open(out / "lda.mat", "wb") as f:
                f.write(b"\0B")
                kaldi_io.write_matrix(f, self.lda_mat)
            files.append(out / "lda.mat")
        return files

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the trained pair (on the training engine when the device backend ran): ``final.mdl``,
        ``ali_am=`` / ``raw_ali_am=`` the alignment model, ``lda=`` when there is one.  Both passes run on ``final.mdl``'s
        transition model, as ``CorpusAligner`` does for any SAT model: ``ali_raw_tm`` is written to ``final.alimdl`` and not
        used here."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             lda=self.lda_mat, ali_am=DiagGmmModel.from_raw(self.ali_raw_am), mfcc_options=self.mfcc_options,
                             silence_phones=self.silence_phones, raw_tm=self.raw_tm, raw_am=self.raw_am,
                             raw_ali_am=self.ali_raw_am, **kw)


# ---- the pronunciation-probability stage ------------------------------------------------------------------------------------------
class PronunciationDeviceBackend:
    """``PronunciationProbabilityTrainer``'s one call on the device: ``CorpusAligner.pronunciation_statistics`` with the
    previous stage's model — one pass, or with ``speaker_adapted`` the alignment model's pass, fMLLR and a second pass."""

    def __init__(self, utterances, lexicon, options=None, mfcc_options: Optional[dict] = None, silence_phones: Sequence[int] = (),
                 device: int = 0, engine=None):
        from .aligner import AlignOptions

        self.utts = list(utterances)
        self.lexicon, self.opt = lexicon, options or AlignOptions()
        self.mfcc_options, self.silence_phones = dict(mfcc_options or {}), list(silence_phones)
        self.device, self.engine = device, engine
        self.al = None

    def pronunciation_counts(self, raw_tm, raw_am, tree, lda, ali_raw_am, speaker_adapted: bool):
        """(``pronprob.PronunciationCounts`` of the corpus, utterances without an alignment)."""
        from .aligner import CorpusAligner

        self.al = CorpusAligner(TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am), tree, self.lexicon, lda=lda,
                                options=self.opt, device=self.device, engine=self.engine, mfcc_options=self.mfcc_options,
                                silence_phones=self.silence_phones, raw_tm=raw_tm, raw_am=raw_am,
                                ali_am=None if ali_raw_am is None else DiagGmmModel.from_raw(ali_raw_am), raw_ali_am=ali_raw_am)
        self.engine = self.al.engine
        counts = self.al.pronunciation_statistics(self.utts, speaker_adapted=speaker_adapted)
        return counts, len(self.al.failed)


class PronunciationProbabilityTrainer:
    """The reference's ``PronunciationProbabilityTrainer`` (MFA/acoustic_modeling/pronunciation_probabilities.py; the estimate
    in MFA/alignment/base.py:937-1176): no model is trained — the corpus is aligned with the previous stage's model, the
    aligned pronunciations and the silences around them are counted, and the lexicon is re-estimated from the counts.
    ``PronunciationProbabilityTrainer(previous, utterances, lexicon).train()`` then ``write(directory)``.

    ``previous``: a trained stage or ``(raw_tm, raw_am, tree)``.  From a stage its ``lda_mat``, its alignment model
    (``ali_raw_tm`` / ``ali_raw_am``) and its ``transforms`` are picked up (``previous_lda=`` / ``ali_model=(raw_tm, raw_am)``
    give the first two by hand); with an alignment model the alignment is the two-pass one (``speaker_adapted=`` overrides).

    ``train`` sets ``counts`` (``pronprob.PronunciationCounts``), ``lexicon`` (the re-estimated ``LexiconCompiler``; the one
    given stays as ``source_lexicon``), ``info`` (the four silence numbers) and ``failed``.  ``raw_tm`` / ``raw_am`` / ``tree``
    (and ``lda_mat``, ``transforms``) are the previous stage's, so that the stage can itself be a ``previous``:
    ``SatTrainer(utterances, lexicon=stage.lexicon, previous=stage)`` continues on graphs compiled from the new lexicon.
    ``write`` writes the model files of the previous stage (``final.mdl``, ``tree``, with them ``final.alimdl`` / ``lda.mat``
    when there are any), ``lexicon.dict`` and ``silence_probabilities.json``."""

    DICTIONARY, SILENCE_INFO = "lexicon.dict", "silence_probabilities.json"

    def __init__(self, previous=None, utterances=None, lexicon=None, previous_lda: Optional[np.ndarray] = None, ali_model=None,
                 speaker_adapted: Optional[bool] = None, align_options=None, silence_phones: Optional[Sequence[int]] = None,
                 mfcc_options: Optional[dict] = None, device: int = 0, engine=None, backend=None):
        if previous is None or lexicon is None:
            raise ValueError("PronunciationProbabilityTrainer needs a lexicon and the previous stage's (raw_tm, raw_am, tree)")
        self.source_lexicon, self.previous = lexicon, previous_models(previous)
        self.raw_tm, self.raw_am, self.tree = self.previous
        if previous_lda is None:
            previous_lda = getattr(previous, "lda_mat", None)
        self.lda_mat = None if previous_lda is None else np.asarray(previous_lda, dtype=np.float32)
        if ali_model is None and getattr(previous, "ali_raw_am", None) is not None:
            ali_model = (previous.ali_raw_tm, previous.ali_raw_am)
        self.ali_raw_tm, self.ali_raw_am = ali_model if ali_model is not None else (None, None)
        self.transforms = getattr(previous, "transforms", None)
        self.speaker_adapted = (self.ali_raw_am is not None) if speaker_adapted is None else bool(speaker_adapted)
        self.opt = align_options or getattr(previous, "opt", None)
        self.silence_phones = list(getattr(previous, "silence_phones", ()) if silence_phones is None else silence_phones)
        self.mfcc_options = dict(getattr(previous, "mfcc_options", {}) if mfcc_options is None else mfcc_options)
        if engine is None:
            engine = getattr(getattr(previous, "backend", None), "engine", None)
        self.backend = backend if backend is not None else PronunciationDeviceBackend(utterances, lexicon, self.opt, self.mfcc_options,
                                                                                      self.silence_phones, device, engine)
        self.lexicon = None
        self.info: Optional[Dict] = None
        self.counts = None
        self.failed = 0

    def train(self) -> "PronunciationProbabilityTrainer":
        from . import pronprob

        self.counts, self.failed = self.backend.pronunciation_counts(self.raw_tm, self.raw_am, self.tree, self.lda_mat,
                                                                     self.ali_raw_am, self.speaker_adapted)
        if self.counts.utterances == 0:
            raise ValueError("PronunciationProbabilityTrainer: the previous model aligned no utterance")
        self.lexicon, self.info = pronprob.estimate(self.source_lexicon, self.counts)
        return self

    def write(self, directory) -> List[Path]:
        from . import pronprob

        if self.lexicon is None:
            raise ValueError("PronunciationProbabilityTrainer.write: train has not been run")
        out = Path(directory)
        files = GmmTrainerBase.write(self, out)
        if self.ali_raw_am is not None:
            with open(out / "final.alimdl", "wb") as f:
                kaldi_io.write_model(f, self.ali_raw_tm if self.ali_raw_tm is not None else self.raw_tm, self.ali_raw_am)
            files.append(out / "final.alimdl")
        if self.lda_mat is not None:
            with open(out / "lda.mat", "wb") as f:
                f.write(b"\0B")
                kaldi_io.write_matrix(f, self.lda_mat)
            files.append(out / "lda.mat")
        files.append(pronprob.write_dictionary(out / self.DICTIONARY, self.lexicon))
        files.append(pronprob.write_silence_info(out / self.SILENCE_INFO, self.info))
        return files

    def aligner(self, **kw):
        """A ``CorpusAligner`` on the previous stage's model and the re-estimated lexicon (on the training engine when the
        device backend ran)."""
        from .aligner import CorpusAligner

        kw.setdefault("engine", getattr(self.backend, "engine", None))
        if self.opt is not None:
            kw.setdefault("options", self.opt)
        return CorpusAligner(TransitionModel(self.raw_tm), DiagGmmModel.from_raw(self.raw_am), self.tree, self.lexicon,
                             lda=self.lda_mat, ali_am=None if self.ali_raw_am is None else DiagGmmModel.from_raw(self.ali_raw_am),
                             mfcc_options=self.mfcc_options, silence_phones=self.silence_phones, raw_tm=self.raw_tm,
                             raw_am=self.raw_am, raw_ali_am=self.ali_raw_am, **kw)
