"""The trainers of the speaker path: the reference's ``DubmTrainer`` and ``IvectorTrainer`` (MFA/ivector/trainer.py) over the
device calls.  No alignments, no lexicon: features in, ``final.dubm`` / ``final.ie`` (and ``plda``) out.

Each stage drives the device through a backend of a few calls — ``load``, ``sample``, ``dense_statistics``, ``select`` and
``statistics`` for the UBM; ``prepare`` and ``estep`` on top of them for the extractor — so that the same loop runs on the host
twins in tests.  ``train`` re-exports the six classes.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import adapt as _adapt
from . import ivector as _iv
from . import kaldi_io
from . import plda as _plda
from . import ubm as _ubm
from .engine import AlignmentEngine
from .stats import (GmmStats, gaussian_selection, gaussian_selection_host, ivector_estep, ivector_estep_host,
                    ivector_utterance_statistics, ivector_utterance_statistics_host, prune_posteriors, prune_posteriors_host,
                    ubm_statistics, ubm_statistics_host)


# ---- diagonal UBM ------------------------------------------------------------------------------------------------------------
class UbmHostBackend:
    """The UBM stage's calls on the host twins (``stats.gaussian_selection_host``, ``stats.ubm_statistics_host``): features
    as numpy batches.  The device backend below has the same five calls."""

    def __init__(self, batch_frames: int = 500_000):
        self.batch_frames = int(batch_frames)
        self.keys: List[str] = []
        self.batches: List = []                 # feature matrices of about batch_frames frames each
        self.batch_keys: List[List[tuple]] = [] # per batch (key, first row, rows) of its utterances
        self.gselect: List = []                 # per batch, the selection of the last ``select``

    def _to_batch(self, mats):
        return np.ascontiguousarray(np.concatenate(mats), dtype=np.float32)

    def load(self, features) -> int:
        """(key, matrix) pairs — a ``FeatureArchive`` among them — cut into batches.  Returns the frames loaded."""
        self.batches, self.batch_keys, self.gselect, self.keys = [], [], [], []
        mats, keys, n = [], [], 0
        for key, m in features:
            m = np.asarray(m, dtype=np.float32)
            if m.shape[0] == 0:
                continue
            keys.append((key, n, m.shape[0])); mats.append(m); n += m.shape[0]
            self.keys.append(key)
            if n >= self.batch_frames:
                self.batches.append(self._to_batch(mats)); self.batch_keys.append(keys)
                mats, keys, n = [], [], 0
        if mats:
            self.batches.append(self._to_batch(mats)); self.batch_keys.append(keys)
        return self.num_frames

    @property
    def num_frames(self) -> int:
        return int(sum(b.shape[0] for b in self.batches))

    def _gather(self, batch, rows):
        return batch[rows]

    def sample(self, rows: np.ndarray):
        """Rows ``rows`` (ascending, over all batches) as one matrix of the backend's kind."""
        out, base = [], 0
        for b in self.batches:
            r = rows[(rows >= base) & (rows < base + b.shape[0])] - base
            if r.shape[0]:
                out.append(self._gather(b, r))
            base += b.shape[0]
        return self._concat(out)

    def _concat(self, parts):
        return np.concatenate(parts)

    def to_host(self, feats) -> np.ndarray:
        return np.asarray(feats)

    def dense_statistics(self, ubm, feats) -> GmmStats:
        return ubm_statistics_host(feats, ubm)

    def select(self, ubm, num_gselect: int):
        """Selects for every batch and keeps the result.  Returns (Σ frame log-likelihood, frames)."""
        self.gselect, tot = [], 0.0
        for b in self.batches:
            gs, ll = gaussian_selection_host(b, ubm, num_gselect)
            self.gselect.append(gs)
            tot += float(np.asarray(ll, dtype=np.float64).sum())
        return tot, self.num_frames

    def statistics(self, ubm) -> GmmStats:
        st = GmmStats.zeros(ubm.num_gauss, ubm.dim, 1)
        for b, gs in zip(self.batches, self.gselect):
            ubm_statistics_host(b, ubm, gs, into=st)
        return st

    def selections(self):
        """(key, int32 [frames, n]) per utterance, on the host: what a gselect archive holds."""
        for keys, gs in zip(self.batch_keys, self.gselect):
            g = self.to_host(gs)
            for key, a, n in keys:
                yield key, g[a: a + n]


class UbmDeviceBackend(UbmHostBackend):
    """The same calls on the device (mfa_ubm_gselect_batch, mfa_ubm_acc_batch): the batches, the sample and the selections
    are device tensors and stay there between the calls."""

    def __init__(self, device: int = 0, engine=None, batch_frames: int = 500_000):
        super().__init__(batch_frames)
        if engine is None:
            engine = AlignmentEngine(device)
        self.engine = engine

    def _to_batch(self, mats):
        return torch.from_numpy(super()._to_batch(mats)).to(self.engine.device)

    def _gather(self, batch, rows):
        return self.engine.gather_rows(batch, rows)

    def _concat(self, parts):
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def to_host(self, feats) -> np.ndarray:
        return feats.cpu().numpy()

    def dense_statistics(self, ubm, feats) -> GmmStats:
        return ubm_statistics(self.engine, feats, ubm)

    def select(self, ubm, num_gselect: int):
        self.gselect, tot = [], 0.0
        for b in self.batches:
            gs, ll = gaussian_selection(self.engine, b, ubm, num_gselect)
            self.gselect.append(gs)
            tot += float(ll.double().sum().item())
        return tot, self.num_frames

    def statistics(self, ubm) -> GmmStats:
        st = GmmStats.zeros(ubm.num_gauss, ubm.dim, 1)
        for b, gs in zip(self.batches, self.gselect):
            ubm_statistics(self.engine, b, ubm, gs, into=st)
        return st


class DubmTrainer:
    """The reference's ``DubmTrainer`` (MFA/ivector/trainer.py:105-388; Kaldi train_diag_ubm.sh) over the device calls.

      sample      ``num_frames`` frames of the features, drawn without replacement by a seeded numpy generator and gathered on
                  the device (``engine.gather_rows``); all frames when there are fewer.  The reference draws with reservoir
                  sampling on Python's ``random``: this draw is not that one.
      init        ``ubm.init_from_random_frames`` on the sample, then ``num_iterations_init`` rounds of dense statistics
                  (every Gaussian, no selection) → ``ubm.update`` → ``ubm.split`` along ``ubm.init_schedule(rule=)``
                  (gmm-global-init-from-feats); ``1.dubm``
      selection   once, with the initial model: every frame's ``num_gselect`` best Gaussians
      iterations  ``num_iterations`` rounds of statistics over all features on the selected Gaussians → ``ubm.update``, low-count
                  Gaussians removed on the last iteration only (trainer.py:340-345); ``<i + 1>.dubm``, at the end ``final.dubm``

    ``features``: (key, matrix) pairs; the reference's are ``FeatureArchive(feats_scp, vad_file_name=, subsample_n=subsample,
    use_sliding_cmvn=True)`` — what the speech-activity stage yields; ``subsample`` is kept for that call and not applied
    again here.  ``loglikes``: per training iteration, the average log-likelihood per frame under the model the iteration
    started from; ``init_loglikes`` the same for the init phase; ``select_loglike`` the selection's."""

    def __init__(self, num_iterations: int = 4, num_gselect: int = 30, subsample: int = 5, num_frames: int = 500000,
                 num_gaussians: int = 256, num_iterations_init: int = 20, initial_gaussian_proportion: float = 0.5,
                 min_gaussian_weight: float = 1e-4, remove_low_count_gaussians: bool = True, seed: int = 0,
                 schedule_rule: str = "kaldi", backend=None, device: int = 0, engine=None):
        self.num_iterations, self.num_gselect, self.subsample = int(num_iterations), int(num_gselect), int(subsample)
        self.num_frames, self.num_gaussians, self.num_iterations_init = int(num_frames), int(num_gaussians), int(num_iterations_init)
        self.initial_gaussian_proportion, self.min_gaussian_weight = float(initial_gaussian_proportion), float(min_gaussian_weight)
        self.remove_low_count_gaussians, self.seed, self.schedule_rule = bool(remove_low_count_gaussians), int(seed), schedule_rule
        self.backend = backend if backend is not None else UbmDeviceBackend(device, engine)
        self.ubm = None
        self.models: List = []                   # the model after the init phase and after every iteration
        self.init_loglikes: List[float] = []
        self.loglikes: List[float] = []
        self.select_loglike: Optional[float] = None
        self.on_statistics = None                # optional callback(iteration, model, statistics): tests compare backends here

    def feature_archive_options(self) -> Dict:
        """The keyword arguments of the ``FeatureArchive`` this stage reads in the reference."""
        return dict(subsample_n=self.subsample, use_sliding_cmvn=True)

    def initialize(self, features) -> None:
        be = self.backend
        total = be.load(features)
        if total == 0:
            raise ValueError("DubmTrainer: no feature frames")
        rng = np.random.default_rng(self.seed)
        rows = np.arange(total) if total <= self.num_frames else np.sort(rng.choice(total, size=self.num_frames, replace=False))
        sample = be.sample(rows)
        start, schedule = _ubm.init_schedule(self.num_gaussians, self.initial_gaussian_proportion, self.num_iterations_init,
                                             self.schedule_rule)
        self.ubm = _ubm.init_from_random_frames(be.to_host(sample), start, rng)
        self.init_loglikes = []
        for target in schedule:
            st = be.dense_statistics(self.ubm, sample)
            self.init_loglikes.append(st.loglike_per_frame)
            self.ubm = _ubm.update(self.ubm, st, True, _adapt.MIN_GAUSSIAN_WEIGHT)[0]    # MleDiagGmmOptions' defaults
            if target > self.ubm.num_gauss:
                self.ubm = _ubm.split(self.ubm, target, 0.1, rng)
        self.models = [self.ubm]
        tot, frames = be.select(self.ubm, self.num_gselect)
        self.select_loglike = tot / frames

    def train(self, features, directory=None) -> "DubmTrainer":
        self.initialize(features)
        self.loglikes = []
        for i in range(1, self.num_iterations + 1):
            st = self.backend.statistics(self.ubm)
            if self.on_statistics is not None:
                self.on_statistics(i, self.ubm, st)
            self.loglikes.append(st.loglike_per_frame)
            remove = self.remove_low_count_gaussians and i == self.num_iterations
            self.ubm = _ubm.update(self.ubm, st, remove, self.min_gaussian_weight)[0]
            self.models.append(self.ubm)
        if directory is not None:
            self.write(directory)
        return self

    def write(self, directory) -> List[Path]:
        """``1.dubm`` … ``<num_iterations + 1>.dubm`` and ``final.dubm``."""
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        out = []
        for i, m in enumerate(self.models, start=1):
            m.write(d / f"{i}.dubm"); out.append(d / f"{i}.dubm")
        self.ubm.write(d / "final.dubm")
        return out + [d / "final.dubm"]


# ---- i-vector extractor ------------------------------------------------------------------------------------------------------
class IvectorHostBackend(UbmHostBackend):
    """The i-vector stage's calls on the host twins: selection, posteriors, pruning and the utterance statistics once
    (``prepare``), then an E-step per iteration (``estep``) over the statistics it keeps.  The device backend below has the
    same calls."""

    def __init__(self, batch_frames: int = 500_000):
        super().__init__(batch_frames)
        self.utt_stats: List = []               # per batch (γ [U, G], X [U, G, D])
        self.S = None                           # global second-order statistics [G, D (D + 1) / 2]

    def _offsets(self, keys) -> np.ndarray:
        return np.array([0] + [a + n for _key, a, n in keys], dtype=np.int64)

    def _batch_stats(self, b, off, ubm, num_gselect, min_post, scale):
        gs, _ll = gaussian_selection_host(b, ubm, num_gselect)
        _st, post = ubm_statistics_host(b, ubm, gs, want_post=True)
        post = prune_posteriors_host(post, min_post, scale)
        gamma, X, self.S = ivector_utterance_statistics_host(b, off, gs, post, ubm.num_gauss, S=self.S, want_S=True)
        return gamma, X

    def prepare(self, ubm, num_gselect: int, min_post: float, scale: float) -> None:
        self.S, self.utt_stats = None, []
        for b, keys in zip(self.batches, self.batch_keys):
            self.utt_stats.append(self._batch_stats(b, self._offsets(keys), ubm, num_gselect, min_post, scale))

    def _estep(self, model, gamma, X, st):
        ivector_estep_host(model, gamma, X, into=st)

    def estep(self, model):
        st = _iv.IvectorStats.zeros(model.num_gauss, model.dim, model.ivector_dim)
        for gamma, X in self.utt_stats:
            self._estep(model, gamma, X, st)
        st.S = np.array(self.to_host(self.S), dtype=np.float64)
        return st


class IvectorDeviceBackend(IvectorHostBackend):
    """The same calls on the device (mfa_ubm_gselect_batch, mfa_ubm_acc_batch's posteriors, mfa_ivector_*): features, selections,
    posteriors and the utterance statistics are device tensors and stay there between the iterations."""

    def __init__(self, device: int = 0, engine=None, batch_frames: int = 500_000):
        super().__init__(batch_frames)
        if engine is None:
            engine = AlignmentEngine(device)
        self.engine = engine

    def _to_batch(self, mats):
        return torch.from_numpy(super()._to_batch(mats)).to(self.engine.device)

    def to_host(self, feats) -> np.ndarray:
        return feats.cpu().numpy()

    def _batch_stats(self, b, off, ubm, num_gselect, min_post, scale):
        gs, _ll = gaussian_selection(self.engine, b, ubm, num_gselect)
        _st, post = ubm_statistics(self.engine, b, ubm, gs, want_post=True)
        post = prune_posteriors(self.engine, post, min_post, scale, inplace=True)
        gamma, X, self.S = ivector_utterance_statistics(self.engine, b, off, gs, post, ubm.num_gauss, S=self.S, want_S=True)
        return gamma, X

    def _estep(self, model, gamma, X, st):
        ivector_estep(self.engine, model, gamma, X, into=st)


class IvectorTrainer:
    """The reference's ``IvectorTrainer`` (MFA/ivector/trainer.py:390-632; Kaldi train_ivector_extractor.sh) over the device
    calls, ``use_weights = False``.

      read        ``final.dubm`` (a path or a ``ubm.DiagUbm``); ``ivector.IvectorExtractorModel.from_diag_ubm`` with a seeded
                  numpy generator; ``1.ie``
      statistics  once: every frame's ``num_gselect`` best Gaussians, their softmax, gauss-to-post's pruning at ``min_post``
                  with scale ``posterior_scale · subsample`` (multiprocessing.py:174), then γ and X per utterance and the
                  global S — none depends on the extractor, so they stay resident
      iterations  ``num_iterations`` rounds of E-step → ``ivector.update``; ``<i + 1>.ie``, at the end ``final.ie``

    ``features``: (key, matrix) pairs, as ``DubmTrainer`` takes them.  ``objectives``: per iteration, ``ivector.objective`` of
    the model the iteration started from.  ``on_statistics(iteration, model, statistics)``: tests compare backends here."""

    def __init__(self, num_iterations: int = 10, subsample: int = 5, gaussian_min_count: float = 100, ivector_dimension: int = 192,
                 num_gselect: int = 20, min_post: float = 0.025, posterior_scale: float = 1.0, seed: int = 0, backend=None,
                 device: int = 0, engine=None, update_variances: bool = True):
        self.num_iterations, self.subsample, self.gaussian_min_count = int(num_iterations), int(subsample), float(gaussian_min_count)
        self.ivector_dimension, self.num_gselect, self.min_post = int(ivector_dimension), int(num_gselect), float(min_post)
        self.posterior_scale, self.seed, self.update_variances = float(posterior_scale), int(seed), bool(update_variances)
        self.backend = backend if backend is not None else IvectorDeviceBackend(device, engine)
        self.model = None
        self.models: List = []                   # the initial model and the one after every iteration
        self.objectives: List[float] = []
        self.update_counts: List[tuple] = []     # per iteration (Gaussians updated, skipped for their count, eigenvalues floored)
        self.on_statistics = None

    def feature_archive_options(self) -> Dict:
        return dict(subsample_n=self.subsample, use_sliding_cmvn=True)

    def initialize(self, features, dubm) -> None:
        ubm = dubm if isinstance(dubm, _ubm.DiagUbm) else _ubm.DiagUbm.read(dubm)
        if self.backend.load(features) == 0:
            raise ValueError("IvectorTrainer: no feature frames")
        self.ubm = ubm
        self.model = _iv.IvectorExtractorModel.from_diag_ubm(ubm, self.ivector_dimension, np.random.default_rng(self.seed))
        self.models = [self.model]
        self.backend.prepare(ubm, self.num_gselect, self.min_post, self.posterior_scale * self.subsample)

    def train(self, features, dubm, directory=None) -> "IvectorTrainer":
        self.initialize(features, dubm)
        self.objectives, self.update_counts = [], []
        for i in range(1, self.num_iterations + 1):
            st = self.backend.estep(self.model)
            if self.on_statistics is not None:
                self.on_statistics(i, self.model, st)
            self.objectives.append(_iv.objective(self.model, st))
            self.model, *counts = _iv.update(self.model, st, self.gaussian_min_count, self.update_variances)
            self.update_counts.append(tuple(counts))
            self.models.append(self.model)
        if directory is not None:
            self.write(directory)
        return self

    def write(self, directory) -> List[Path]:
        """``1.ie`` … ``<num_iterations + 1>.ie`` and ``final.ie``."""
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        out = []
        for i, m in enumerate(self.models, start=1):
            m.write(d / f"{i}.ie"); out.append(d / f"{i}.ie")
        self.model.write(d / "final.ie")
        return out + [d / "final.ie"]

    def compute_plda(self, ivectors, utt2spk, directory=None, minimum_utterance_count: int = 1, num_em_iters: int = 10):
        """The reference's ``compute_plda`` (MFA/corpus/ivector_corpus.py:196-283), where its ``IvectorTrainer`` ends: a PLDA
        model from the extracted i-vectors and their speakers (``plda.train_plda``: every vector length-normalised, a class per
        speaker, the reference's three refusals as ``plda.PldaTrainingError``), written as ``plda`` beside ``final.ie`` when a
        ``directory`` is given.  ``ivectors``: utterance → vector, or the vector ark ``export_ivectors`` wrote."""

        if isinstance(ivectors, (str, Path)):
            ivectors = dict(kaldi_io.read_ark(Path(ivectors).read_bytes(), "vector"))
        self.plda = _plda.train_plda(ivectors, utt2spk, minimum_utterance_count, num_em_iters)
        if directory is not None:
            d = Path(directory)
            d.mkdir(parents=True, exist_ok=True)
            self.plda.write(d / "plda")
        return self.plda
