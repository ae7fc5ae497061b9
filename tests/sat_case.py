"""What tests/test_sat_cpu.py runs ``SatTrainer`` on: the 48-utterance corpus of tests/train_mono_case.py with a fixed
per-speaker distortion, and ``SatHostBackend`` — the host twins for the GMM statistics (one and two features) and the tree
statistics, the float64 fMLLR restatement of tests/test_fmllr_cpu.py (oracle/np_oracle.py ``fmllr_acc``) for the fMLLR
statistics, ``fmllr.estimate_fmllr`` for the solve, the oracle's aligner on the adapted features.  Test-side code.

The distortion.  The unadapted features are the oracle's Δ+ΔΔ features (MFCC → per-speaker CMVN → Δ+ΔΔ) put through a diagonal
affine map per speaker, y = s ⊙ x + o: scales s drawn once in [0.8, 1.25] (log-uniform), offsets o within ±0.5 of the column's
standard deviation over the corpus.  The generator's speakers differ little after CMVN; this gives speaker adaptation
something to undo.  Chosen on the CPU so that the conditions of tests/test_sat_cpu.py hold with room (figures in that file's
docstrings): the first fMLLR estimate gains more than a nat per frame, and on the unadapted features the alignment model
beats the speaker-adapted model by more than a nat per frame."""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Optional

import numpy as np

from montreal_forced_aligner_amd import fmllr as F
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import tree
from montreal_forced_aligner_amd.aligner import AlignOptions
from montreal_forced_aligner_amd.model import DiagGmmModel, TransitionModel, pdfs_of_phones
from montreal_forced_aligner_amd.stats import (GmmStats, gmm_statistics_host, gmm_statistics_twofeats_host, silence_weights, tid_tables,
                                               tree_statistics_host)
from oracle import np_oracle as N
from oracle import oracle as O
from tests import helpers
from tests import train_mono_case as TC

MIN_COUNT = 100.0          # the corpus has 46 speakers of one or two 3 s utterances


@lru_cache(maxsize=1)
def distorted_features():
    """(unadapted features per utterance, speaker names in first-appearance order, speaker row per utterance)."""
    corpus = TC.train_corpus()
    clean = corpus.features()
    names = list(dict.fromkeys(corpus.spk))
    rows = np.array([names.index(s) for s in corpus.spk], dtype=np.int32)
    rng = np.random.default_rng(4600)
    D = clean[0].shape[1]
    dev = np.concatenate(clean).std(axis=0)
    scale = np.exp(rng.uniform(np.log(0.8), np.log(1.25), size=(len(names), D)))
    offset = rng.uniform(-0.5, 0.5, size=(len(names), D)) * dev[None, :]
    return [(x * scale[r] + offset[r]).astype(np.float32) for x, r in zip(clean, rows)], names, rows


class SatHostBackend(TC.HostBackend):
    """``SatTrainer``'s calls on the host."""

    def __init__(self, corpus: TC.Corpus, opt: Optional[AlignOptions] = None):
        super().__init__(corpus, opt or AlignOptions(boost_silence=1.0, fmllr_min_count=MIN_COUNT))
        self.unadapted, self.speakers, self.rows = distorted_features()
        self.all_unadapted = np.concatenate(self.unadapted)
        self.lda = None
        self.transforms: Optional[np.ndarray] = None
        self.steps: List[np.ndarray] = []
        self._adapt()

    def _adapt(self) -> None:
        """The resident features: the unadapted ones through ``transforms`` (none: as they are)."""
        if self.transforms is None:
            self.feats = list(self.unadapted)
        else:
            self.feats = [O.affine(x, self.transforms[r]) for x, r in zip(self.unadapted, self.rows)]
        self.all_feats = np.concatenate(self.feats)

    def _align_on(self, raw_tm, raw_am, tree_, beam: float) -> int:
        tm, am = TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am)
        if self.opt.boost_silence != 1.0:
            am.gconsts = am.gconsts.copy()
            am.boost_silence(self.opt.boost_silence, pdfs_of_phones(tm, TC.silence_ids()))
        gc = G.TrainingGraphCompiler(tm, tree_, self.corpus.world.lexicon)
        scaled = tm.scaled_log_probs(self.opt.transition_scale, self.opt.self_loop_scale)
        failed, self.ali = 0, []
        for text, x in zip(self.corpus.text, self.feats):
            fst = G.add_transition_probs(gc.compile_fst(text), scaled)
            r = helpers.oracle_align_feats(tm, fst, x, am, self.opt.acoustic_scale, beam, self.opt.retry_beam)
            ok = r["status"] in (0, 1)
            failed += not ok
            self.ali.append(np.asarray(r["ali"], dtype=np.int32) if ok else np.zeros(x.shape[0], np.int32))
        return failed

    def align_previous(self, raw_tm, raw_am, tree_, previous_lda, beam: float, previous_transforms=None) -> int:
        assert previous_lda is None
        n, D = len(self.speakers), self.dim
        self.transforms = (np.tile(np.eye(D, D + 1, dtype=np.float32), (n, 1, 1)) if previous_transforms is None
                           else np.array(previous_transforms, dtype=np.float32))
        self.steps = []
        self._adapt()
        return self._align_on(raw_tm, raw_am, tree_, beam)

    def align(self, raw_tm, raw_am, tree_, beam: float) -> int:
        return self._align_on(raw_tm, raw_am, tree_, beam)

    def fmllr_stats(self, raw_tm, raw_am):
        """Per speaker (β, K, G) of the resident adapted features and alignments, in float64."""
        tm, am = TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am)
        id2pdf, w = tid_tables(tm, silence_weights(tm, TC.silence_ids(), self.opt.silence_weight))
        out = []
        for s in range(len(self.speakers)):
            mine = np.flatnonzero(self.rows == s)
            x = np.concatenate([self.feats[u] for u in mine])
            a = np.concatenate([self.ali[u] for u in mine])
            ok = a > 0
            pdf = np.where(ok, id2pdf[np.where(ok, a, 0)], -1).astype(np.int32)
            r = N.fmllr_acc(x, pdf, np.where(ok, w[np.where(ok, a, 0)], 0.0), am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
            out.append((float(r["beta"]), r["K"], r["G"]))
        return out

    def estimate_transforms(self, raw_tm, raw_am) -> Dict:
        n, D = len(self.speakers), self.dim
        step = np.tile(np.eye(D, D + 1, dtype=np.float32), (n, 1, 1))
        rejected, impr, frames, done, gains = [], 0.0, 0.0, 0, []
        for s, (beta, K, Gs) in enumerate(self.fmllr_stats(raw_tm, raw_am)):
            step[s], gain, why = F.estimate_fmllr(beta, K, Gs, min_count=self.opt.fmllr_min_count)
            if why is not None:
                rejected.append(self.speakers[s])
                continue
            gains.append(gain)
            done, impr, frames = done + 1, impr + gain, frames + beta
            self.transforms[s] = F.compose_transforms(step[s], self.transforms[s])
        self.steps.append(step)
        self.gains = getattr(self, "gains", []) + [gains]
        self._adapt()
        return dict(speakers=done, rejected=rejected, objf_impr_per_frame=impr / frames if frames else 0.0, frames=frames)

    def accumulate_two_feats(self, raw_tm, raw_am) -> GmmStats:
        return gmm_statistics_twofeats_host(DiagGmmModel.from_raw(raw_am), self.all_feats, self.all_unadapted, np.concatenate(self.ali),
                                            TransitionModel(raw_tm))

    def tree_accumulate(self, raw_tm, ci_phones):
        st, fe, skipped = tree_statistics_host(self.all_feats, self.frame_off, np.concatenate(self.ali), TransitionModel(raw_tm), ci_phones)
        self.tree_batch = (st, fe)
        return st, skipped

    def convert_alignments(self, old_raw_tm, raw_tm, raw_am, new_tree) -> None:
        st, fe = self.tree_batch
        old_tm, new_tm = TransitionModel(old_raw_tm), TransitionModel(raw_tm)
        new = tree.convert_alignments(tree.convert_table(old_tm, new_tm, new_tree, st), tree.local_of_tid(old_tm), fe, np.concatenate(self.ali))
        self.ali = [new[self.frame_off[k]: self.frame_off[k + 1]] for k in range(len(self.ali))]


@lru_cache(maxsize=1)
def mono_on_distorted():
    """A monophone model of 6 iterations trained on the unadapted (distorted) features: the SAT stage's ``previous``."""
    from montreal_forced_aligner_amd.train import MonophoneTrainer

    corpus = TC.train_corpus()
    b = SatHostBackend(corpus, AlignOptions(boost_silence=1.25))
    return MonophoneTrainer(lexicon=corpus.world.lexicon, topology=TC.topology(), backend=b, silence_phones=TC.silence_ids(),
                            num_iterations=6, max_gaussians=208).train()
