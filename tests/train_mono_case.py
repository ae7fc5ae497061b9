"""What tests/test_train_mono_cpu.py and tests/test_gpu_train_mono.py share: the 48-utterance synthetic corpus, the host
backend of ``MonophoneTrainer`` (the twins: mfa_debug_align_equal_host, gmm_statistics_host, the oracle's aligner on the
oracle's features), and the measures — the EM check on a ``history``, the share of frames on the right phone, the phone
boundary error against the generator's segmentation.  Test-side code: the package imports nothing from here or from oracle/."""
from __future__ import annotations

from functools import lru_cache
from typing import List, Optional

import numpy as np

import synth_workload as S
from montreal_forced_aligner_amd import equal_align as E
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusUtterance
from montreal_forced_aligner_amd.model import DiagGmmModel, TransitionModel, pdfs_of_phones
from montreal_forced_aligner_amd.stats import GmmStats, gmm_statistics_host
from oracle import oracle as O
from tests import helpers

N_TRAIN, N_HELD_OUT = 48, 16
FIRST_TRAIN, FIRST_HELD_OUT = 1_000_000, 2_000_000
SAMPLES, N_WORDS = 48000, 8
U64 = 2.0 ** -53


class Corpus:
    def __init__(self, world: S.SynthWorld, first: int, n: int):
        self.world = world
        self.pcm, self.text, self.segs, self.spk = [], [], [], []
        for i in range(n):
            pcm, text, segs, spk = world.utterance(first + i, n_words=N_WORDS, samples=SAMPLES)
            self.pcm.append(pcm); self.text.append(text); self.segs.append(segs); self.spk.append(spk)

    def utterances(self) -> List[CorpusUtterance]:
        return [CorpusUtterance(f"utt{i:03d}", f"spk{s}", p, t) for i, (p, t, s) in enumerate(zip(self.pcm, self.text, self.spk))]

    @lru_cache(maxsize=None)
    def features(self) -> List[np.ndarray]:
        """MFCC → per-speaker CMVN → Δ+ΔΔ by the oracle: what the device pipeline computes."""
        mf = [O.mfcc(p.astype(np.float32), O.default_mfcc_opts()) for p in self.pcm]
        out: List[Optional[np.ndarray]] = [None] * len(mf)
        for s in dict.fromkeys(self.spk):
            mine = [i for i, v in enumerate(self.spk) if v == s]
            st = O.cmvn_stats([mf[i] for i in mine])
            for i in mine:
                out[i] = O.deltas(O.cmvn_apply(st, mf[i]))
        return out


@lru_cache(maxsize=1)
def world() -> S.SynthWorld:
    return S.SynthWorld.build()


@lru_cache(maxsize=1)
def train_corpus() -> Corpus:
    return Corpus(world(), FIRST_TRAIN, N_TRAIN)


@lru_cache(maxsize=1)
def held_out_corpus() -> Corpus:
    return Corpus(world(), FIRST_HELD_OUT, N_HELD_OUT)


def topology():
    pt = world().lexicon.phone_table
    ids = [k for k, s in pt if s != "<eps>"]
    return S._topology(max(ids), silence_ids())


def silence_ids() -> List[int]:
    pt = world().lexicon.phone_table
    return [pt.find("sil"), pt.find("spn")]


def host_align(corpus: Corpus, raw_tm, raw_am, tree, opt: AlignOptions, beam: Optional[float] = None):
    """The oracle's aligner over a corpus: per utterance the transition-ids, or None where it failed."""
    tm = TransitionModel(raw_tm)
    am = DiagGmmModel.from_raw(raw_am)
    if opt.boost_silence != 1.0:
        am.gconsts = am.gconsts.copy()
        am.boost_silence(opt.boost_silence, pdfs_of_phones(tm, silence_ids()))
    gc = G.TrainingGraphCompiler(tm, tree, corpus.world.lexicon)
    scaled = tm.scaled_log_probs(opt.transition_scale, opt.self_loop_scale)
    out = []
    for text, x in zip(corpus.text, corpus.features()):
        fst = G.add_transition_probs(gc.compile_fst(text), scaled)
        r = helpers.oracle_align_feats(tm, fst, x, am, opt.acoustic_scale, opt.beam if beam is None else beam, opt.retry_beam)
        out.append(np.asarray(r["ali"], dtype=np.int32) if r["status"] in (0, 1) else None)
    return out


class HostBackend:
    """``MonophoneTrainer``'s three calls on the host twins."""

    def __init__(self, corpus: Corpus, opt: Optional[AlignOptions] = None):
        self.corpus, self.opt = corpus, opt or AlignOptions(boost_silence=1.25)
        self.feats = corpus.features()
        self.dim = int(self.feats[0].shape[1])
        self.frame_off = np.concatenate([[0], np.cumsum([x.shape[0] for x in self.feats])]).astype(np.int64)
        self.all_feats = np.concatenate(self.feats)
        self.ali: List[np.ndarray] = []

    def equal_align(self, raw_tm, raw_am, tree, seed: int) -> int:
        tm = TransitionModel(raw_tm)
        gc = G.TrainingGraphCompiler(tm, tree, self.corpus.world.lexicon)
        fsts = [gc.compile_fst(t) for t in self.corpus.text]
        ali, status = E.equal_align_host(fsts, self.frame_off, np.arange(len(fsts), dtype=np.uint32), seed)
        self.ali = [ali[self.frame_off[k]: self.frame_off[k + 1]] for k in range(len(fsts))]
        return int((status != 0).sum())

    def align(self, raw_tm, raw_am, tree, beam: float) -> int:
        got = host_align(self.corpus, raw_tm, raw_am, tree, self.opt, beam)
        self.ali = [a if a is not None else np.zeros(x.shape[0], np.int32) for a, x in zip(got, self.feats)]
        return sum(a is None for a in got)

    def accumulate(self, raw_tm, raw_am) -> GmmStats:
        return gmm_statistics_host(DiagGmmModel.from_raw(raw_am), self.all_feats, np.concatenate(self.ali), TransitionModel(raw_tm))

    def alignments(self) -> List[np.ndarray]:
        return list(self.ali)


# ---- measures ---------------------------------------------------------------------------------------------------------------
def em_violations(history, bound_scale: float = 1.0):
    """Iterations at which EM guarantees that the average log-likelihood per frame did not fall, and those where it fell by
    more than the float64 summation bound of tests/gmm_acc_ref.py (two sums of T terms in two orders: 2·T·2⁻⁵³·Σ|terms| each;
    every frame's log-likelihood is negative here, so Σ|terms| = |total|).  An iteration i is checked when its predecessor
    neither realigned nor mixed up (the issue's rule), and when i itself did not realign and its predecessor did not mix up
    (statistics i − 1 and i are then of the same alignments, and model i − 1's update was a plain M-step)."""
    checked, bad = [], []
    for prev, cur in zip(history, history[1:]):
        rule = not prev["realigned"] and not prev["mixed_up"]
        same_alignments = not cur["realigned"] and not prev["mixed_up"]
        if not (rule or same_alignments):
            continue
        bound = bound_scale * 2 * U64 * (prev["frames"] * abs(prev["loglike"]) + cur["frames"] * abs(cur["loglike"]))
        checked.append(cur["iteration"])
        if cur["loglike"] < prev["loglike"] - bound:
            bad.append((cur["iteration"], prev["loglike"], cur["loglike"]))
    return checked, bad


def phone_share(corpus: Corpus, raw_tm, alignments) -> float:
    """Share of the corpus's frames whose aligned phone is the generator's (frames of failed utterances count as wrong)."""
    tm = TransitionModel(raw_tm)
    right = total = 0
    for segs, x, ali in zip(corpus.segs, corpus.features(), alignments):
        truth = np.array([p for p, _s in S.state_labels(corpus.world, segs, x.shape[0])])
        total += len(truth)
        if ali is not None and len(ali) == len(truth):
            right += int((tm.id2phone[np.asarray(ali)] == truth).sum())
    return right / total


def boundary_errors(corpus: Corpus, raw_tm, alignments, frame_shift: float = 0.01) -> np.ndarray:
    """|aligned − generated| begin and end times (seconds) of every non-silence phone, over the utterances whose aligned
    non-silence phone sequence is the generator's (another pronunciation variant, or a failure, leaves an utterance out)."""
    tm = TransitionModel(raw_tm)
    sil = set(silence_ids())
    pt = corpus.world.lexicon.phone_table
    errs = []
    for segs, ali in zip(corpus.segs, alignments):
        if ali is None or not np.all(np.asarray(ali) > 0):
            continue
        ali = np.asarray(ali)
        phones, ok = O.split_to_phones(ali, tm.id2state, tm.is_self_loop, tm.is_final, tm.tuples)     # (begin, frames, phone)
        if not ok:
            continue
        mine = [(int(p), int(a), int(a + n)) for a, n, p in phones if int(p) not in sil]
        truth = [(pt.find(p), a, b) for p, a, b in segs if pt.find(p) not in sil]
        if [m[0] for m in mine] != [t[0] for t in truth]:
            continue
        for (_p, a, b), (_q, ta, tb) in zip(mine, truth):
            errs += [abs(a * frame_shift - ta / S.SR), abs(b * frame_shift - tb / S.SR)]
    return np.asarray(errs)


class _Yardstick:
    """synth_workload.train_monophone's view of the training corpus: the same utterances, by index."""

    def __init__(self, corpus: Corpus):
        self.corpus, self.lexicon = corpus, corpus.world.lexicon

    def utterance(self, index: int):
        k = index - FIRST_TRAIN
        return self.corpus.pcm[k], self.corpus.text[k], self.corpus.segs[k], self.corpus.spk[k]


@lru_cache(maxsize=1)
def supervised_yardstick() -> S.SynthModel:
    """The supervised model of the same 48 utterances: one Gaussian per state from the generator's own labels."""
    corpus = train_corpus()
    feats = {id(p): x for p, x in zip(corpus.pcm, corpus.features())}
    return S.train_monophone(_Yardstick(corpus), lambda pcm, _spk: feats[id(pcm)], n_train=N_TRAIN, first_index=FIRST_TRAIN)
