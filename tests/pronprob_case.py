"""What tests/test_pronprob_cpu.py and tests/test_gpu_pronprob_flow.py share: a toy lexicon whose token streams go through
the real interval extractor, the translation between ``pronprob.PronunciationCounts`` and the restatement's dicts
(tests/pronprob_ref.py), the ground-truth token streams of the synthetic corpus, and the host backend of
``PronunciationProbabilityTrainer`` (the oracle's aligner, ctm.py, ``count_from_ctm``).  Test-side code."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from montreal_forced_aligner_amd import ctm as CTM
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import intervals_native as N
from montreal_forced_aligner_amd import pronprob as P
from tests import pronprob_ref as R

SIL = ("<eps>", "sil")
OOV = ("<unk>", "spn")


# ---- counts as the restatement's dicts -------------------------------------------------------------------------------------
def key_names(ix: P.PronunciationIndex) -> List[Tuple[str, str]]:
    lex = ix.lexicon
    names = [(p.orthography, " ".join(p.pronunciation.split())) for p in lex.pronunciations]
    return names + [(lex.silence_word, lex.silence_phone), (lex.oov_word, lex.oov_phone), R.BOS, R.EOS]


def as_dict(counts: P.PronunciationCounts, ix: P.PronunciationIndex) -> Dict[str, dict]:
    """``Tables.as_dict`` of the arrays."""
    names = key_names(ix)
    out = {}
    for theirs, mine in (("pron", "count"), ("sil_following", "silence_following"), ("non_sil_following", "non_silence_following"),
                         ("sil_before", "silence_before"), ("non_sil_before", "non_silence_before")):
        arr = getattr(counts, mine)
        out[theirs] = {names[k]: int(arr[k]) for k in np.flatnonzero(arr).tolist()}
    out["ngram"] = {(names[a], names[b]): v for (a, b), v in counts.pairs().items()}
    return out


def dictionary(lexicon) -> List[Tuple[str, str]]:
    return [(p.orthography, " ".join(p.pronunciation.split())) for p in lexicon.pronunciations]


def ctm_stream(lexicon, ctm) -> Optional[List[Tuple[str, str]]]:
    """The (word, pronunciation) stream the reference's counter reads off a ctm: the word-table name of the item's id (an
    out-of-vocabulary item is ``<unk>`` there, whatever label the transcript gave it afterwards)."""
    if ctm is None:
        return None
    return [(lexicon.word_table.find(int(w.word_id)), w.pronunciation) for w in ctm.word_intervals]


def records(lexicon) -> List[tuple]:
    return [(p.orthography, p.pronunciation, p.probability, p.silence_after_probability, p.silence_before_correction,
             p.non_silence_before_correction) for p in lexicon.pronunciations]


# ---- a toy lexicon and alignments made from token streams ------------------------------------------------------------------
class ToyTm:
    """One transition-state per phone, a forward-final and a self-loop transition-id each: enough for SplitToPhones."""

    def __init__(self, n_phones):
        self.num_transition_ids = 2 * n_phones
        self.id2state = np.zeros(2 * n_phones + 1, np.int32)
        self.id2phone = np.zeros(2 * n_phones + 1, np.int32)
        self.is_self_loop = np.zeros(2 * n_phones + 1, np.int32)
        self.is_final = np.zeros(2 * n_phones + 1, np.int32)
        for p in range(1, n_phones + 1):
            for k, tid in enumerate((2 * p - 1, 2 * p)):
                self.id2state[tid], self.id2phone[tid] = p, p
                self.is_final[tid], self.is_self_loop[tid] = int(k == 0), int(k == 1)


def toy_lexicon(n_words: int = 12) -> G.LexiconCompiler:
    """Word i spells itself with phones of its own (x{i}a, x{i}b, x{i}c), so a phone string has one reading: "x{i}a", for two
    words in three "x{i}a x{i}b" (listed AFTER the shorter one: the extractor's variant order is not the lexicon's), for one
    in four also "x{i}c x{i}a"."""
    lex = G.LexiconCompiler(position_dependent_phones=False, silence_phone="sil", oov_phone="spn")
    for i in range(n_words):
        lex.add_pronunciation(G.Pronunciation(f"w{i:02d}", f"x{i}a"))
        if i % 3 != 2:
            lex.add_pronunciation(G.Pronunciation(f"w{i:02d}", f"x{i}a x{i}b"))
        if i % 4 == 0:
            lex.add_pronunciation(G.Pronunciation(f"w{i:02d}", f"x{i}c x{i}a"))
    lex.build_phone_table()
    return lex


class ToyAligned:
    """Token streams — per utterance a list of (word, pronunciation), silences as ``SIL``, out-of-vocabulary items as
    (spelling, "spn") — turned into alignments of ``ToyTm`` and through ``IntervalExtractor.extract``.  ``status`` (per
    utterance, the decoder's) and ``scramble`` (utterances whose word ids are replaced by ones their phones do not spell)
    make utterances the interval stage reports.  ``batch``: the arrays; ``ctms``: the ``HierarchicalCtm`` per utterance,
    None where ``err != 0``; ``streams``: what the reference's counter would be handed, None likewise."""

    def __init__(self, lex, streams: Sequence[Sequence[Tuple[str, str]]], status: Optional[Sequence[int]] = None,
                 scramble: Sequence[int] = ()):
        pt = lex.phone_table
        self.lex = lex
        self.tm = ToyTm(max(k for k, _ in pt))
        self.ex = N.IntervalExtractor(self.tm, lex, 0.01)
        alis, word_ids, texts = [], [], []
        for u, stream in enumerate(streams):
            ali: List[int] = []
            ids: List[int] = []
            for word, pron in stream:
                for ph in pron.split():
                    p = pt.find(ph)
                    ali += [2 * p - 1, 2 * p, 2 * p]
                if (word, pron) != SIL:
                    ids.append(lex.to_int(word))
            if u in scramble:
                ids = [lex.to_int("w02")] * (len(ids) + 1)
            alis.append(np.asarray(ali, dtype=np.int32))
            word_ids.append(ids)
            texts.append(" ".join(w for w, p in stream if (w, p) != SIL))
        fo = np.concatenate([[0], np.cumsum([len(a) for a in alis])]).astype(np.int64)
        total = max(int(fo[-1]), 1)
        ali = np.zeros(total, np.int32)
        words = np.zeros(total, np.int32)
        for u, (a, ids) in enumerate(zip(alis, word_ids)):
            ali[fo[u]: fo[u + 1]] = a
            words[fo[u]: fo[u] + len(ids)] = ids[: len(a)]
        nw = np.array([min(len(ids), len(a)) for ids, a in zip(word_ids, alis)], dtype=np.int32)
        st = None if status is None else np.asarray(status, dtype=np.int32)
        self.batch = self.ex.extract(fo, ali, words, nw, st)
        self.err = self.batch.err[: len(streams)].copy()
        self.ctms = [self.batch.ctm(u, text=texts[u]) if self.err[u] == 0 else None for u in range(len(streams))]
        known = lambda w: lex.word_table.find(w) != -1          # noqa: E731
        self.streams = [[(w, p) if (w, p) == SIL or known(w) else (lex.oov_word, p) for w, p in s] if self.err[u] == 0 else None
                        for u, s in enumerate(streams)]


def random_streams(lex, n: int, seed: int) -> List[List[Tuple[str, str]]]:
    """``n`` token streams: 0–6 words (one in ten out of vocabulary), a silence at the start and after every word with
    probability 0.4, a second one right after it with probability 0.2; some streams are empty, some silence only."""
    rng = np.random.default_rng(seed)
    by_word: Dict[str, List[str]] = {}
    for p in lex.pronunciations:
        by_word.setdefault(p.orthography, []).append(p.pronunciation)
    names = sorted(by_word)
    out = []
    for _ in range(n):
        s: List[Tuple[str, str]] = []

        def maybe_silence():
            if rng.random() < 0.4:
                s.append(SIL)
                if rng.random() < 0.2:
                    s.append(SIL)

        maybe_silence()
        for _w in range(int(rng.integers(0, 7))):
            if rng.random() < 0.1:
                s.append((f"oov{int(rng.integers(0, 5))}", "spn"))
            else:
                w = names[int(rng.integers(0, len(names)))]
                s.append((w, by_word[w][int(rng.integers(0, len(by_word[w])))]))
            maybe_silence()
        out.append(s)
    return out


# ---- the synthetic corpus of tests/train_mono_case.py ----------------------------------------------------------------------
def truth_stream(lexicon, text: str, segs) -> List[Tuple[str, str]]:
    """The generator's token stream of one utterance from its segmentation: the transcript's words, each with the variant
    whose phones come next (the generator's own rule), a silence token wherever silence segments lie between (consecutive
    ones are one silence: the lexicon has one optional silence between two words)."""
    out: List[Tuple[str, str]] = []
    phones = [s[0] for s in segs]
    k = 0

    def silence():
        nonlocal k
        hit = False
        while k < len(phones) and phones[k] == "sil":
            k, hit = k + 1, True
        if hit:
            out.append(SIL)

    silence()
    for w in text.split():
        for pron in lexicon.word_pronunciations(w):
            ph = pron.pronunciation.split()
            if phones[k: k + len(ph)] == ph:
                out.append((w, pron.pronunciation))
                k += len(ph)
                break
        else:
            raise AssertionError(f"the segmentation does not spell {w!r}")
        silence()
    assert k == len(phones)
    return out


def word_tokens(stream) -> List[Tuple[Tuple[str, str], bool]]:
    """(word item, a silence follows it) for every word item of a stream."""
    return [(wp, i + 1 < len(stream) and stream[i + 1] == SIL) for i, wp in enumerate(stream) if wp != SIL]


def aligned_ctm(lexicon, tm, text: str, ali) -> Optional[CTM.HierarchicalCtm]:
    """ctm.py on one alignment of the transcript's words (the aligned words are the transcript's)."""
    if ali is None:
        return None
    ivs = CTM.generate_ctm(ali, tm, lexicon.phone_table, 0.01)
    h = CTM.phones_to_pronunciations(lexicon, [lexicon.to_int(w) for w in text.split()], ivs, text=text)
    h.word_intervals = CTM.fix_unk_words(text.split(), h.word_intervals, lexicon)
    return h


class HostBackend:
    """``PronunciationProbabilityTrainer``'s one call on the host: the oracle's aligner on the oracle's features
    (``train_mono_case.host_align``), ctm.py, ``count_from_ctm``."""

    def __init__(self, corpus, opt):
        self.corpus, self.opt = corpus, opt
        self.ctms: List[Optional[CTM.HierarchicalCtm]] = []

    def pronunciation_counts(self, raw_tm, raw_am, tree, lda, ali_raw_am, speaker_adapted):
        from montreal_forced_aligner_amd.model import TransitionModel
        from tests import train_mono_case as C

        assert lda is None and ali_raw_am is None and not speaker_adapted
        lex = self.corpus.world.lexicon
        tm = TransitionModel(raw_tm)
        alis = C.host_align(self.corpus, raw_tm, raw_am, tree, self.opt)
        self.ctms = [aligned_ctm(lex, tm, text, ali) for text, ali in zip(self.corpus.text, alis)]
        return P.count_from_ctm(lex, self.ctms), sum(a is None for a in alis)
