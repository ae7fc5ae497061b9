"""Pronunciation-probability training: counts from alignments, a lexicon with probabilities out.

Reference boundary: ``GeneratePronunciationsFunction._process_pronunciations`` (MFA/alignment/multiprocessing.py:1476-1510) is
the counter, ``compute_pronunciation_probabilities`` (MFA/alignment/base.py:937-1176) the estimate, ``format_probability`` /
``format_correction`` (MFA/helper.py:934-944) the rounding; ``DictionaryTrainer.export_lexicons``
(MFA/alignment/pretrained.py:561-613) and ``PronunciationProbabilityTrainer`` (MFA/acoustic_modeling/
pronunciation_probabilities.py) are the two users.  Everything here is host code: the stage's device work is the alignment pass
(``CorpusAligner.pronunciation_statistics``), the counting runs over the interval arrays the native extractor hands back, and
the tables are lexicon-sized.

Keys.  A pronunciation is a key: the lexicon's records in lexicon order (``lexicon.pronunciations[k]``, i.e. a word id and the
variant's position among the word's records), then four keys of their own — the silence word, the out-of-vocabulary word (the
aligner spells it with the OOV phone whatever the dictionary says), ``<s>`` and ``</s>``.

  ``count_from_ctm``        the specification: the reference's loop, token by token, over ``HierarchicalCtm.word_intervals``
  ``count_from_intervals``  the same tables from ``IntervalBatch`` arrays: shifts, ``bincount`` and ``unique`` on packed keys
  ``estimate``              counts → a new ``LexiconCompiler`` and the four silence numbers its constructor takes
  ``write_dictionary`` / ``write_silence_info``   the files ``load_pronunciations`` / ``LexiconCompiler(**json)`` read

Not here: cutoff, laughter and bracketed word models, phonological rules, several dictionaries per corpus, the
``for_g2p`` branch.
"""
from __future__ import annotations

import dataclasses
import inspect
import json
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import graph as _graph

LAMBDA_2 = 2          # smoothing of the silence-after probability (towards silence_probability)
LAMBDA_3 = 2          # smoothing of the before-corrections (towards 1)
BOS_SILENCE_AFTER = 1        # hundredths: the 0.01 the reference's expected counts use for "<s>" (quirk 1, see ``estimate``)

SILENCE_INFO_KEYS = ("silence_probability", "initial_silence_probability", "final_silence_correction",
                     "final_non_silence_correction")


def format_probability(value: float) -> float:
    """MFA/helper.py:934-936: two decimals by Python's ``round`` (``np.round`` is another function), inside [0.01, 0.99]."""
    return min(max(round(value, 2), 0.01), 0.99)


def format_correction(value: float) -> float:
    """MFA/helper.py:939-944: two decimals, 0.01 when that is not positive; no upper clamp."""
    value = round(value, 2)
    return 0.01 if value <= 0 else value


class PronunciationIndex:
    """Keys of a lexicon's pronunciations.  ``n_records`` record keys in lexicon order, then ``sil``, ``oov``, ``bos``,
    ``eos``; ``word_id[k]`` / ``variant[k]`` name a record key as (word id, position among the word's records)."""

    def __init__(self, lexicon: _graph.LexiconCompiler):
        self.lexicon = lexicon
        recs = lexicon.pronunciations
        self.n_records = len(recs)
        self.sil, self.oov, self.bos, self.eos = (self.n_records + i for i in range(4))
        self.n_keys = self.n_records + 4
        self.sil_word = int(lexicon.word_table.find(lexicon.silence_word))
        self.oov_word = int(lexicon.word_table.find(lexicon.oov_word))
        self.word_id = np.zeros(self.n_records, dtype=np.int64)
        self.variant = np.zeros(self.n_records, dtype=np.int64)
        self._by_text: Dict[Tuple[int, str], int] = {}
        self._table: Optional[tuple] = None
        seen: Dict[int, int] = {}
        for k, p in enumerate(recs):
            w = int(lexicon.word_table.find(p.orthography))
            self.word_id[k], self.variant[k] = w, seen.get(w, 0)
            seen[w] = seen.get(w, 0) + 1
            self._by_text[(w, " ".join(p.pronunciation.split()))] = k

    def key(self, word_id: int, pronunciation: str) -> int:
        """The key of one aligned word item (``WordCtmInterval.word_id`` / ``.pronunciation``)."""
        word_id = int(word_id)
        if word_id == self.sil_word:
            return self.sil
        if word_id == self.oov_word:
            return self.oov
        k = self._by_text.get((word_id, " ".join(pronunciation.split())))
        if k is None:
            raise KeyError(f"word id {word_id} has no pronunciation {pronunciation!r} in the lexicon")
        return k

    def variant_table(self, extractor) -> Tuple[np.ndarray, np.ndarray]:
        """(offset per word id, key per (word id, extractor variant)): ``IntervalBatch.it_var`` counts a word's variants in
        the extractor's order (longest first), not the lexicon's."""
        if self._table is None or self._table[0] is not extractor:          # (built once per extractor: lexicon-sized)
            off = np.zeros(len(extractor._var_text) + 1, dtype=np.int64)
            keys: List[int] = []
            for w, texts in enumerate(extractor._var_text):
                keys.extend(self.key(w, t) for t in texts)
                off[w + 1] = len(keys)
            self._table = (extractor, off, np.asarray(keys + [0], dtype=np.int64))
        return self._table[1], self._table[2]


class PronunciationCounts:
    """The counter's tables, additive like ``GmmStats``: per key ``count`` (tokens of the pronunciation; ``<s>`` / ``</s>``:
    utterances), ``silence_following`` / ``non_silence_following``, ``silence_before`` / ``non_silence_before`` (the silence
    word and ``</s>`` are keys of these two, as in the reference), and the pair table — ``pair_keys`` sorted unique int64
    ``left · n_keys + right`` with ``pair_counts[:, 0]`` silence between the two, ``[:, 1]`` none."""

    FIELDS = ("count", "silence_following", "non_silence_following", "silence_before", "non_silence_before")

    def __init__(self, n_keys: int):
        self.n_keys = int(n_keys)
        for f in self.FIELDS:
            setattr(self, f, np.zeros(self.n_keys, dtype=np.int64))
        self.pair_keys = np.zeros(0, dtype=np.int64)
        self.pair_counts = np.zeros((0, 2), dtype=np.int64)

    @classmethod
    def zeros(cls, n_keys: int) -> "PronunciationCounts":
        return cls(n_keys)

    def copy(self) -> "PronunciationCounts":
        out = PronunciationCounts(self.n_keys)
        out += self
        return out

    def set_pairs(self, packed: np.ndarray, column: np.ndarray) -> None:
        """The pair table from one packed key and one column (0 silence, 1 non-silence) per observed pair."""
        keys, inv = np.unique(np.asarray(packed, dtype=np.int64), return_inverse=True)
        counts = np.zeros((keys.shape[0], 2), dtype=np.int64)
        np.add.at(counts, (inv.reshape(-1), np.asarray(column, dtype=np.int64)), 1)
        self.pair_keys, self.pair_counts = keys, counts

    def __iadd__(self, other: "PronunciationCounts") -> "PronunciationCounts":
        if other.n_keys != self.n_keys:
            raise ValueError(f"counts over {other.n_keys} keys added to counts over {self.n_keys}")
        for f in self.FIELDS:
            getattr(self, f).__iadd__(getattr(other, f))
        keys, inv = np.unique(np.concatenate([self.pair_keys, other.pair_keys]), return_inverse=True)
        counts = np.zeros((keys.shape[0], 2), dtype=np.int64)
        np.add.at(counts, inv.reshape(-1), np.concatenate([self.pair_counts, other.pair_counts]))
        self.pair_keys, self.pair_counts = keys, counts
        return self

    def equals(self, other: "PronunciationCounts") -> bool:
        return (self.n_keys == other.n_keys and all(np.array_equal(getattr(self, f), getattr(other, f)) for f in self.FIELDS)
                and np.array_equal(self.pair_keys, other.pair_keys) and np.array_equal(self.pair_counts, other.pair_counts))

    @property
    def utterances(self) -> int:
        return int(self.count[self.n_keys - 2])          # one "<s>" per counted utterance

    def pairs(self) -> Dict[Tuple[int, int], Tuple[int, int]]:
        """{(left key, right key): (silence, non_silence)}."""
        return {(int(k) // self.n_keys, int(k) % self.n_keys): (int(c[0]), int(c[1]))
                for k, c in zip(self.pair_keys, self.pair_counts)}


# ---- the counter: specification --------------------------------------------------------------------------------------------
def count_from_ctm(lexicon: _graph.LexiconCompiler, ctms: Iterable, index: Optional[PronunciationIndex] = None) -> PronunciationCounts:
    """The reference's ``_process_pronunciations`` over every ``HierarchicalCtm`` of ``ctms`` (``None`` — an utterance
    without an alignment or whose interval stage failed — contributes nothing).  Items are told apart by their word id and
    their spelt pronunciation: ``fix_unk_words`` may have given an out-of-vocabulary item the transcript's label, which the
    reference's counter never sees."""
    ix = index or PronunciationIndex(lexicon)
    out = PronunciationCounts(ix.n_keys)
    packed: List[int] = []
    column: List[int] = []
    for ctm in ctms:
        if ctm is None:
            continue
        toks = [ix.bos] + [ix.key(w.word_id, w.pronunciation) for w in ctm.word_intervals] + [ix.eos]
        for i, k in enumerate(toks):
            if i != 0:                                     # "before" counts: from the token right before, silence included
                (out.silence_before if toks[i - 1] == ix.sil else out.non_silence_before)[k] += 1
            if k == ix.sil:
                continue
            out.count[k] += 1
            if i == len(toks) - 1:
                continue
            if toks[i + 1] == ix.sil:                      # "following": the next token; the pair skips that one silence
                out.silence_following[k] += 1
                packed.append(k * ix.n_keys + toks[i + 2])     # (after two silences in a row this is the second one)
                column.append(0)
            else:
                out.non_silence_following[k] += 1
                packed.append(k * ix.n_keys + toks[i + 1])
                column.append(1)
    out.set_pairs(np.asarray(packed, dtype=np.int64), np.asarray(column, dtype=np.int64))
    return out


# ---- the counter: fast path ------------------------------------------------------------------------------------------------
def count_from_intervals(extractor, batch, select: Optional[np.ndarray] = None,
                         index: Optional[PronunciationIndex] = None) -> PronunciationCounts:
    """``count_from_ctm``'s tables from a batch's interval arrays (``it_off`` / ``it_word`` / ``it_var`` / ``err``), numpy
    only.  Utterances with ``err != 0`` contribute nothing — they are the ones whose ``ctm`` is ``None`` —; ``select``
    (bool per utterance) leaves out more (an utterance whose result comes from another batch)."""
    ix = index or PronunciationIndex(extractor.lexicon)
    out = PronunciationCounts(ix.n_keys)
    n = batch.n_utt
    ok = np.asarray(batch.err[:n]) == 0
    if select is not None:
        ok &= np.asarray(select, dtype=bool)[:n]
    if not ok.any():
        return out
    it_off = np.asarray(batch.it_off, dtype=np.int64)
    n_items = np.diff(it_off)
    keep = np.repeat(ok, n_items)
    word, var = np.asarray(batch.it_word, dtype=np.int64)[keep], np.asarray(batch.it_var, dtype=np.int64)[keep]
    off, var_key = ix.variant_table(extractor)
    is_word = var >= 0
    items = np.where(is_word, var_key[np.where(is_word, off[word] + var, 0)], ix.sil)
    # the token stream of all counted utterances, "<s>" and "</s>" around each
    lens = n_items[ok] + 2
    ends = np.cumsum(lens)
    starts = ends - lens
    tok = np.empty(int(ends[-1]), dtype=np.int64)
    inner = np.ones(tok.shape[0], dtype=bool)
    inner[starts] = inner[ends - 1] = False
    tok[starts], tok[ends - 1], tok[inner] = ix.bos, ix.eos, items
    sil = tok == ix.sil
    nk = ix.n_keys

    def add(field: str, keys: np.ndarray) -> None:
        getattr(out, field).__iadd__(np.bincount(keys, minlength=nk))

    not_first = np.ones(tok.shape[0], dtype=bool)
    not_first[starts] = False
    prev_sil = np.concatenate([[False], sil[:-1]])
    add("silence_before", tok[not_first & prev_sil])
    add("non_silence_before", tok[not_first & ~prev_sil])
    add("count", tok[~sil])
    left = np.flatnonzero(~sil & (tok != ix.eos))          # every one has a successor in its own utterance
    nxt_sil = sil[left + 1]
    add("silence_following", tok[left[nxt_sil]])
    add("non_silence_following", tok[left[~nxt_sil]])
    # after a silence the utterance goes on ("</s>" at the latest), so left + 2 stays inside it
    right = np.where(nxt_sil, tok[np.minimum(left + 2, tok.shape[0] - 1)], tok[left + 1])
    out.set_pairs(tok[left] * nk + right, (~nxt_sil).astype(np.int64))
    return out


# ---- the estimate ----------------------------------------------------------------------------------------------------------
def copy_lexicon(lexicon: _graph.LexiconCompiler, records: Optional[Sequence[_graph.Pronunciation]] = None,
                 **keywords) -> _graph.LexiconCompiler:
    """A ``LexiconCompiler`` with ``lexicon``'s settings and tables (``keywords`` override constructor arguments) and copies
    of its records, or ``records`` in their place (same words, same order)."""
    kw = dict(disambiguation=lexicon.disambiguation, silence_probability=lexicon.silence_probability,
              initial_silence_probability=lexicon.initial_silence_probability,
              final_silence_correction=lexicon.final_silence_correction,
              final_non_silence_correction=lexicon.final_non_silence_correction, silence_word=lexicon.silence_word,
              oov_word=lexicon.oov_word, silence_phone=lexicon.silence_phone, oov_phone=lexicon.oov_phone,
              position_dependent_phones=lexicon.position_dependent_phones, ignore_case=lexicon.ignore_case,
              phones=sorted(lexicon.phones) if lexicon._fixed_inventory else None, share_suffixes=lexicon.share_suffixes)
    kw.update(keywords)
    new = _graph.LexiconCompiler(**kw)
    for p in (lexicon.pronunciations if records is None else records):
        new.add_pronunciation(dataclasses.replace(p))
    if len(new.pronunciations) != len(lexicon.pronunciations):
        raise ValueError("copy_lexicon: the records given are not the lexicon's")
    new.phones = set(lexicon.phones)
    new.word_table = _graph.SymbolTable()
    for k, s in lexicon.word_table:
        new.word_table.add_symbol(s, k)
    if lexicon.phone_table is not None:
        new.phone_table = _graph.SymbolTable()
        for k, s in lexicon.phone_table:
            new.phone_table.add_symbol(s, k)
    return new


def estimate(lexicon: _graph.LexiconCompiler, counts: PronunciationCounts,
             index: Optional[PronunciationIndex] = None) -> Tuple[_graph.LexiconCompiler, Dict[str, float]]:
    """``compute_pronunciation_probabilities`` for one dictionary: (a new lexicon — ``lexicon``'s words, tables and settings,
    the records of every word with a token in ``counts`` re-estimated, the others as they were — and ``info``, the four
    silence numbers under ``LexiconCompiler``'s constructor keywords, which the new lexicon carries).

    Probabilities enter later formulas as the two-decimal numbers ``format_probability`` made of them, so every quotient is
    formed here from integers in hundredths and divided once: the reference's floating-point sums, without their dependence
    on the order in which a dict happens to be walked.  Rounding is Python's ``round`` per value.

    The reference's quirks, kept:
      1. in the expected counts ``<s>`` as a left item has silence-after probability 0.01 (``silence_probabilities.get(w_p1,
         0.01)``: ``<s>`` is never given one), however often an utterance starts with silence;
      2. the worker-level ``final_silence_correction`` goes through ``format_probability``, not ``format_correction``: it
         cannot exceed 0.99 (``final_non_silence_correction`` is left unclamped);
      3. nothing precedes ``<s>``, so its "before" counts are zero and ``initial_silence_probability`` is the smoothing
         prior alone: it equals ``silence_probability``.
    One departure: the pronunciation probability itself is not capped at 0.99 (see below), so that the most frequent
    variant of a word stands at 1.00."""
    ix = index or PronunciationIndex(lexicon)
    if counts.n_keys != ix.n_keys:
        raise ValueError(f"counts over {counts.n_keys} keys for a lexicon of {ix.n_keys}")
    R = ix.n_records
    # words with a token in the counts; every record of such a word takes part (and gets the reference's +1)
    tokens_of_word = np.bincount(ix.word_id, weights=counts.count[:R], minlength=1) if R else np.zeros(1)
    seen = np.flatnonzero(tokens_of_word[ix.word_id] > 0) if R else np.zeros(0, dtype=np.int64)
    smoothed = counts.count[:R] + 1
    largest: Dict[int, int] = {}
    for k in seen.tolist():
        w = int(ix.word_id[k])
        largest[w] = max(largest.get(w, 0), int(smoothed[k]))

    sil_total, non_sil_total = int(counts.silence_before.sum()), int(counts.non_silence_before.sum())
    silence_probability = format_probability(sil_total / (sil_total + non_sil_total)) if sil_total + non_sil_total > 0 else 0.0
    sp100 = round(silence_probability * 100)

    def silence_after(k: int) -> float:
        sf, nsf = int(counts.silence_following[k]), int(counts.non_silence_following[k])
        return format_probability((100 * sf + sp100 * LAMBDA_2) / (100 * (sf + nsf + LAMBDA_2)))

    # expected counts over the pair table, in hundredths: Σ pairs · P(silence after the left item) for the right item
    after100 = np.zeros(ix.n_keys, dtype=np.int64)
    lefts = np.unique(counts.pair_keys // ix.n_keys)
    for k in lefts.tolist():
        after100[k] = round(silence_after(k) * 100)
    after100[ix.bos] = BOS_SILENCE_AFTER                                                  # quirk 1
    total = counts.pair_counts.sum(axis=1)
    p_left = after100[counts.pair_keys // ix.n_keys]
    right = counts.pair_keys % ix.n_keys
    bar_sil100, bar_non100 = np.zeros(ix.n_keys, dtype=np.int64), np.zeros(ix.n_keys, dtype=np.int64)
    np.add.at(bar_sil100, right, total * p_left)
    np.add.at(bar_non100, right, total * (100 - p_left))

    def corrections(k: int) -> Tuple[float, float]:
        s = 100 * (int(counts.silence_before[k]) + LAMBDA_3) / (int(bar_sil100[k]) + 100 * LAMBDA_3)
        ns = 100 * (int(counts.non_silence_before[k]) + LAMBDA_3) / (int(bar_non100[k]) + 100 * LAMBDA_3)
        return format_correction(s), format_correction(ns)

    records = [dataclasses.replace(p) for p in lexicon.pronunciations]
    for k in seen.tolist():
        p = records[k]
        # two decimals, at least 0.01 — and no cap at 0.99: a word's most frequent variant keeps 1.00 (cost 0 in the graph), as
        # Kaldi's max-normalised pronunciation probabilities do; the reference's format_probability would write 0.99 there
        p.probability = max(round(int(smoothed[k]) / largest[int(ix.word_id[k])], 2), 0.01)
        p.silence_after_probability = silence_after(k)
        p.silence_before_correction, p.non_silence_before_correction = corrections(k)

    initial_sil = int(counts.silence_before[ix.bos]) * 100 + sp100 * LAMBDA_2             # quirk 3: the counts are zero
    initial_non = int(counts.non_silence_before[ix.bos]) * 100 + (100 - sp100) * LAMBDA_2
    initial = format_probability(initial_sil / (initial_sil + initial_non)) if initial_sil + initial_non > 0 else 0.0
    final_sil, final_non = corrections(ix.eos)
    info = dict(silence_probability=format_probability(silence_probability),
                initial_silence_probability=format_probability(initial),
                final_silence_correction=format_probability(final_sil),               # quirk 2
                final_non_silence_correction=final_non)
    return copy_lexicon(lexicon, records, **info), info


# ---- files -----------------------------------------------------------------------------------------------------------------
_COLUMNS = ("probability", "silence_after_probability", "silence_before_correction", "non_silence_before_correction")


def write_dictionary(path, lexicon: _graph.LexiconCompiler) -> Path:
    """The MFA text dictionary ``LexiconCompiler.load_pronunciations`` reads: ``word  probability  silence-after
    silence-before-correction  non-silence-before-correction  phones``, tab separated; words sorted, a word's pronunciations in
    lexicon order.  A record without numbers is written without the columns; one with some of them only as far as they form
    a prefix the reader can tell (anything else is refused).  Numbers are written so that they read back as they are."""
    order = sorted(range(len(lexicon.pronunciations)), key=lambda k: lexicon.pronunciations[k].orthography)   # (stable)
    lines = []
    for k in order:
        p = lexicon.pronunciations[k]
        nums = [getattr(p, c) for c in _COLUMNS]
        n = next((i for i, v in enumerate(nums) if v is None), len(nums))
        if any(v is not None for v in nums[n:]):
            raise ValueError(f"write_dictionary: {p.orthography!r} has {_COLUMNS[n]} unset and a later column set")
        phones = p.pronunciation.split()
        if n < len(nums) and _graph._is_float(phones[0]):
            raise ValueError(f"write_dictionary: {p.orthography!r}: a phone named {phones[0]!r} would be read as a number")
        lines.append("\t".join([p.orthography] + [repr(float(v)) for v in nums[:n]] + [" ".join(phones)]))
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("".join(line + "\n" for line in lines), encoding="utf8")
    return path


def write_silence_info(path, info: Dict[str, float]) -> Path:
    """``info`` as JSON; its keys are ``LexiconCompiler`` constructor keywords (``LexiconCompiler(**json.load(f))``)."""
    known = set(inspect.signature(_graph.LexiconCompiler.__init__).parameters) - {"self"}
    unknown = sorted(set(info) - known)
    if unknown:
        raise ValueError(f"write_silence_info: {unknown} are not LexiconCompiler keywords")
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(dict(info), indent=2, sort_keys=True) + "\n", encoding="utf8")
    return path
