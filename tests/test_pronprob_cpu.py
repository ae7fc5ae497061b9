"""Pronunciation-probability training on the host (montreal_forced_aligner_amd/pronprob.py and
``train.PronunciationProbabilityTrainer`` on a host backend): a corpus worked by hand, the specification against the
restatement of tests/pronprob_ref.py and the array path on random token streams that go through the real interval
extractor, additivity, the estimate's properties, the files, and the stage on the synthetic corpus of
tests/train_mono_case.py against the generator's own token streams."""
import json
import math

import numpy as np
import pytest

from montreal_forced_aligner_amd import adapt as A
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import pronprob as P
from montreal_forced_aligner_amd.aligner import AlignOptions
from montreal_forced_aligner_amd.train import PronunciationProbabilityTrainer
from tests import pronprob_case as PC
from tests import pronprob_ref as R

SIL, BOS, EOS = PC.SIL, R.BOS, R.EOS


# ---- a corpus worked by hand -----------------------------------------------------------------------------------------------
def _hand_lexicon():
    lex = G.LexiconCompiler(position_dependent_phones=False, silence_phone="sil", oov_phone="spn")
    lex.add_pronunciation(G.Pronunciation("a", "A1"))             # the extractor lists "A2 A3" first (longest first)
    lex.add_pronunciation(G.Pronunciation("a", "A2 A3"))
    lex.add_pronunciation(G.Pronunciation("b", "B"))
    lex.add_pronunciation(G.Pronunciation("d", "D", 0.5, 0.4, 1.1, 0.9))       # never spoken
    lex.build_phone_table()
    return lex


A1, A2, B = ("a", "A1"), ("a", "A2 A3"), ("b", "B")
HAND = [[SIL, A1, SIL, SIL, B],          # <s> sil a1 sil sil b </s>: initial silence, two silences in a row, no final silence
        [A2, B, SIL],                    # <s> a2 b sil </s>:         no initial silence, final silence
        [A1, B]]                         # <s> a1 b </s>:             no silence at all


def test_hand_worked_corpus():
    lex = _hand_lexicon()
    toy = PC.ToyAligned(lex, HAND)
    assert toy.err.tolist() == [0, 0, 0]
    ix = P.PronunciationIndex(lex)
    assert (ix.word_id[:4].tolist(), ix.variant[:4].tolist()) == ([2, 2, 3, 4], [0, 1, 0, 0])
    spec = P.count_from_ctm(lex, toy.ctms)
    fast = P.count_from_intervals(toy.ex, toy.batch)
    assert spec.equals(fast) and spec.utterances == 3
    # counted by hand, token by token ("before": the token right before; "following": the next one; after a silence the pair
    # is formed with the token after it — in the first stream that is the second silence)
    want = dict(
        pron={BOS: 3, EOS: 3, A1: 2, A2: 1, B: 3},
        sil_before={A1: 1, SIL: 1, B: 1, EOS: 1},                            # 4
        non_sil_before={SIL: 3, EOS: 2, A2: 1, B: 2, A1: 1},                 # 9
        sil_following={BOS: 1, A1: 1, B: 1},
        non_sil_following={BOS: 2, A2: 1, A1: 1, B: 2},
        ngram={(BOS, A1): (1, 1), (A1, SIL): (1, 0), (B, EOS): (1, 2), (BOS, A2): (0, 1), (A2, B): (0, 1), (A1, B): (0, 1)})
    assert PC.as_dict(spec, ix) == want
    assert R.count(toy.streams, lex.silence_word).as_dict() == want

    new, info = P.estimate(lex, spec)
    # silence_probability 4 / 13 = 0.3077 → 0.31
    # pronunciation probability (+1 each): a1 3/3 = 1.00, a2 2/3 = 0.67, b 4/4 = 1.00
    # silence after (sf + 0.31·2) / (sf + nsf + 2):  a1 1.62/4 = 0.405 → 0.41 (the double nearest 0.405 lies above it),
    #                                                a2 0.62/3 = 0.2067 → 0.21,  b 1.62/5 = 0.324 → 0.32
    # expected counts, "<s>" on the left at 0.01 (quirk 1; its own formula would give 1.62/5 = 0.32):
    #   a1 ← (<s>, a1)·2:              silence 0.02,               non-silence 1.98
    #   a2 ← (<s>, a2)·1:              silence 0.01,               non-silence 0.99
    #   b  ← (a2, b)·1 + (a1, b)·1:    silence 0.21 + 0.41 = 0.62, non-silence 0.79 + 0.59 = 1.38
    #   </s> ← (b, </s>)·3:            silence 0.96,               non-silence 2.04
    # corrections (count + 2) / (expected + 2):
    #   a1 3/2.02 = 1.485 → 1.49 and 3/3.98 = 0.754 → 0.75;  a2 2/2.01 = 0.995 → 1.0 and 3/2.99 = 1.003 → 1.0
    #   b  3/2.62 = 1.145 → 1.15 and 4/3.38 = 1.183 → 1.18
    #   </s> 3/2.96 = 1.0135 → 1.01, written through format_probability: 0.99 (quirk 2);  4/4.04 = 0.990 → 0.99
    # initial silence: nothing is counted before "<s>" → (0 + 0.62) / 2 = 0.31 (quirk 3), although one stream in three starts silent
    assert PC.records(new) == [("a", "A1", 1.0, 0.41, 1.49, 0.75), ("a", "A2 A3", 0.67, 0.21, 1.0, 1.0),
                               ("b", "B", 1.0, 0.32, 1.15, 1.18), ("d", "D", 0.5, 0.4, 1.1, 0.9)]
    assert info == dict(silence_probability=0.31, initial_silence_probability=0.31, final_silence_correction=0.99,
                        final_non_silence_correction=0.99)
    assert (new.silence_probability, new.initial_silence_probability, new.final_silence_correction,
            new.final_non_silence_correction) == (0.31, 0.31, 0.99, 0.99)
    assert PC.records(lex)[0] == ("a", "A1", None, None, None, None)          # the lexicon given is left as it was
    # without quirk 1 a1's silence-before correction would be 3 / (2·0.32 + 2) = 1.14: the 0.01 is what is pinned above

    # the lower clamps, by hand: one stream "a1" — no silence anywhere: 0 / 2 → 0.01; silence after a1 (0 + 0.02) / 3 → 0.01
    one = PC.ToyAligned(lex, [[A1]])
    new1, info1 = P.estimate(lex, P.count_from_intervals(one.ex, one.batch))
    # expected: a1 ← (<s>, a1): 0.01 / 0.99 → 2/2.01 → 1.0 and 3/2.99 → 1.0;  </s> ← (a1, </s>) at 0.01: the same;
    # a2 (the word was seen, this variant was not): 1/2 = 0.5, silence after 0.02/2 → 0.01, corrections 2/2 = 1.0
    assert PC.records(new1)[:2] == [("a", "A1", 1.0, 0.01, 1.0, 1.0), ("a", "A2 A3", 0.5, 0.01, 1.0, 1.0)]
    assert info1 == dict(silence_probability=0.01, initial_silence_probability=0.01, final_silence_correction=0.99,
                         final_non_silence_correction=1.0)


# ---- specification ≡ restatement ≡ array path ------------------------------------------------------------------------------
N_RANDOM = 300


@pytest.fixture(scope="module")
def random_case():
    lex = PC.toy_lexicon()
    streams = PC.random_streams(lex, N_RANDOM, seed=20)
    status = np.zeros(N_RANDOM, np.int32)
    status[[5, 77, 78, 200]] = 2                       # the decoder failed on these
    status[[9, 150]] = 1                               # (retried: fine)
    toy = PC.ToyAligned(lex, streams, status=status, scramble=(31, 120))
    return lex, streams, toy


def test_random_streams_three_ways(random_case):
    lex, streams, toy = random_case
    skipped = np.flatnonzero(toy.err != 0).tolist()
    assert set(skipped) >= {5, 77, 78, 200, 31, 120}
    empty = [u for u, s in enumerate(streams) if not s]
    assert empty and any(s and all(t == SIL for t in s) for s in streams)
    assert any(w.startswith("oov") for s in streams for w, _p in s)
    assert any(a == SIL and b == SIL for s in streams for a, b in zip(s, s[1:]))
    # an utterance without items is no error: it is "<s> </s>" on every path (one non-silence-before for "</s>")
    assert set(skipped) == {5, 77, 78, 200, 31, 120} and not set(empty) & set(skipped)
    ix = P.PronunciationIndex(lex)
    spec = P.count_from_ctm(lex, toy.ctms)
    fast = P.count_from_intervals(toy.ex, toy.batch)
    ref = R.count(toy.streams, lex.silence_word)
    assert spec.utterances == N_RANDOM - len(skipped)
    assert PC.as_dict(spec, ix) == ref.as_dict()
    for f in P.PronunciationCounts.FIELDS + ("pair_keys", "pair_counts"):
        assert np.array_equal(getattr(spec, f), getattr(fast, f)), f
        assert getattr(fast, f).dtype == np.int64
    assert np.all(np.diff(fast.pair_keys) > 0)
    # ``select`` leaves utterances out like ``err`` does
    keep = np.arange(N_RANDOM) % 3 != 0
    part = P.count_from_intervals(toy.ex, toy.batch, select=keep)
    assert part.equals(P.count_from_ctm(lex, [c if k else None for c, k in zip(toy.ctms, keep)]))


def test_counts_are_additive(random_case):
    lex, _streams, toy = random_case
    whole = P.count_from_ctm(lex, toy.ctms)
    half = N_RANDOM // 2
    first = np.arange(N_RANDOM) < half
    total = P.count_from_intervals(toy.ex, toy.batch, select=first)
    total += P.count_from_intervals(toy.ex, toy.batch, select=~first)
    assert total.equals(whole)
    two = P.count_from_ctm(lex, toy.ctms[:half])
    two += P.count_from_ctm(lex, toy.ctms[half:])
    assert two.equals(whole)
    empty = P.PronunciationCounts.zeros(whole.n_keys)
    empty += whole
    assert empty.equals(whole) and whole.copy().equals(whole)
    with pytest.raises(ValueError, match="keys"):
        empty += P.PronunciationCounts.zeros(whole.n_keys + 1)


# ---- the estimate ----------------------------------------------------------------------------------------------------------
def _hundredth(x):
    return abs(x * 100 - round(x * 100)) < 1e-9


def test_estimate_equals_restatement_and_keeps_its_properties(random_case):
    lex, _streams, toy = random_case
    lex = P.copy_lexicon(lex)
    lex.add_pronunciation(G.Pronunciation("unseen", "x0a x1a", 0.25, 0.6, 1.3, 0.8))
    lex.add_pronunciation(G.Pronunciation("bare", "x2a"))
    lex.word_table.add_symbol("unseen"); lex.word_table.add_symbol("bare")
    counts = P.count_from_ctm(lex, toy.ctms)
    new, info = P.estimate(lex, counts)
    want, want_info = R.estimate(R.count(toy.streams, lex.silence_word), PC.dictionary(lex), PC.OOV)
    got = {(r[0], r[1]): r[2:] for r in PC.records(new)}
    seen_words = {w for w, _p in want}
    assert len(seen_words) == 12
    assert {k: v for k, v in got.items() if k[0] in seen_words} == want and info == want_info
    # an unseen word is untouched — with numbers or without
    assert got[("unseen", "x0a x1a")] == (0.25, 0.6, 1.3, 0.8) and got[("bare", "x2a")] == (None, None, None, None)
    assert [p.orthography for p in new.pronunciations] == [p.orthography for p in lex.pronunciations]
    assert list(new.word_table) == list(lex.word_table) and list(new.phone_table) == list(lex.phone_table)
    # the most frequent variant of every seen word stands at 1.00; everything is a multiple of 0.01 inside its clamp
    ix = P.PronunciationIndex(lex)
    for w in seen_words:
        keys = [k for k in range(ix.n_records) if lex.pronunciations[k].orthography == w]
        top = max(keys, key=lambda k: counts.count[k])
        assert new.pronunciations[top].probability == 1.0
        for k in keys:
            p = new.pronunciations[k]
            assert 0.01 <= p.probability <= 1.0 and 0.01 <= p.silence_after_probability <= 0.99
            assert p.silence_before_correction >= 0.01 and p.non_silence_before_correction >= 0.01
            assert all(_hundredth(v) for v in (p.probability, p.silence_after_probability, p.silence_before_correction,
                                               p.non_silence_before_correction))
    assert all(_hundredth(v) for v in info.values())
    assert 0.01 <= info["silence_probability"] <= 0.99 and 0.01 <= info["initial_silence_probability"] <= 0.99
    assert 0.01 <= info["final_silence_correction"] <= 0.99 and info["final_non_silence_correction"] >= 0.01
    with pytest.raises(ValueError, match="keys"):
        P.estimate(PC.toy_lexicon(3), counts)


def test_silence_after_every_word_and_no_silence_at_all():
    """``silence_probability`` is Σ silence-before / Σ before over ALL keys, and a silence token is itself a key of those
    tables (the reference's rule): in "w sil w sil …" every silence is preceded by a word, which is one non-silence-before for
    every silence-before a word collects, and the quotient stays below one half however regular the silences are.  It reaches the
    0.99 clamp when next to every token is preceded by silence — silence after every word (and before it), in runs: 70
    silence items on either side of a word give 140 silence-before against 2 per utterance, 0.986 → 0.99.  No silence at
    all gives 0 → the 0.01 clamp."""
    lex = PC.toy_lexicon()
    words = [(p.orthography, p.pronunciation) for p in lex.pronunciations]
    plain = [[t for j in range(5) for t in (words[(7 * u + 3 * j) % len(words)], SIL)] for u in range(40)]
    toy = PC.ToyAligned(lex, plain)
    counts = P.count_from_intervals(toy.ex, toy.batch)
    assert int(counts.non_silence_following[: len(words)].sum()) == 0          # silence after every word
    new, info = P.estimate(lex, counts)
    assert info["silence_probability"] == 0.45         # per stream 5 silence-before (4 words, "</s>") of 11: 0.4545
    runs = [[SIL] * 70 + [words[u]] + [SIL] * 70 for u in range(5)]
    toy = PC.ToyAligned(lex, runs)
    assert toy.err.tolist() == [0] * 5
    counts = P.count_from_intervals(toy.ex, toy.batch)
    assert counts.equals(P.count_from_ctm(lex, toy.ctms))
    assert (int(counts.silence_before.sum()), int(counts.non_silence_before.sum())) == (5 * 140, 5 * 2)
    assert int(counts.non_silence_following[: len(words)].sum()) == 0          # silence after every word
    new, info = P.estimate(lex, counts)
    assert info["silence_probability"] == 0.99 and info["initial_silence_probability"] == 0.99
    none = [[words[(7 * u + 3 * j) % len(words)] for j in range(5)] for u in range(40)]
    toy = PC.ToyAligned(lex, none)
    new, info = P.estimate(lex, P.count_from_intervals(toy.ex, toy.batch))
    assert info["silence_probability"] == 0.01 and info["initial_silence_probability"] == 0.01
    assert all(p.silence_after_probability == 0.01 for p in new.pronunciations if p.silence_after_probability is not None)


# ---- files -----------------------------------------------------------------------------------------------------------------
def _path_costs(lex, words):
    """{(phone names of a path, rounded cost)} of ``phone_graph(words)`` without suffix sharing."""
    g = lex.phone_graph(words)
    out = []

    def walk(u, phones, cost):
        if u in g.final:
            out.append((tuple(phones), round(cost + g.final[u], 9)))
        for (v, ph, _ol, w) in g.arcs[u]:
            walk(v, phones + [lex.phone_table.find(ph)], cost + w)

    walk(g.start, [], 0.0)
    return sorted(out)


def test_dictionary_round_trip_and_graph_costs(tmp_path):
    lex = _hand_lexicon()
    toy = PC.ToyAligned(lex, HAND)
    new, info = P.estimate(lex, P.count_from_intervals(toy.ex, toy.batch))
    new.add_pronunciation(G.Pronunciation("0zero", "B"))                   # sorts first, written without columns
    path = P.write_dictionary(tmp_path / "out" / "lexicon.dict", new)
    lines = path.read_text(encoding="utf8").splitlines()
    assert [ln.split("\t")[0] for ln in lines] == ["0zero", "a", "a", "b", "d"]
    assert lines[0] == "0zero\tB" and lines[1] == "a\t1.0\t0.41\t1.49\t0.75\tA1" and lines[2].endswith("\tA2 A3")
    jpath = P.write_silence_info(tmp_path / "out" / "silence.json", info)
    kw = json.loads(jpath.read_text())
    assert kw == info
    back = G.LexiconCompiler(position_dependent_phones=False, silence_phone="sil", oov_phone="spn", share_suffixes=False, **kw)
    back.load_pronunciations(path)
    back.build_phone_table()
    assert sorted(PC.records(back)) == sorted(PC.records(new))
    assert [r[:2] for r in PC.records(back)][1:3] == [("a", "A1"), ("a", "A2 A3")]          # lexicon order inside a word
    # −log of the numbers on the arcs: every path of the one-word graph of "a" (two variants), by formula
    ln = lambda p: -math.log(p)          # noqa: E731
    p_init, f_sil, f_non = kw["initial_silence_probability"], kw["final_silence_correction"], kw["final_non_silence_correction"]
    want = []
    for phones, prob, after, s_corr, n_corr in ((("A1",), 1.0, 0.41, 1.49, 0.75), (("A2", "A3"), 0.67, 0.21, 1.0, 1.0)):
        for first in (True, False):
            for last in (True, False):
                cost = (ln(p_init) + ln(s_corr) if first else ln(1 - p_init) + ln(n_corr)) + ln(prob)
                cost += (ln(after) + ln(f_sil)) if last else (ln(1 - after) + ln(f_non))
                want.append((("sil",) * first + phones + ("sil",) * last, round(cost, 9)))
    assert _path_costs(back, ["a"]) == sorted(want)
    # refusals
    gap = P.copy_lexicon(lex)
    gap.pronunciations[0].silence_after_probability = 0.5
    with pytest.raises(ValueError, match="probability unset"):
        P.write_dictionary(tmp_path / "gap.dict", gap)
    with pytest.raises(ValueError, match="not LexiconCompiler keywords"):
        P.write_silence_info(tmp_path / "bad.json", dict(silence_probability=0.3, sil_prob=0.3))


# ---- the stage on a host backend -------------------------------------------------------------------------------------------
MEASURED_DIFFERING = 0           # word tokens whose (variant, silence after) is not the generator's, of MEASURED_TOKENS
MEASURED_TOKENS = 292


@pytest.fixture(scope="module")
def stage():
    from tests import train_mono_case as C

    corpus = C.train_corpus()
    y = C.supervised_yardstick()
    opt = AlignOptions(boost_silence=1.25)
    backend = PC.HostBackend(corpus, opt)
    tr = PronunciationProbabilityTrainer((y.tm.raw, A.raw_from_soa(y.am), y.tree), lexicon=corpus.world.lexicon, backend=backend,
                                         silence_phones=C.silence_ids(), align_options=opt)
    tr.train()
    return corpus, tr, backend


def test_trainer_on_host_backend_against_the_generators_streams(stage, tmp_path):
    """The oracle's alignments with the supervised yardstick model on the 48 training utterances, counted, against the
    counts of the generator's own token streams (``SynthWorld.utterance``'s segments: silence after a word with probability
    0.5, variants drawn uniformly).

    Measured on the CPU with the oracle alone: 0 of 292 word tokens (MEASURED_DIFFERING of MEASURED_TOKENS) carry another
    (variant, silence after) than the generator's — the shortest planted silence is 50 ms, five frames, and the yardstick
    model finds every one.  The cap is twice that share plus one token — one token here —: a short silence may legitimately
    be absorbed by its neighbours.

    Estimates: with at most D differing tokens in all, a record of a word with n tokens can have d = min(D, n) of them
    changed; its numbers move by at most what d tokens can move them (derived at ``_bounds``), plus 0.01 for rounding."""
    corpus, tr, backend = stage
    lex = corpus.world.lexicon
    assert tr.failed == 0 and all(c is not None for c in backend.ctms)
    truth = [PC.truth_stream(lex, text, segs) for text, segs in zip(corpus.text, corpus.segs)]
    aligned = [PC.ctm_stream(lex, c) for c in backend.ctms]
    differing = tokens = 0
    for t, a in zip(truth, aligned):
        tw, aw = PC.word_tokens(t), PC.word_tokens(a)
        assert [x[0][0] for x in tw] == [x[0][0] for x in aw]                      # the transcript's words, in order
        tokens += len(tw)
        differing += sum(x != y for x, y in zip(tw, aw))
    print(f"word tokens whose (variant, silence after) differs from the generator's: {differing} of {tokens}")
    cap = 2 * MEASURED_DIFFERING + 1
    assert tokens == MEASURED_TOKENS and differing <= cap
    ix = P.PronunciationIndex(lex)
    true_counts = R.count(truth, lex.silence_word)
    assert PC.as_dict(tr.counts, ix)["pron"].keys() <= set(PC.key_names(ix))
    # word tokens are the transcript's on both sides; what differs is bounded by the cap
    got, want = PC.as_dict(tr.counts, ix), true_counts.as_dict()
    assert sum(got["pron"].values()) == sum(want["pron"].values())
    for name in ("pron", "sil_following", "non_sil_following"):
        keys = set(got[name]) | set(want[name])
        assert sum(abs(got[name].get(k, 0) - want[name].get(k, 0)) for k in keys) <= 2 * cap, name
    want_rec, want_info = R.estimate(true_counts, PC.dictionary(lex), PC.OOV)
    bounds, sp_bound = _bounds(true_counts, want_rec, cap)
    assert abs(tr.info["silence_probability"] - want_info["silence_probability"]) <= sp_bound
    checked = 0
    for rec in PC.records(tr.lexicon):
        wp = rec[:2]
        if wp not in want_rec:
            assert rec[2:] == (None, None, None, None)
            continue
        for got_v, want_v, b in zip(rec[2:], want_rec[wp], bounds[wp]):
            assert abs(got_v - want_v) <= b + 1e-12, (wp, rec[2:], want_rec[wp], bounds[wp])
        checked += 1
    assert checked == len(want_rec) > 200
    # the stage carries the previous model and writes it with the dictionary and the silence numbers
    assert tr.raw_tm is tr.previous[0] and tr.raw_am is tr.previous[1] and tr.tree is tr.previous[2] and tr.lda_mat is None
    files = tr.write(tmp_path / "pp")
    assert [f.name for f in files] == ["final.mdl", "tree", "lexicon.dict", "silence_probabilities.json"]
    back = G.LexiconCompiler(position_dependent_phones=False, phones=corpus.world.phones, silence_phone="sil", oov_phone="spn",
                             **json.loads(files[3].read_text()))
    back.load_pronunciations(files[2])
    assert sorted(PC.records(back)) == sorted(PC.records(tr.lexicon))
    with pytest.raises(ValueError, match="lexicon"):
        PronunciationProbabilityTrainer((1, 2, 3))
    # the native batch compiler and graph.py agree on graphs that carry the new numbers
    from montreal_forced_aligner_amd.model import TransitionModel
    from tests.test_graph_native_cpu import _same as same_graph
    tm = TransitionModel(tr.raw_tm)
    gc = G.TrainingGraphCompiler(tm, tr.tree, tr.lexicon)
    scaled = tm.scaled_log_probs(1.0, 0.1)
    plain = G.TrainingGraphCompiler(tm, tr.tree, lex)
    for text, got in zip(corpus.text[:6], gc.compile_fsts(corpus.text[:6], scaled)):
        want_fst = G.add_transition_probs(gc.compile_fst(text), scaled)
        same_graph(got, want_fst)
        old = G.add_transition_probs(plain.compile_fst(text), scaled)
        assert old.arcs.shape != want_fst.arcs.shape or not np.array_equal(old.arcs["weight"], want_fst.arcs["weight"])
    print("info", tr.info)


def _bounds(t: R.Tables, want_rec, D: int):
    """Per record (probability, silence-after, silence-before correction, non-silence-before correction): how far D differing
    word tokens can move the estimate from the one of the true counts ``t``, each plus 0.01 for rounding.

    A differing token of word w moves one count of w's records by one (its variant's, or its silence-following /
    non-silence-following), and — through its silence-after — the "before" count and the pair of the token that follows it.
      silence_probability  s / (s + n): a token's silence-after flips one silence token in or out: s and n each move by at
                           most D, the total by at most D:  |Δ| ≤ 2D / (s + n − D)
      probability          c / m with the word's largest smoothed count m; c and m move by d = min(D, tokens of the word):
                           |Δ| ≤ d (m + c) / (m (m − d)) ≤ 2d / (m − d)  (m > d; else anything in [0, 1])
      silence-after        (sf + 2 sp) / (N + 2), N the record's tokens: sf and N move by d, sp by Δsp:
                           |Δ| ≤ (2d + 2 Δsp) / (max(N − d, 0) + 2)
      corrections          (c + 2) / (e + 2): c moves by d; the expected count e = Σ pairs · P(silence after the left item)
                           moves by at most 2d for pairs that come or go (a token's own variant and its predecessor's
                           silence) and by Σ pairs · bound(left) for the left items' probabilities:
                           |Δ| ≤ (d + v · Δe) / 2 with v the true value's own quotient (denominators are at least 2)"""
    s, n = sum(t.sil_before.values()), sum(t.non_sil_before.values())
    sp_bound = 2 * D / (s + n - D) + 0.01
    per_word = {}
    for (w, _p), c in t.pron.items():
        per_word[w] = per_word.get(w, 0) + c
    after_bound = {}
    for wp in want_rec:
        d = min(D, per_word[wp[0]])
        N = t.pron[wp]
        after_bound[wp] = min(1.0, (2 * d + 2 * sp_bound) / (max(N - d, 0) + 2) + 0.01)
    after_bound[PC.OOV] = 1.0
    after_bound[R.BOS] = 0.0
    de_sil, de_non = {}, {}
    for (left, right), (a, b) in t.ngram.items():
        de_sil[right] = de_sil.get(right, 0.0) + (a + b) * after_bound[left]
        de_non[right] = de_non.get(right, 0.0) + (a + b) * after_bound[left]
    out = {}
    for wp, (prob, _after, s_corr, n_corr) in want_rec.items():
        d = min(D, per_word[wp[0]])
        m = max(t.pron[k] + 1 for k in want_rec if k[0] == wp[0])
        b_prob = min(1.0, 2 * d / (m - d)) if m > d else 1.0
        b_s = (d + (s_corr + 0.01) * (2 * d + de_sil.get(wp, 0.0))) / 2
        b_n = (d + (n_corr + 0.01) * (2 * d + de_non.get(wp, 0.0))) / 2
        out[wp] = (b_prob + 0.01, after_bound[wp], b_s + 0.01, b_n + 0.01)
    return out, sp_bound
