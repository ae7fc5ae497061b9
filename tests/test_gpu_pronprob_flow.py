"""The pronunciation-probability stage on the device: ``CorpusAligner.pronunciation_statistics`` (the array counter over every
batch's interval arrays) against ``pronprob.count_from_ctm`` over the ``ctm`` objects of an ``align`` call on the same
utterances — one batch and several, a failed utterance and an empty transcript among them, the two-pass flow of a model with
an alignment model —, ``train_dictionary``, and ``PronunciationProbabilityTrainer`` after a short ``MonophoneTrainer`` run:
written, reloaded, aligned with against the oracle, and continued by a ``SatTrainer`` on graphs from the new lexicon.  The
corpus is the 48 utterances of 3 s of tests/train_mono_case.py; no kernel is new here, the device work is ``align``'s."""
import copy
import dataclasses
import json

import numpy as np
import pytest

from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd import pronprob as P
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance
from montreal_forced_aligner_amd.train import MonophoneTrainer, PronunciationProbabilityTrainer, SatTrainer
from tests import helpers
from tests import pronprob_case as PC
from tests import train_mono_case as C
from tests.test_graph_native_cpu import _same as same_graph

pytestmark = pytest.mark.gpu

MIN_COUNT = 100.0          # 46 speakers of one or two 3 s utterances


@pytest.fixture(scope="module")
def yard():
    """The supervised yardstick model of the corpus (one Gaussian per state from the generator's labels) and a
    speaker-independent "alignment model" of the same layout: broader variances, slightly shifted means."""
    y = C.supervised_yardstick()
    rng = np.random.default_rng(22)
    am = y.am
    ali_am = copy.copy(am)
    var = 1.0 / am.inv_vars
    mean = am.means_invvars * var
    var2 = var * 1.3
    mean2 = mean + 0.05 * np.sqrt(var) * rng.normal(size=mean.shape)
    w_log = am.gconsts + 0.5 * (am.dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
    ali_am.inv_vars = (1.0 / var2).astype(np.float32)
    ali_am.means_invvars = (mean2 / var2).astype(np.float32)
    ali_am.gconsts = (w_log - 0.5 * (am.dim * np.log(2 * np.pi) + np.log(var2).sum(axis=1) + (mean2 * mean2 / var2).sum(axis=1))).astype(np.float32)
    return y, ali_am


def _utterances(broken: bool):
    utts = C.train_corpus().utterances()
    if broken:
        long_text = " ".join(u.text for u in utts[:6])
        utts[20] = CorpusUtterance("short", utts[20].speaker, utts[20].pcm[:3200].copy(), long_text)   # 20 frames for 40 words
        utts[21] = dataclasses.replace(utts[21], text="")                                              # optional silence only
    return utts


def _aligner(engine, yard, batch_frames, ali=False):
    y, ali_am = yard
    return CorpusAligner(y.tm, y.am, y.tree, C.world().lexicon, engine=engine, silence_phones=C.silence_ids(),
                         options=AlignOptions(boost_silence=1.25, batch_frames=batch_frames, fmllr_min_count=MIN_COUNT),
                         ali_am=ali_am if ali else None)


@pytest.mark.parametrize("batch_frames,broken,adapted", [(2_000_000, False, False), (2000, False, False), (2000, True, False),
                                                          (2_000_000, True, False), (2000, False, True)],
                         ids=["one-batch", "batches", "batches-failed-and-empty", "one-batch-failed-and-empty", "two-pass"])
def test_statistics_equal_the_specification_on_the_ctms(engine, yard, batch_frames, broken, adapted):
    utts = _utterances(broken)
    al = _aligner(engine, yard, batch_frames, ali=adapted)
    assert (len(al._batches(utts)) == 1) == (batch_frames > 2000)
    res = al.align(utts, speaker_adapted=adapted)
    failed = list(al.failed)
    want = P.count_from_ctm(al.lexicon, [None if r is None else r.ctm for r in res])
    got = al.pronunciation_statistics(utts, speaker_adapted=adapted)
    assert got is al.pronunciation_counts and al.failed == failed
    for f in P.PronunciationCounts.FIELDS + ("pair_keys", "pair_counts"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert got.utterances == sum(r is not None and r.ctm is not None for r in res)
    if broken:
        assert failed == ["short"] and res[20] is None and got.utterances == len(utts) - 1
        assert [w.label for w in res[21].ctm.word_intervals] == [al.lexicon.silence_word]           # "<s> sil </s>"
    else:
        assert not failed and got.utterances == len(utts)
    ix = P.PronunciationIndex(al.lexicon)
    n_words = sum(len(u.text.split()) for u, r in zip(utts, res) if r is not None)
    assert int(got.count[: ix.n_records].sum() + got.count[ix.oov]) == n_words
    if adapted:
        assert al.transforms is not None and al.transforms.shape == (46, 39, 40)


def test_train_dictionary_is_the_estimate_of_the_specifications_counts(engine, yard):
    utts = _utterances(False)
    al = _aligner(engine, yard, 2000)
    res = al.align(utts)
    want_lex, want_info = P.estimate(al.lexicon, P.count_from_ctm(al.lexicon, [r.ctm for r in res]))
    lex, info = al.train_dictionary(utts)
    assert info == want_info and PC.records(lex) == PC.records(want_lex)
    assert lex is not al.lexicon and all(p.probability is None for p in al.lexicon.pronunciations)
    seen = [p for p in lex.pronunciations if p.probability is not None]
    assert len(seen) > 200 and 0.2 <= info["silence_probability"] <= 0.45


@pytest.fixture(scope="module")
def stage(engine, tmp_path_factory):
    corpus = C.train_corpus()
    mono = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=6, max_gaussians=208,
                            silence_phones=C.silence_ids(), engine=engine).train()
    pp = PronunciationProbabilityTrainer(mono, corpus.utterances(), C.world().lexicon).train()
    out = tmp_path_factory.mktemp("pronprob")
    files = pp.write(out)
    reloaded = G.LexiconCompiler(position_dependent_phones=False, phones=C.world().phones, silence_phone="sil", oov_phone="spn",
                                 **json.loads((out / pp.SILENCE_INFO).read_text()))
    reloaded.load_pronunciations(out / pp.DICTIONARY)
    reloaded.build_phone_table()
    return corpus, mono, pp, files, reloaded


def test_trainer_output_reloads_and_aligns_like_the_oracle(engine, stage):
    corpus, mono, pp, files, reloaded = stage
    assert [f.name for f in files] == ["final.mdl", "tree", pp.DICTIONARY, pp.SILENCE_INFO]
    # (a flat-start model of 6 iterations may lose an utterance at beam 10 / 40: it then counts nowhere)
    assert pp.failed <= 2 and pp.counts.utterances == len(corpus.text) - pp.failed and pp.opt is mono.opt and pp.backend.engine is engine
    assert pp.raw_tm is mono.raw_tm and pp.raw_am is mono.raw_am and pp.tree is mono.tree and not pp.speaker_adapted
    assert sorted(PC.records(reloaded)) == sorted(PC.records(pp.lexicon)) and list(reloaded.phone_table) == list(pp.lexicon.phone_table)
    assert (reloaded.silence_probability, reloaded.initial_silence_probability, reloaded.final_silence_correction,
            reloaded.final_non_silence_correction) == tuple(pp.info[k] for k in P.SILENCE_INFO_KEYS)
    tm, am = M.load_model_bytes(files[0].read_bytes())
    tree = K.read_tree(files[1].read_bytes())
    al = CorpusAligner(tm, am, tree, reloaded, engine=engine, silence_phones=C.silence_ids(), options=mono.opt)
    res = al.align(corpus.utterances(), make_ctm=False)
    # the oracle on the oracle's features, on graphs compiled by graph.py from the same reloaded lexicon
    boosted = copy.copy(am)
    boosted.gconsts = am.gconsts.copy()
    boosted.boost_silence(mono.opt.boost_silence, M.pdfs_of_phones(tm, C.silence_ids()))
    gc = G.TrainingGraphCompiler(tm, tree, reloaded)
    scaled = tm.scaled_log_probs(mono.opt.transition_scale, mono.opt.self_loop_scale)
    plain = G.TrainingGraphCompiler(tm, tree, C.world().lexicon)
    moved = n_ok = 0
    for k, (text, x, r) in enumerate(zip(corpus.text, corpus.features(), res)):
        fst = G.add_transition_probs(gc.compile_fst(text), scaled)
        ref = helpers.oracle_align_feats(tm, fst, x, boosted, mono.opt.acoustic_scale, mono.opt.beam, mono.opt.retry_beam)
        if ref["status"] not in (0, 1):
            assert r is None and corpus.utterances()[k].utt_id in al.failure_reasons, k
            continue
        assert r is not None, (k, al.failure_reasons)
        n_ok += 1
        T = len(ref["ali"])
        assert r.num_frames == T and np.array_equal(r.alignment, ref["ali"]), f"utterance {k}: alignment differs from the oracle"
        assert np.array_equal(r.words, ref["words"]), k
        assert abs(r.likelihood - ref["like"]) / T < 1e-3, k
        if k < 4:          # the new weights are in the graphs: the same transcript under the lexicon without numbers costs otherwise
            old = G.add_transition_probs(plain.compile_fst(text), scaled)
            moved += not (old.arcs.shape == fst.arcs.shape and np.array_equal(old.arcs["weight"], fst.arcs["weight"]))
    assert moved >= 3 and n_ok >= len(corpus.text) - 2


def test_sat_stage_continues_on_graphs_of_the_new_lexicon(engine, stage):
    corpus, mono, pp, _files, reloaded = stage
    utts = corpus.utterances()
    opt = dataclasses.replace(mono.opt, fmllr_min_count=MIN_COUNT)
    sat = SatTrainer(utts, pp.lexicon, previous=pp, num_iterations=1, fmllr_iterations=(), num_leaves=100, max_gaussians=140,
                     align_options=opt, silence_phones=C.silence_ids(), engine=engine).train()
    assert [e["iteration"] for e in sat.history] == [0, 1] and all(np.isfinite(e["loglike"]) for e in sat.history)
    assert "fmllr" in sat.history[0] and sat.ali_raw_am is not None and sat.lexicon is pp.lexicon
    al = sat.backend.al
    assert al.lexicon is pp.lexicon
    # the stage's own training graphs (its aligner's compiler, on the transition model it last aligned with) against graph.py
    # on the dictionary and silence numbers read back from the files — and not the graphs of the lexicon without numbers
    assert al.tree == sat.tree
    gc = G.TrainingGraphCompiler(al.tm, sat.tree, reloaded)
    plain = G.TrainingGraphCompiler(al.tm, sat.tree, C.world().lexicon)
    for k in (0, 17):
        got = al.compiler.compile_fsts([utts[k].text], al.scaled)[0]
        same_graph(got, G.add_transition_probs(gc.compile_fst(utts[k].text), al.scaled))
        old = G.add_transition_probs(plain.compile_fst(utts[k].text), al.scaled)
        assert old.arcs.shape != got.arcs.shape or not np.array_equal(old.arcs["weight"], got.arcs["weight"])
