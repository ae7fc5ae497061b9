"""The LDA stage through the host layers, on the device: ``CorpusAligner.estimate_lda`` against the chain by hand (downloaded
base features, CMVN and alignments → ``lda_statistics_host`` → ``estimate_lda``), with and without ``corpus_compression``;
one ``LdaTrainer`` run of 8 iterations held to what the host run is held to (tests/test_lda_cpu.py), written, reloaded and
aligned with; the kalpy names.  The corpus is the 48 utterances of tests/train_mono_case.py, the previous model a monophone
model of 6 iterations trained here."""
import dataclasses

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import kalpy_api as KA
from montreal_forced_aligner_amd import lda
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner
from montreal_forced_aligner_amd.stats import LdaStats, lda_statistics_host, silence_weights, tid_tables
from montreal_forced_aligner_amd.train import LdaTrainer, MonophoneTrainer
from tests import lda_ref
from tests import train_mono_case as C
from tests.test_lda_cpu import check_lda_training

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mono(engine):
    corpus = C.train_corpus()
    tr = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=6, max_gaussians=208,
                          silence_phones=C.silence_ids(), engine=engine)
    tr.backend.equal_align(tr.raw_tm, tr.raw_am, tr.tree, tr.seed)
    equal_share = C.phone_share(corpus, tr.raw_tm, tr.backend.alignments())
    tr.train()
    al = tr.aligner()
    res = al.align(corpus.utterances(), make_ctm=False)
    mono_share = C.phone_share(corpus, tr.raw_tm, [None if r is None else r.alignment for r in res])
    return corpus, tr, equal_share, mono_share


def by_hand(al, utts):
    """What ``estimate_lda`` works on, downloaded: per batch (base rows, frame offsets, speaker rows, CMVN or None,
    alignments, corpus positions) — with ``corpus_compression`` the twice-compressed CMVN-applied rows without CMVN."""
    out = []
    with al._run():
        _res, kept = al._align(utts, False, False, None, keep_last=True)
        _ids, cmvn = al.speaker_cmvn(utts)
        for idx, _feats, ali, fo, rows in kept:
            mfcc, _fo = al._mfcc(utts, idx)
            cm = cmvn.cpu().numpy()
            if al.opt.corpus_compression:
                mfcc = al.engine.compress_round_trip(mfcc, fo, cols=(0, mfcc.shape[1]), cmvn=cmvn, utt2spk=rows)
                cm = None
            out.append((mfcc.cpu().numpy(), np.asarray(fo, np.int64), rows, cm, ali.cpu().numpy(), np.asarray(idx, np.uint32)))
    return out


def check_estimate(al, utts):
    mat, full = al.estimate_lda(utts, dim=40)
    got = al.lda_stats
    tm = al.tm
    weights = silence_weights(tm, C.silence_ids(), 0.0)
    want = None
    n_total, abs2, abs1 = 0, 0.0, 0.0
    for mfcc, fo, rows, cm, ali, _keys in by_hand(al, utts):
        want = lda_statistics_host(mfcc, fo, rows if cm is not None else None, cm, ali, tm, weights=weights, into=want)
        id2class, w = tid_tables(tm, weights)
        case = lda_ref.Case(mfcc, fo, rows if cm is not None else None, cm, ali, id2class, w, tm.num_pdfs, 3)
        _st, a2, a1, n = lda_ref.statistics(case, want_abs=True)
        n_total, abs2, abs1 = n_total + n, abs2 + a2, abs1 + a1
    assert n_total > 5000 and got.first.shape == (tm.num_pdfs, 91)
    assert np.array_equal(got.zero, want.zero)
    assert np.all(np.abs(got.second - want.second) <= lda_ref.bound(n_total, abs2))
    assert np.all(np.abs(got.first - want.first) <= lda_ref.bound(n_total, abs1))
    # the two matrices through the identities, evaluated with the twin's within / between
    _N, _m, within, between = lda_ref.scatter(want)
    mat_h, full_h = lda.estimate_lda(want, dim=40)
    r_host = lda_ref.identity_residuals(full_h, within, between)
    r_dev = lda_ref.identity_residuals(full, within, between)
    print("identity residuals: host statistics", r_host[:2], "device statistics", r_dev[:2])
    assert mat.shape == (40, 91) and np.array_equal(mat, full[:40])
    # the twin's own float32 result sets the scale (the cast: tests/test_lda_cpu.py); ×64 as there
    assert r_dev[0] <= 64 * r_host[0] and r_dev[1] <= 64 * r_host[1]
    return got, lda_ref.bound(n_total, abs2), lda_ref.bound(n_total, abs1)


def test_estimate_lda_against_the_chain_by_hand(mono):
    corpus, tr, _e, _m = mono
    check_estimate(tr.aligner(), corpus.utterances())


def test_estimate_lda_with_corpus_compression(mono):
    corpus, tr, _e, _m = mono
    opt = dataclasses.replace(tr.opt, corpus_compression=True)
    plain = tr.aligner()
    plain.estimate_lda(corpus.utterances())
    got, _b2, _b1 = check_estimate(tr.aligner(options=opt), corpus.utterances())
    assert not np.array_equal(got.second, plain.lda_stats.second)          # quantised rows: other statistics


@pytest.fixture(scope="module")
def lda_run(mono, engine):
    corpus, tr, equal_share, mono_share = mono
    ldat = LdaTrainer(corpus.utterances(), C.world().lexicon, previous=(tr.raw_tm, tr.raw_am, tr.tree), num_iterations=8,
                      max_gaussians=208, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    return ldat


def test_lda_trainer_on_the_device(mono, lda_run, engine, tmp_path):
    corpus, tr, equal_share, mono_share = mono
    ldat = lda_run
    utts = corpus.utterances()
    own = ldat.aligner().align(utts, make_ctm=False)
    assert all(r is not None for r in own)
    check_lda_training(corpus, tr, ldat, [r.alignment for r in own], equal_share, mono_share)
    # write, reload the three files, align every training utterance: the same alignments
    mdl, tree_path, mat_path = ldat.write(tmp_path / "lda")
    tm, am = M.load_model_bytes(mdl.read_bytes())
    tree = K.read_tree(tree_path.read_bytes())
    mat = K.read_matrix_file(mat_path.read_bytes())
    assert am.dim == 40 and np.array_equal(mat, ldat.lda_mat)
    al = CorpusAligner(tm, am, tree, C.world().lexicon, lda=mat, options=ldat.opt, engine=engine, silence_phones=C.silence_ids())
    res = al.align(utts, make_ctm=False)
    assert all(r is not None for r in res) and al.failed == []
    for a, b in zip(res, own):
        assert np.array_equal(a.alignment, b.alignment)


def test_kalpy_layer(mono, engine, tmp_path, monkeypatch):
    corpus, tr, _e, _m = mono
    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    utts = corpus.utterances()
    al = tr.aligner()
    batches = by_hand(al, utts)
    mdl, _tree = tr.write(tmp_path / "mono")
    # a FeatureArchive / AlignmentArchive pair as the reference's LdaAccStatsFunction opens them
    feats, alis, u2s, cmvn = [], [], {}, {}
    for mfcc, fo, rows, cm, ali, keys in batches:
        for k, i in enumerate(keys.tolist()):
            feats.append((utts[i].utt_id, mfcc[fo[k]: fo[k + 1]]))
            alis.append((utts[i].utt_id, ali[fo[k]: fo[k + 1]]))
            u2s[utts[i].utt_id] = utts[i].speaker
        names = {r: utts[i].speaker for r, i in zip(rows.tolist(), keys.tolist())}
        for r, name in names.items():
            cmvn[name] = cm[r]
    feats.sort(key=lambda e: e[0]); alis.sort(key=lambda e: e[0])
    K.write_table(tmp_path / "feats.ark", feats, "matrix", tmp_path / "feats.scp")
    K.write_table(tmp_path / "cmvn.ark", sorted(cmvn.items()), "matrix", tmp_path / "cmvn.scp")
    K.write_table(tmp_path / "ali.ark", alis, "int_vector")
    archive = KA.FeatureArchive(tmp_path / "feats.scp", utt2spk=u2s, cmvn_file_name=tmp_path / "cmvn.scp", deltas=False,
                                splices=True, splice_frames=3)
    with pytest.raises(NotImplementedError):
        next(iter(archive))                                    # spliced rows without a matrix are still not made
    acc = KA.LdaStatsAccumulator(mdl, C.silence_ids(), rand_prune=0.0)
    seen = []
    acc.accumulate_stats(archive, KA.AlignmentArchive(tmp_path / "ali.ark"), callback=seen.append)
    assert sorted(seen) == [u.utt_id for u in utts]
    st = acc.lda.stats
    assert isinstance(st, LdaStats) and st.zero.sum() > 5000
    mat, full = acc.lda.estimate(KA.LdaEstimateOptions())
    want_mat, want_full = lda.estimate_lda(st)
    assert np.array_equal(mat, want_mat) and np.array_equal(full, want_full) and mat.shape == (40, 91)
    # the statistics are the aligner's own (the utterances in another order: under the summation bound)
    own, bound2, bound1 = check_estimate(al, utts)
    assert np.array_equal(st.zero, own.zero)
    assert np.all(np.abs(st.second - own.second) <= bound2) and np.all(np.abs(st.first - own.first) <= bound1)
    # Add, and pruning as the reference asks for it
    total = KA.LdaEstimate()
    total.Add(acc.lda); total.Add(acc.lda)
    assert np.array_equal(total.stats.zero, 2 * st.zero)
    pruned = KA.LdaStatsAccumulator(mdl, C.silence_ids(), rand_prune=4.0)
    pruned.accumulate_stats(archive, KA.AlignmentArchive(tmp_path / "ali.ark"))
    z = pruned.lda.stats.zero
    assert np.all(z % 4.0 == 0) and 0.15 * st.zero.sum() < z.sum() / 4.0 < 0.35 * st.zero.sum()
