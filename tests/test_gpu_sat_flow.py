"""The SAT stage through the host layers, on the device: ``CorpusAligner.estimate_alignment_model`` against the chain by hand
(the same device calls in the same order: byte-equal) and its two-feature statistics against the two-feature host twin on the
downloaded features and alignments (tier 3 of tests/test_gpu_gmm_acc_twofeats.py); one short ``SatTrainer`` run on Δ+ΔΔ
features, written, reloaded and aligned with as a ``final.mdl`` + ``final.alimdl`` pair; the same from an ``LdaTrainer``
stage; the kalpy name.  The corpus is the 48 utterances of tests/train_mono_case.py (46 speakers of one or two 3 s
utterances: ``fmllr_min_count`` is lowered to 100 frames so that speakers are estimated), the previous model a monophone model
of 6 iterations trained here."""
import dataclasses

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import fmllr as F
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import kalpy_api as KA
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.aligner import CorpusAligner
from montreal_forced_aligner_amd.engine import GmmStats, gmm_statistics_twofeats, gmm_statistics_twofeats_host
from montreal_forced_aligner_amd.train import LdaTrainer, MonophoneTrainer, SatTrainer, alignment_model
from tests import gmm_acc2_ref as R2
from tests import train_mono_case as C
from tests.test_gpu_gmm_acc_twofeats import check_against_twin

pytestmark = pytest.mark.gpu

MIN_COUNT = 100.0


def _bits(st):
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count], st.tid_count))


def _same_model(a, b):
    return all(np.array_equal(x, y) for f in ("gconsts", "weights", "means_invvars", "inv_vars") for x, y in zip(getattr(a, f), getattr(b, f)))


@pytest.fixture(scope="module")
def mono(engine):
    corpus = C.train_corpus()
    tr = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=6, max_gaussians=208,
                          silence_phones=C.silence_ids(), engine=engine)
    tr.train()
    return corpus, tr, dataclasses.replace(tr.opt, fmllr_min_count=MIN_COUNT)


def by_hand(al, utts):
    """``estimate_alignment_model``'s device calls, in its order; per batch also the downloaded (adapted features, unadapted
    features, alignments)."""
    down = []
    with al._run():
        _res, kept = al._align(utts, True, False, None, keep_last=True)
        spk_ids, cmvn = al.speaker_cmvn(utts)
        model = M.DiagGmmModel.from_raw(al.raw_am)
        al.engine.load_gmm(model)
        al._loaded = model
        st = GmmStats.zeros(model.num_gauss, model.dim, al.tm.num_transition_ids + 1)
        for idx, feats, ali, fo, _rows in kept:
            plain, fo2, _r = al._batch_features(utts, idx, spk_ids, cmvn, None, None)
            assert np.array_equal(fo, fo2)
            gmm_statistics_twofeats(al.engine, feats, plain, ali, al.tm, into=st)
            down.append((feats.cpu().numpy(), plain.cpu().numpy(), ali.cpu().numpy()))
        al._load(al.am)
    return st, down, model


def test_estimate_alignment_model_against_the_chain_by_hand(mono):
    corpus, tr, opt = mono
    utts = corpus.utterances()
    al = tr.aligner(options=opt)
    ali_tm, ali_am, stats = al.estimate_alignment_model(utts)
    assert stats is al.alimdl_stats and stats.tot_count > 12000
    W = al.transforms
    assert W.shape == (46, 39, 40) and np.isfinite(W).all()
    # estimates, not identities: a 3 s utterance has 300 frames, most of them speech, against a minimum of 100
    moved = np.abs(W[:, :, :39] - np.eye(39)).reshape(46, -1).max(axis=1) > 1e-2
    print(f"speakers with an estimate: {int(moved.sum())} of 46, rejected as degenerate: {al.fmllr_rejected}")
    assert moved.sum() >= 23
    want, down, model = by_hand(al, utts)
    assert _bits(stats) == _bits(want)
    want_tm, want_am = alignment_model(al.raw_tm, al.raw_am, want)
    assert _same_model(ali_am, want_am) and _same_model(ali_am, mle.mle_update(al.raw_am, want, remove_low_count_gaussians=False)[0])
    assert np.array_equal(ali_tm.log_probs, want_tm.log_probs) and not np.array_equal(ali_tm.log_probs, al.raw_tm.log_probs)
    assert [w.shape[0] for w in ali_am.weights] == [w.shape[0] for w in al.raw_am.weights]
    # the adapted and the unadapted rows differ, and the sums are those of the unadapted ones: the two-feature twin on the download
    x = np.concatenate([d[0] for d in down]); y = np.concatenate([d[1] for d in down]); a = np.concatenate([d[2] for d in down])
    assert x.shape == y.shape and np.abs(x - y).max() > 0.1
    case = R2.AccCase2("downloaded corpus", model, al.tm, x, y, a, None)
    twin = gmm_statistics_twofeats_host(model, x, y, a, al.tm)
    pdf, fw = R2.frame_tables(al.tm, a, None)
    ref = R2.gmm_acc2(x, y, pdf, fw, model)
    check_against_twin(stats, twin, ref, case, "estimate_alignment_model")
    # what the alignment model is for: the unadapted features under the resident alignments
    from montreal_forced_aligner_amd.engine import gmm_statistics_host
    ll_ali = gmm_statistics_host(M.DiagGmmModel.from_raw(ali_am), y, a, al.tm).loglike_per_frame
    ll_sat = gmm_statistics_host(model, y, a, al.tm).loglike_per_frame
    print(f"unadapted features, log-likelihood per frame: alignment model {ll_ali:.4f}, model {ll_sat:.4f}")
    assert np.isfinite(ll_ali) and np.isfinite(ll_sat)


def check_sat_history(sat, num_iterations, fmllr_iterations):
    h = sat.history
    assert [e["iteration"] for e in h] == list(range(num_iterations + 1)) and all(np.isfinite(e["loglike"]) for e in h)
    assert [("fmllr" in e) for e in h] == [i == 0 or i in fmllr_iterations for i in range(num_iterations + 1)]
    for e in h:
        if "fmllr" in e:
            f = e["fmllr"]
            assert set(f) == {"speakers", "rejected", "objf_impr_per_frame", "frames"}
            assert f["speakers"] + len(f["rejected"]) == len(sat.speakers) and f["speakers"] > 0
            assert f["objf_impr_per_frame"] > 0 and f["frames"] > 0
    assert {"events", "leaves", "questions", "tree_gain_per_frame", "skipped"} <= set(h[0])
    assert sat.raw_am.num_pdfs == h[0]["leaves"]
    # transforms: the composition of the recorded steps
    n, D = len(sat.speakers), sat.raw_am.dim
    assert len(sat.fmllr_steps) == 1 + len(fmllr_iterations) and sat.transforms.shape == (n, D, D + 1)
    rejected = [e["fmllr"]["rejected"] for e in h if "fmllr" in e]
    want = np.tile(np.eye(D, D + 1, dtype=np.float32), (n, 1, 1))
    for step, rej in zip(sat.fmllr_steps, rejected):
        for s, name in enumerate(sat.speakers):
            if name not in rej:
                want[s] = F.compose_transforms(step[s], want[s])
    assert np.array_equal(sat.transforms, want)
    # the alignment model
    assert set(sat.history_alimdl) == {"loglike", "frames", "updated", "floored"} and sat.history_alimdl["frames"] == sat.alimdl_stats.tot_count
    assert [w.shape[0] for w in sat.ali_raw_am.weights] == [w.shape[0] for w in sat.raw_am.weights]
    assert not _same_model(sat.ali_raw_am, sat.raw_am)


def check_written_pair(sat, files, engine, utts, lda):
    names = [p.name for p in files]
    assert names == ["final.mdl", "tree", "final.alimdl"] + (["lda.mat"] if lda else [])
    tm, am = M.load_model_bytes(files[0].read_bytes())
    tree = K.read_tree(files[1].read_bytes())
    ali_tm, ali_am = M.load_model_bytes(files[2].read_bytes())
    raw_ali_tm, raw_ali_am = K.read_model(files[2].read_bytes())
    assert _same_model(raw_ali_am, sat.ali_raw_am) and tree == sat.tree
    assert np.array_equal(raw_ali_tm.log_probs, sat.ali_raw_tm.log_probs) and np.array_equal(raw_ali_tm.tuples, sat.ali_raw_tm.tuples)
    assert np.array_equal(ali_am.pdf_offsets, am.pdf_offsets)
    mat = K.read_matrix_file(files[3].read_bytes()) if lda else None
    if lda:
        assert np.array_equal(mat, sat.lda_mat)
    al = CorpusAligner(tm, am, tree, C.world().lexicon, lda=mat, ali_am=ali_am, options=sat.opt, engine=engine, silence_phones=C.silence_ids())
    res = al.align(utts, speaker_adapted=True, make_ctm=False)
    assert all(r is not None for r in res) and al.failed == [] and al.fallback_first_pass == []
    assert al.transforms.shape == sat.transforms.shape
    return al


def test_sat_trainer_on_the_device(mono, engine, tmp_path):
    corpus, tr, opt = mono
    utts = corpus.utterances()
    opt = dataclasses.replace(opt, boost_silence=1.0)
    sat = SatTrainer(utts, C.world().lexicon, previous=tr, num_iterations=4, fmllr_iterations=(2,), num_leaves=100, max_gaussians=140,
                     align_options=opt, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    check_sat_history(sat, 4, (2,))
    assert sat.raw_am.dim == 39 and sat.lda_mat is None and sat.history[0]["leaves"] <= 100
    check_written_pair(sat, sat.write(tmp_path / "sat"), engine, utts, lda=False)
    own = sat.aligner()
    assert own.ali_am is not None and own.raw_ali_am is sat.ali_raw_am and own.lda is None
    # a stage on top: the transforms are picked up and the first estimate is skipped
    again = SatTrainer(utts, C.world().lexicon, previous=sat, num_iterations=1, fmllr_iterations=(), num_leaves=100, max_gaussians=140,
                       align_options=opt, silence_phones=C.silence_ids(), engine=engine).train()
    assert "fmllr" not in again.history[0] and np.array_equal(again.transforms, sat.transforms) and again.fmllr_steps == []


def test_sat_trainer_from_an_lda_stage(mono, engine, tmp_path):
    corpus, tr, opt = mono
    utts = corpus.utterances()
    opt = dataclasses.replace(opt, boost_silence=1.0)
    ldat = LdaTrainer(utts, C.world().lexicon, previous=(tr.raw_tm, tr.raw_am, tr.tree), num_iterations=8, max_gaussians=208,
                      silence_phones=C.silence_ids(), engine=engine).train()
    sat = SatTrainer(utts, C.world().lexicon, previous=ldat, num_iterations=4, fmllr_iterations=(2,), num_leaves=100, max_gaussians=140,
                     align_options=opt, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    check_sat_history(sat, 4, (2,))
    assert sat.raw_am.dim == 40 and np.array_equal(sat.lda_mat, ldat.lda_mat) and sat.transforms.shape[1:] == (40, 41)
    check_written_pair(sat, sat.write(tmp_path / "sat_lda"), engine, utts, lda=True)
    assert np.array_equal(sat.aligner().lda, ldat.lda_mat)


def test_kalpy_layer(mono, engine, tmp_path, monkeypatch):
    corpus, tr, opt = mono
    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    utts = corpus.utterances()
    al = tr.aligner(options=opt)
    with al._run():
        _res, kept = al._align(utts, True, False, None, keep_last=True)
        spk_ids, cmvn = al.speaker_cmvn(utts)
        batches = [(list(idx), feats.cpu().numpy(), al._batch_features(utts, idx, spk_ids, cmvn, None, None)[0].cpu().numpy(),
                    ali.cpu().numpy(), np.asarray(fo, np.int64)) for idx, feats, ali, fo, _rows in kept]
    mdl, _tree = tr.write(tmp_path / "mono")
    feats, si_feats, alis = {}, {}, []
    for idx, x, y, ali, fo in batches:
        for k, i in enumerate(idx):
            feats[utts[i].utt_id] = x[fo[k]: fo[k + 1]]
            si_feats[utts[i].utt_id] = y[fo[k]: fo[k + 1]]
            alis.append((utts[i].utt_id, ali[fo[k]: fo[k + 1]]))
    alis.sort(key=lambda e: e[0])
    K.write_table(tmp_path / "ali.ark", alis, "int_vector")
    short = alis[3][0]
    si_feats[short] = si_feats[short][:-1]               # other frame counts in the two archives: skipped
    del feats[alis[5][0]]                                # missing from one archive: skipped
    acc = KA.TwoFeatsStatsAccumulator(mdl)
    seen = []
    acc.accumulate_stats(feats, si_feats, KA.AlignmentArchive(tmp_path / "ali.ark"), callback=seen.append)
    keep = [k for j, (k, _a) in enumerate(alis) if j not in (3, 5)]
    assert seen == keep
    # the same batch by the function itself, with the model as the accumulator read it
    engine.load_gmm(acc.acoustic_model)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(engine.device)      # noqa: E731
    by_key = dict(alis)
    want = gmm_statistics_twofeats(engine, dev(np.concatenate([feats[k] for k in keep])), dev(np.concatenate([si_feats[k] for k in keep])),
                                   dev(np.concatenate([by_key[k] for k in keep])), acc.transition_model)
    assert _bits(acc.gmm_accs.stats) == _bits(want) and want.tot_count > 12000
    assert np.array_equal(acc.transition_accs, want.tid_count.astype(np.float64))
