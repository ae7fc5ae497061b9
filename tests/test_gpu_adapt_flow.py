"""Model adaptation end to end on the synthetic world (synth_workload.py): 24 utterances of 2 s, two speakers; a monophone
model on Δ+ΔΔ features and a small mixture model (4 Gaussians per leaf) on LDA + fMLLR features with an alignment model,
each with its means pushed off by 0.3 deviations first.  ``CorpusAligner.adapt`` against the chain run by hand, the
likelihood of the adapted model on the same alignments, the adapted model back through a file and through an alignment,
and the kalpy layer."""

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import adapt as A
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance
from montreal_forced_aligner_amd.engine import GmmStats, gmm_statistics
from tests import gmm_acc_ref as R
from tests import synth

pytestmark = pytest.mark.gpu

OPTS = dict(beam=10.0, retry_beam=40.0, batch_frames=2000)       # about ten utterances per batch: three batches


def _bits(st):
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count], st.tid_count))


def _same_model(a, b):
    return a.dim == b.dim and all(x.tobytes() == y.tobytes() and x.dtype == y.dtype == np.float32
                                  for name in ("gconsts", "weights", "means_invvars", "inv_vars")
                                  for x, y in zip(getattr(a, name), getattr(b, name)))


def _pushed(am, rng, by=0.3):
    """The model's per-pdf form with every mean moved by ``by`` deviations (weights read back out of the gconsts)."""
    raw = A.raw_from_soa(am)
    for p in range(raw.num_pdfs):
        iv = raw.inv_vars[p].astype(np.float64)
        mean = raw.means_invvars[p] / iv + by * rng.normal(size=iv.shape) / np.sqrt(iv)
        raw.means_invvars[p] = (mean * iv).astype(np.float32)
        raw.gconsts[p] = A.gconsts(raw.weights[p], raw.means_invvars[p], raw.inv_vars[p])
    return raw


@pytest.fixture(scope="module")
def world(engine):
    engine.configure_mfcc()
    w = synth.SynthWorld.build()
    utts = []
    for i in range(24):
        pcm, text, _segs, spk = w.utterance(9300 + i, n_words=6, samples=32000, speaker=3 + (i % 2))
        utts.append(CorpusUtterance(f"s{spk}-{i}", f"s{spk}", pcm, text))
    pt = w.lexicon.phone_table
    return w, utts, [pt.find("sil"), pt.find("spn")]


def _feature_fn(engine, d_lda=None):
    def fn(pcm, spk):
        so = np.array([0, len(pcm)], dtype=np.int64)
        mfcc, fo = engine.mfcc(torch.from_numpy(pcm.copy()).to(engine.device), so)
        own = np.zeros(1, dtype=np.int32)
        return engine.features(mfcc, fo, own, engine.cmvn_stats(mfcc, fo, own, 1), lda=d_lda).cpu().numpy()
    return fn


@pytest.fixture(scope="module")
def mono(engine, world):
    w, _utts, _sil = world
    model = synth.train_monophone(w, _feature_fn(engine), n_train=30)
    return model, _pushed(model.am, np.random.default_rng(31))


@pytest.fixture(scope="module")
def mixture(engine, world):
    w, _utts, _sil = world
    lda = synth.seeded_lda()
    model = synth.train_triphone(w, _feature_fn(engine, torch.from_numpy(lda).to(engine.device)), n_train=30, n_gauss=4, n_classes=2)
    rng = np.random.default_rng(32)
    raw = _pushed(model.am, rng)
    # a speaker-independent alignment model with the same layout: broader variances, its own pushed means
    raw_ali = _pushed(model.am, rng)
    for p in range(raw_ali.num_pdfs):
        mean = raw_ali.means_invvars[p] / raw_ali.inv_vars[p].astype(np.float64)
        raw_ali.inv_vars[p] = (raw_ali.inv_vars[p] / np.float32(1.3)).astype(np.float32)
        raw_ali.means_invvars[p] = (mean * raw_ali.inv_vars[p]).astype(np.float32)
        raw_ali.gconsts[p] = A.gconsts(raw_ali.weights[p], raw_ali.means_invvars[p], raw_ali.inv_vars[p])
    return model, raw, raw_ali, lda


def _by_hand(engine, aligner, utts, speaker_adapted, raw):
    """The chain the issue names, on the batches the aligner's last pass leaves: engine.gmm_statistics over them."""
    _results, kept = aligner._align(list(utts), speaker_adapted, False, None, keep_last=True)
    assert len(kept) >= 3
    return kept, _accumulate(engine, kept, aligner.tm, raw)


def _accumulate(engine, kept, tm, raw):
    am = M.DiagGmmModel.from_raw(raw)
    engine.load_gmm(am)
    st = GmmStats.zeros(am.num_gauss, am.dim, tm.num_transition_ids + 1)
    for _idx, feats, ali, _fo, _rows in kept:
        gmm_statistics(engine, feats, ali, tm, into=st)
    return st


def _check_written(aligner, tmp_path):
    written = aligner.write_adapted(tmp_path / "adapted")
    tm, am, ali = aligner.adapted
    assert [p.name for p in written] == (["final.mdl"] if ali is None else ["final.mdl", "final.alimdl"])
    for path, want in zip(written, (am, ali)):
        rtm, ram = K.read_model(path.read_bytes())
        assert _same_model(ram, want) and rtm.log_probs.tobytes() == tm.log_probs.tobytes() and np.array_equal(rtm.tuples, tm.tuples)
        ltm, lam = M.load_model_bytes(path.read_bytes())
        assert lam.means_invvars.tobytes() == np.concatenate(want.means_invvars).tobytes()
        assert lam.gconsts.tobytes() == np.concatenate(want.gconsts).tobytes() and ltm.log_probs.tobytes() == tm.log_probs.tobytes()


def test_monophone_adapt_equals_the_chain_by_hand(engine, world, mono, tmp_path):
    w, utts, sil = world
    model, raw = mono
    raw_tm = model.tm.raw

    def make():
        return CorpusAligner(M.TransitionModel(raw_tm), M.DiagGmmModel.from_raw(raw), model.tree, w.lexicon, engine=engine,
                             options=AlignOptions(**OPTS), silence_phones=sil, raw_tm=raw_tm, raw_am=raw)

    with pytest.raises(ValueError, match="raw_tm"):
        CorpusAligner(model.tm, M.DiagGmmModel.from_raw(raw), model.tree, w.lexicon, engine=engine, silence_phones=sil).adapt(utts)
    al = make()
    results = al.adapt(utts)
    assert all(r is not None for r in results) and al.failed == []
    kept, st = _by_hand(engine, make(), utts, False, raw)
    assert _bits(st) == _bits(al.adapt_stats)
    assert st.tot_count == sum(r.num_frames for r in results) and st.tid_count.sum() == st.tot_count
    new_am, updated, kept_g = A.map_update(raw, A.ismooth_from_model(raw, st, 20.0))
    new_tm = A.transition_update(raw_tm, st.tid_count)
    tm_a, am_a, ali_a = al.adapted
    assert ali_a is None and _same_model(am_a, new_am) and tm_a.log_probs.tobytes() == new_tm.log_probs.tobytes()
    assert al.adapt_counts["mdl"] == (updated, kept_g) and updated > 0
    assert not np.array_equal(new_tm.log_probs, raw_tm.log_probs)
    assert al.adapt_loglike["mdl"] == st.tot_like / st.tot_count and al.adapt_loglike["alimdl"] is None
    # EM with a prior centred on the old means cannot lower the likelihood of the same alignments
    again = _accumulate(engine, kept, al.tm, new_am)
    print(f"monophone: average log-likelihood per frame {st.loglike_per_frame:.4f} -> {again.loglike_per_frame:.4f}")
    assert again.tot_count == st.tot_count and again.loglike_per_frame > st.loglike_per_frame
    # the adapted model is the aligner's own now: it aligns the corpus, and survives its file
    assert _same_model(al.raw_am, new_am) and al.am.means_invvars.tobytes() == np.concatenate(new_am.means_invvars).tobytes()
    al._loaded = None          # (the accumulation above loaded its own model into the shared engine)
    second = al.align(utts, make_ctm=False)
    assert all(r is not None for r in second) and al.failed == []
    _check_written(al, tmp_path)


def test_mixture_model_with_alignment_model_and_fmllr(engine, world, mixture, tmp_path):
    w, utts, sil = world
    model, raw, raw_ali, lda = mixture
    raw_tm = model.tm.raw

    def make():
        return CorpusAligner(M.TransitionModel(raw_tm), M.DiagGmmModel.from_raw(raw), model.tree, w.lexicon, lda=lda, engine=engine,
                             options=AlignOptions(**OPTS), silence_phones=sil, ali_am=M.DiagGmmModel.from_raw(raw_ali),
                             raw_tm=raw_tm, raw_am=raw, raw_ali_am=raw_ali)

    al = make()
    results = al.adapt(utts, speaker_adapted=True, make_ctm=False)
    assert all(r is not None for r in results) and al.transforms is not None
    hand = make()
    kept, st = _by_hand(engine, hand, utts, True, raw)
    assert np.array_equal(hand.transforms, al.transforms)
    st_ali = _accumulate(engine, kept, hand.tm, raw_ali)
    assert _bits(st) == _bits(al.adapt_stats) and _bits(st_ali) == _bits(al.adapt_ali_stats)
    # the alignment model saw the same frames and the same alignments
    assert np.array_equal(st.tid_count, st_ali.tid_count) and st.tot_count == st_ali.tot_count
    assert not np.array_equal(st.occ, st_ali.occ)
    tm_a, am_a, ali_a = al.adapted
    new_am, up, keep = A.map_update(raw, A.ismooth_from_model(raw, st, 20.0))
    new_ali, up2, keep2 = A.map_update(raw_ali, A.ismooth_from_model(raw_ali, st_ali, 20.0))
    assert _same_model(am_a, new_am) and _same_model(ali_a, new_ali)
    assert tm_a.log_probs.tobytes() == A.transition_update(raw_tm, st.tid_count).log_probs.tobytes()
    assert al.adapt_counts == {"mdl": (up, keep), "alimdl": (up2, keep2)} and up > 0
    for name, r, s, new in (("mdl", raw, st, new_am), ("alimdl", raw_ali, st_ali, new_ali)):
        again = _accumulate(engine, kept, al.tm, new)
        print(f"mixture {name}: average log-likelihood per frame {s.loglike_per_frame:.4f} -> {again.loglike_per_frame:.4f}")
        assert again.loglike_per_frame > s.loglike_per_frame
        assert al.adapt_loglike[name] == s.loglike_per_frame
    al._loaded = None          # (the accumulation above loaded its own model into the shared engine)
    second = al.align(utts, speaker_adapted=True, make_ctm=False)
    assert all(r is not None for r in second) and al.failed == []
    _check_written(al, tmp_path)
    # update_transitions=False keeps the transition model
    al2 = make()
    al2.adapt(utts[:6], speaker_adapted=False, update_transitions=False, make_ctm=False)
    assert al2.adapted[0] is raw_tm and al2.adapted[2] is None


def test_kalpy_layer_gives_the_engines_statistics(engine, world, mono, tmp_path):
    from montreal_forced_aligner_amd import kalpy_api as KA

    w, utts, sil = world
    model, raw = mono
    with open(tmp_path / "final.mdl", "wb") as f:
        K.write_model(f, model.tm.raw, raw)
    some = utts[:8]
    mfcc = KA.MfccComputer(sample_frequency=16000, frame_length=25, frame_shift=10, num_mel_bins=23, num_coefficients=13,
                           snip_edges=False, dither=0.0, use_energy=False)
    mfcc.export_feats(tmp_path / "feats.ark", [(u.utt_id, u.pcm) for u in some], write_scp=True, compress=False)
    spk2utt = {}
    for u in some:
        spk2utt.setdefault(u.speaker, []).append(u.utt_id)
    KA.CmvnComputer().export_cmvn(tmp_path / "cmvn.ark", dict(K.read_ark((tmp_path / "feats.ark").read_bytes(), "matrix")), spk2utt)
    fa = KA.FeatureArchive(tmp_path / "feats.scp", utt2spk={u.utt_id: u.speaker for u in some}, cmvn_file_name=tmp_path / "cmvn.scp",
                           deltas=True)
    gc = KA.TrainingGraphCompiler(model.tm, model.tree, w.lexicon)
    gc.export_graphs(tmp_path / "fsts.ark", [(u.utt_id, u.text) for u in some])
    aligner = KA.GmmAligner(tmp_path / "final.mdl")
    aligner.export_alignments(tmp_path / "ali.ark", KA.FstArchive(tmp_path / "fsts.ark"), fa)
    aa = KA.AlignmentArchive(tmp_path / "ali.ark")
    seen = []
    acc = KA.GmmStatsAccumulator(tmp_path / "final.mdl", batch_frames=500)          # several device batches
    acc.accumulate_stats(fa, aa, callback=seen.append)
    assert len(seen) >= 6 and set(seen) <= {u.utt_id for u in some}
    feats = dict(fa)
    x = np.concatenate([feats[k] for k in seen]).astype(np.float32)
    ali = np.concatenate([np.asarray(aa[k].alignment, np.int32) for k in seen])
    tm, am = KA.read_gmm_model(tmp_path / "final.mdl")
    engine.load_gmm(am)
    one = gmm_statistics(engine, torch.from_numpy(x).to(engine.device), torch.from_numpy(ali).to(engine.device), tm)
    got = acc.gmm_accs.stats
    pdf, fw = R.frame_tables(tm, ali)
    ref = R.gmm_acc(x, pdf, fw, am)
    T2 = 2.0 * ref["n_frames"] * R.U64            # the same posteriors summed in two associations
    assert (np.abs(got.occ - one.occ) <= T2 * ref["occ"]).all()
    assert (np.abs(got.mean_acc - one.mean_acc) <= T2[:, None] * ref["S_mean"]).all()
    assert (np.abs(got.var_acc - one.var_acc) <= T2[:, None] * ref["var"]).all()
    assert abs(got.tot_like - one.tot_like) <= 2 * len(ali) * R.U64 * ref["S_tot"] and got.tot_count == one.tot_count == len(ali)
    assert np.array_equal(acc.transition_accs, one.tid_count.astype(np.float64)) and acc.gmm_accs.TotCount() == len(ali)
    # the reference's sequence on these objects (MFA/alignment/adapting.py:103-135)
    total = KA.AccumAmDiagGmm()
    total.init(am)
    total.Add(1.0, acc.gmm_accs)
    assert total.TotLogLike() == got.tot_like
    KA.IsmoothStatsAmDiagGmmFromModel(am, 20, total)
    want_am, _, _ = A.map_update(A.raw_from_soa(am), total.stats)
    want_tm = A.transition_update(tm.raw, got.tid_count)
    impr_t, count_t = tm.mle_update(acc.transition_accs)
    impr, count = am.mle_update(total, update_flags_str="m", remove_low_count_gaussians=False)
    assert impr > 0 and count == total.stats.occ.sum() and count_t > 0 and np.isfinite(impr_t)
    with pytest.raises(NotImplementedError):
        am.mle_update(total, update_flags_str="mv")
    with pytest.raises(NotImplementedError):
        am.mle_update(total, remove_low_count_gaussians=True)
    KA.write_gmm_model(tmp_path / "adapted.mdl", tm, am)
    rtm, ram = K.read_model((tmp_path / "adapted.mdl").read_bytes())
    assert _same_model(ram, want_am) and rtm.log_probs.tobytes() == want_tm.log_probs.tobytes()
