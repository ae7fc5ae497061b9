"""Speaker adaptation on the Δ+ΔΔ feature path through the public flow: a triphone model that lives in delta features
(no LDA), CorpusAligner's two passes (MFA/alignment/base.py:510-539), transforms a run comes with
(``previous_transforms``), and the kalpy-shaped layer (FeatureArchive / Utterance.generate_features with a transform and
no LDA matrix: Job.construct_feature_archive with ``deltas=True``, MFA/db.py:2101-2136).  Checked against the oracle's chain
O.mfcc → speaker CMVN → O.deltas → O.affine(W[spk]) → lazy-decodable alignment."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import graph as G
from oracle import oracle as O
from tests import delta_fmllr_helpers as H
from tests import helpers, synth

pytestmark = pytest.mark.gpu

SAMPLES = 80000        # 5 s utterances: 4 per speaker leave each speaker well over MIN_COUNT non-silence frames
MIN_COUNT = 300.0


@pytest.fixture(scope="module")
def flow(engine):
    from montreal_forced_aligner_amd.aligner import CorpusUtterance

    world = synth.SynthWorld.build()
    engine.configure_mfcc()

    def delta_feats(pcm, spk):
        so = np.array([0, len(pcm)], dtype=np.int64)
        mfcc, fo = engine.mfcc(torch.from_numpy(pcm).to(engine.device), so)
        own = np.zeros(1, dtype=np.int32)
        return engine.features(mfcc, fo, own, engine.cmvn_stats(mfcc, fo, own, 1)).cpu().numpy()

    model = synth.train_triphone(world, delta_feats, n_train=40, n_gauss=8)
    assert model.am.dim == 39
    utts = []
    for i in range(8):
        pcm, text, _segs, spk = world.utterance(9000 + i, n_words=15, samples=SAMPLES, speaker=3 + (i % 2))
        utts.append(CorpusUtterance(f"s{spk}-{i}", f"s{spk}", pcm, text))
    pt = world.lexicon.phone_table
    sil = [pt.find("sil"), pt.find("spn")]
    # the oracle's front end up to the deltas, per utterance, with the speaker's CMVN (speaker rows in first-appearance order)
    mf = [O.mfcc(u.pcm.astype(np.float32), O.default_mfcc_opts()) for u in utts]
    names = list(dict.fromkeys(u.speaker for u in utts))
    stats = {s: O.cmvn_stats([m for m, u in zip(mf, utts) if u.speaker == s]) for s in names}
    deltas = [O.deltas(O.cmvn_apply(stats[u.speaker], m)) for u, m in zip(utts, mf)]
    gc = G.TrainingGraphCompiler(model.tm, model.tree, world.lexicon)
    scaled = model.tm.scaled_log_probs(1.0, 0.1)
    return dict(world=world, model=model, utts=utts, sil=sil, names=names, deltas=deltas, gc=gc, scaled=scaled, cache={})


def _aligner(engine, flow, **kw):
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    m = flow["model"]
    return CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, lda=None, engine=engine, silence_phones=flow["sil"],
                         options=AlignOptions(beam=10.0, retry_beam=40.0, fmllr_min_count=MIN_COUNT), **kw)


def _first_pass(engine, flow):
    """The unadapted run, shared by the tests that compare against it."""
    if "first" not in flow["cache"]:
        al = _aligner(engine, flow)
        flow["cache"]["first"] = al.align(flow["utts"], speaker_adapted=False, make_ctm=False)
        assert al.transforms is None
    return flow["cache"]["first"]


def _matches_oracle(flow, results, W, which=(0, 1)):
    """Utterances ``which`` (one per speaker): the oracle's path with transform ``W[speaker row]`` gives a frame-identical
    alignment and the same per-frame likelihood to 1e-3."""
    m = flow["model"]
    for u in which:
        utt, r = flow["utts"][u], results[u]
        x = O.affine(flow["deltas"][u], W[flow["names"].index(utt.speaker)])
        fst = G.add_transition_probs(flow["gc"].compile_fst(utt.text), flow["scaled"])
        ref = helpers.oracle_align_feats(m.tm, fst, x, m.am, beam=10.0, retry_beam=40.0)
        assert ref["status"] in (0, 1) and r is not None          # both aligned (a failed utterance has no result)
        T = len(ref["ali"])
        assert r.num_frames == T and np.array_equal(r.alignment, ref["ali"]), f"utterance {u}: boundaries differ from the oracle"
        assert np.array_equal(r.words, ref["words"])
        assert abs(r.likelihood - ref["like"]) / T < 1e-3


def test_two_pass_alignment_on_delta_features(engine, flow):
    from montreal_forced_aligner_amd import fmllr as F
    from montreal_forced_aligner_amd.engine import fmllr_statistics

    utts, model = flow["utts"], flow["model"]
    first = _first_pass(engine, flow)
    al = _aligner(engine, flow)
    second = al.align(utts, speaker_adapted=True)
    assert all(r is not None for r in first) and all(r is not None for r in second)
    assert al.failed == [] and al.fmllr_rejected == []
    W = al.transforms
    assert W.shape == (2, 39, 40) and W.dtype == np.float32 and np.isfinite(W).all()
    # an estimate, not a copy of the starting point: float32 rounding of an identity would be below 1e-6, two voices that
    # differ in pitch and vocal-tract length move a 39×39 estimate from a few hundred frames by far more than 1e-2
    assert np.abs(W[:, :, :39] - np.eye(39)).max() > 1e-2
    # the same statistics and solve, by hand, from the first-pass alignments
    spk_ids, cmvn = al.speaker_cmvn(utts)
    assert list(spk_ids) == flow["names"]
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    mfcc, fo = engine.mfcc(torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(engine.device), so)
    rows = np.array([spk_ids[u.speaker] for u in utts], dtype=np.int32)
    feats = engine.features(mfcc, fo, rows, cmvn)
    ali = torch.from_numpy(np.concatenate([r.alignment for r in first]).astype(np.int32)).to(engine.device)
    ids, beta, K, Gm = fmllr_statistics(engine, feats, fo, ali, model.tm, rows, flow["sil"], 0.0)
    assert np.all(beta >= MIN_COUNT), beta
    for k, s in enumerate(ids):
        Wk, impr = F.compute_fmllr(beta[k], K[k], Gm[k], min_count=MIN_COUNT)
        assert impr > 0 and np.array_equal(Wk, W[s])
    for u, r in zip(utts, second):
        words = [w.label for w in r.ctm.word_intervals if w.label != flow["world"].lexicon.silence_word]
        assert words == u.text.split()
    _matches_oracle(flow, second, W)


def test_previous_transforms_reach_the_delta_features(engine, flow):
    utts = flow["utts"]
    prev = H.seeded_delta_fmllr(2)
    first = _first_pass(engine, flow)
    al = _aligner(engine, flow)
    res = al.align(utts, speaker_adapted=False, previous_transforms=prev, make_ctm=False)
    assert all(r is not None for r in res) and np.array_equal(al.transforms, prev)
    _matches_oracle(flow, res, prev)
    assert any(r.per_frame_likelihood != f.per_frame_likelihood for r, f in zip(res, first)), \
        "the transforms the run came with left every likelihood as it was"


def test_two_model_form_on_delta_features(engine, flow):
    """``ali_am`` (a final.alimdl) with a delta-feature model: first pass and posteriors on it, statistics and second pass
    on ``am``.  The statistics are checked at dimension 39 by tests/test_gpu_fmllr_stats.py; here: the flow runs."""
    ali_am = H.second_model(np.random.default_rng(11), flow["model"].am)
    al = _aligner(engine, flow, ali_am=ali_am)
    utts = flow["utts"][:4]
    res = al.align(utts, speaker_adapted=True, make_ctm=False)
    assert len(res) == 4 and all(r is not None for r in res)
    assert al.transforms.shape == (2, 39, 40) and np.isfinite(al.transforms).all()


def test_kalpy_layer_applies_transforms_after_deltas(tmp_path):
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd import kalpy_api as KA

    rng = np.random.default_rng(77)
    mats = {"a-1": helpers.mfcc_like(rng, 37, 13), "b-1": helpers.mfcc_like(rng, 5, 13), "a-2": helpers.mfcc_like(rng, 130, 13)}
    utt2spk = {"a-1": "a", "b-1": "b", "a-2": "a"}
    stats = {s: O.cmvn_stats([m for k, m in mats.items() if utt2spk[k] == s]) for s in ("a", "b")}
    W = helpers.random_affine(rng, 39, 40)
    K.write_table(tmp_path / "feats.ark", mats.items(), "matrix", scp_path=tmp_path / "feats.scp")
    K.write_table(tmp_path / "cmvn.ark", stats.items(), "matrix")
    K.write_table(tmp_path / "trans.ark", [("a", W)], "matrix")            # speaker b has no transform
    fa = KA.FeatureArchive(tmp_path / "feats.scp", utt2spk=utt2spk, cmvn_file_name=tmp_path / "cmvn.ark",
                           transform_file_name=tmp_path / "trans.ark", deltas=True)
    got = dict(fa)
    assert list(got) == list(mats)
    for k, m in mats.items():
        d = O.deltas(O.cmvn_apply(stats[utt2spk[k]], m))
        want = O.affine(d, W) if utt2spk[k] == "a" else d
        assert got[k].shape == want.shape and np.abs(got[k] - want).max() < 1e-4, k
    assert np.abs(got["a-1"] - O.deltas(O.cmvn_apply(stats["a"], mats["a-1"]))).max() > 1.0   # not the plain deltas
    with pytest.raises(NotImplementedError):             # CMVN-only features take no transform: refused, not dropped
        KA.FeatureArchive(tmp_path / "feats.scp", utt2spk=utt2spk, cmvn_file_name=tmp_path / "cmvn.ark",
                          transform_file_name=tmp_path / "trans.ark")
    # Utterance.generate_features: the same for one utterance, the transform given without an LDA matrix
    utt = KA.Utterance(None, "")
    utt.mfccs = mats["a-2"]
    utt.apply_cmvn(stats["a"])
    one = utt.generate_features(None, fmllr_trans=W)
    assert np.abs(one - O.affine(O.deltas(O.cmvn_apply(stats["a"], mats["a-2"])), W)).max() < 1e-4
    assert np.array_equal(one, got["a-2"])


def test_fine_tune_boundaries_passes_delta_transforms_on(fx, tmp_path):
    """fine_tune_boundaries(fmllr=…, lda=None): the 1 ms features carry the speaker's transform.  The identity [I | 0] is exact
    in the fmaf chain (every other term is 0·y), so it must leave every boundary where the run without a transform puts it;
    a transform that moves the features by a few units a dimension must move boundaries on the 1 ms grid."""
    from montreal_forced_aligner_amd import finetune as FT
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd import kalpy_api as KA

    ar = K.load_acoustic_model_archive(helpers.REF / "mono_model.zip")
    (tmp_path / "final.mdl").write_bytes(ar["final.mdl"])
    pcm = fx.pcm[: 16000 * 3]
    aligner = KA.GmmAligner(tmp_path / "final.mdl", beam=100, retry_beam=400, transition_scale=1.0, acoustic_scale=0.1,
                            self_loop_scale=0.1)
    eng = aligner._engine()
    eng.configure_mfcc()
    mfcc, fo = eng.mfcc(torch.from_numpy(pcm.astype(np.int16)).to(eng.device), np.array([0, len(pcm)], dtype=np.int64))
    own = np.zeros(1, np.int32)
    cmvn = eng.cmvn_stats(mfcc, fo, own, 1)
    al = aligner.align_utterance(fx.mono_gc.compile_fst("this is the acoustic corpus i'm talking"), eng.features(mfcc, fo, own, cmvn).cpu().numpy())
    assert al is not None
    ivs = al.generate_ctm(aligner.transition_model, fx.mono_lex.phone_table, 0.01)

    def tuned(W):
        fm = None if W is None else torch.from_numpy(W).to(eng.device)
        new, deleted = FT.fine_tune_boundaries(aligner, fx.mono_gc, [pcm], [ivs], utt2spk=[0], cmvn=cmvn, fmllr=fm)
        return [(iv.begin, iv.end) for iv in new[0]], deleted[0]

    plain = tuned(None)
    assert tuned(np.eye(39, 40, dtype=np.float32)[None].copy()) == plain
    assert tuned(H.seeded_delta_fmllr(1)) != plain
