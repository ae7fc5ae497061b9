"""Pitch through the public layers: a synthetic triphone model that lives in 45-dimensional features — Δ+ΔΔ of a 15-column
base, 13 MFCCs + POV feature + normalised log-pitch — through CorpusAligner(pitch_options=…), the same base through a
40 x 105 LDA with speaker adaptation, a batch of mixed sample rates, and the kalpy-shaped layer (PitchComputer,
Utterance.generate_features with a pitch computer).

What is checked.  The MFCC-derived columns of the pasted features are bit-identical to the features of the same audio without
pitch (pasting after CMVN disturbs nothing: zero sums in the padded CMVN statistics).  The pitch-derived columns equal Δ+ΔΔ of
the restatement's float64 ProcessPitch on the restatement's float32 chain within 4 x the float32-against-float64 yardstick of
tests/test_gpu_pitch.py (measured here on these inputs) plus float32 rounding of the delta chain: the delta filters' absolute
weights sum to 0.6 and 0.36, so they do not amplify the difference.  Alignments equal the oracle decoder's on the device's own
features."""
import wave

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd.model import pitch_options
from oracle import oracle as O
from tests import helpers, pitch_ref as R, synth

pytestmark = pytest.mark.gpu

SAMPLES = 48000                      # 3 s utterances
META = {"features": {"use_pitch": True, "use_voicing": True, "snip_edges": False}}       # (the engine's MFCC default: no snip_edges)
POPTS = pitch_options(META)
ROPTS = R.Opts(snip_edges=False)     # the same options for the restatement
MFCC_COLS = [c + 15 * b for b in range(3) for c in range(13)]
PITCH_COLS = [c + 15 * b for b in range(3) for c in (13, 14)]


@pytest.fixture(scope="module")
def pe():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from montreal_forced_aligner_amd.engine import AlignmentEngine

    e = AlignmentEngine(0)
    e.configure_mfcc()
    e.configure_pitch(**POPTS)
    yield e
    e.close()


def _base_and_cmvn(e, pcm):
    so = np.array([0, len(pcm)], dtype=np.int64)
    base, fo = e.base_features(torch.from_numpy(pcm).to(e.device), so)
    own = np.zeros(1, dtype=np.int32)
    stats = e.cmvn_stats(base[:, :13].contiguous(), fo, own, 1)
    return base, fo, own, e.pad_cmvn_stats(stats, 2)


@pytest.fixture(scope="module")
def flow(pe):
    from montreal_forced_aligner_amd.aligner import CorpusUtterance

    world = synth.SynthWorld.build()

    def delta_feats(pcm, spk):
        base, fo, own, cm = _base_and_cmvn(pe, pcm)
        return pe.features(base, fo, own, cm).cpu().numpy()

    model = synth.train_triphone(world, delta_feats, n_train=24, n_gauss=4)
    assert model.am.dim == 45
    utts = []
    for i in range(4):
        pcm, text, _segs, spk = world.utterance(9100 + i, n_words=9, samples=SAMPLES, speaker=3 + (i % 2))
        utts.append(CorpusUtterance(f"s{spk}-{i}", f"s{spk}", pcm, text))
    pt = world.lexicon.phone_table
    return dict(world=world, model=model, utts=utts, sil=[pt.find("sil"), pt.find("spn")],
                gc=G.TrainingGraphCompiler(model.tm, model.tree, world.lexicon), scaled=model.tm.scaled_log_probs(1.0, 0.1))


def _device_features(e, al, utts, lda=None, fmllr=None):
    """The final features of a corpus as the aligner forms them, from the engine's public pieces (one batch)."""
    spk_ids, cmvn = al.speaker_cmvn(utts)
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    base, fo = e.base_features(torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(e.device), so)
    rows = np.array([spk_ids[u.speaker] for u in utts], dtype=np.int32)
    d_lda = None if lda is None else torch.from_numpy(lda).to(e.device)
    d_fm = None if fmllr is None else torch.from_numpy(fmllr).to(e.device)
    feats = e.features(base, fo, rows, cmvn, lda=d_lda, fmllr=d_fm).cpu().numpy()
    return [feats[fo[k]: fo[k + 1]] for k in range(len(utts))], base.cpu().numpy(), fo, rows


def _oracle_agrees(flow, am, utts, results, feats):
    for u, r, x in zip(utts, results, feats):
        fst = G.add_transition_probs(flow["gc"].compile_fst(u.text), flow["scaled"])
        ref = helpers.oracle_align_feats(flow["model"].tm, fst, x, am, beam=10.0, retry_beam=40.0)
        assert ref["status"] in (0, 1) and r is not None
        assert r.num_frames == len(ref["ali"]) and np.array_equal(r.alignment, ref["ali"]) and np.array_equal(r.words, ref["words"])
        assert abs(r.likelihood - ref["like"]) / len(ref["ali"]) < 1e-3


def test_corpus_aligner_with_pitch_on_delta_features(pe, flow):
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    m, utts = flow["model"], flow["utts"]
    al = CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, engine=pe, silence_phones=flow["sil"],
                       options=AlignOptions(beam=10.0, retry_beam=40.0), pitch_options=POPTS)
    assert al.n_pitch == 2
    res = al.align(utts, speaker_adapted=False)
    assert al.failed == [] and all(r is not None for r in res)
    feats, base, fo, rows = _device_features(pe, al, utts)
    assert feats[0].shape[1] == 45 and base.shape[1] == 15
    _oracle_agrees(flow, m.am, utts, res, feats)
    for u, r in zip(utts, res):
        assert [w.label for w in r.ctm.word_intervals if w.label != flow["world"].lexicon.silence_word] == u.text.split()
    # MFCC columns and their deltas: exactly the features of the same corpus without pitch
    plain = CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, engine=pe, silence_phones=flow["sil"])     # (never aligns: 39 != 45)
    spk_ids, cmvn13 = plain.speaker_cmvn(utts)
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    mfcc, mfo = pe.mfcc(torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(pe.device), so)
    assert np.array_equal(mfo, fo)                                   # without snip_edges both counts are round(n / shift) here
    f39 = pe.features(mfcc, mfo, rows, cmvn13).cpu().numpy()
    got = np.concatenate(feats)
    assert np.array_equal(got[:, MFCC_COLS].view(np.uint32), f39.view(np.uint32))
    assert np.array_equal(base[:, :13].view(np.uint32), mfcc.cpu().numpy().view(np.uint32))
    # pitch columns: untouched by CMVN, and Δ+ΔΔ of the restatement's ProcessPitch within the tolerance
    yard = worst = 0.0
    for k, u in enumerate(utts):
        raw = R.compute(u.pcm, ROPTS, chain=True)["raw"]
        assert raw.shape[0] == fo[k + 1] - fo[k]
        want = R.process(raw, ROPTS)
        yard = max(yard, float(np.abs(R.process(raw, ROPTS, dt=np.float32).astype(np.float64) - want).max()))
        assert np.abs(base[fo[k]: fo[k + 1], 13:] - want).max() <= 4 * yard
        d = O.deltas(want.astype(np.float32))
        assert np.array_equal(feats[k][:, [13, 14]], base[fo[k]: fo[k + 1], 13:])
        worst = max(worst, float(np.abs(feats[k][:, PITCH_COLS] - d[:, [0, 1, 2, 3, 4, 5]]).max()))
        bound = 4 * yard + 8 * 2.0 ** -24 * float(np.abs(want).max())
        assert worst <= bound, (k, worst, bound)
    print(f"pitch-derived feature columns against the restatement: {worst:.3e} (float32 yardstick {yard:.3e})")


def test_pitch_options_none_is_the_path_without_the_keyword(engine, fx):
    """An existing small case (tests/test_gpu_corpus_aligner.py) with the keyword at its default.  What this checks is the
    oracle's alignment below, as the tests from before the keyword do: both constructions take the same code path, so their
    byte-for-byte agreement only says that the keyword is accepted and that ``None`` switches nothing on."""
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance

    sr = 16000
    cuts = [("spkA", 0.0, 4.2, "this is the acoustic corpus i'm talking pretty fast here"),
            ("spkB", 23.5, 26.72, "um and that should be all thanks")]
    utts = [CorpusUtterance(f"{s}-{k}", s, fx.pcm[int(a * sr): int(b * sr)], t) for k, (s, a, b, t) in enumerate(cuts)]
    runs = []
    for kw in ({}, {"pitch_options": None}):
        al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, options=AlignOptions(beam=100.0, retry_beam=400.0),
                           engine=engine, **kw)
        assert al.n_pitch == 0
        runs.append(al.align(utts, make_ctm=False))
    for a, b in zip(*runs):
        assert a.alignment.tobytes() == b.alignment.tobytes() and a.words.tobytes() == b.words.tobytes()
        assert a.likelihood == b.likelihood
    # and it is the oracle's alignment, as before
    mf = [O.mfcc(u.pcm.astype(np.float32), O.default_mfcc_opts()) for u in utts]
    for u, r, m in zip(utts, runs[1], mf):
        x = O.deltas(O.cmvn_apply(O.cmvn_stats([m]), m))
        fst = fx.mono_graph(u.text)
        pl = np.unique(fx.mono_tm.id2pdf[fst.arcs["ilabel"]])
        am = fx.mono_am
        ref = helpers.oracle_align(fx.mono_tm, fst, O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl), pl,
                                   beam=100.0, retry_beam=400.0)
        assert np.array_equal(r.alignment, ref["ali"])


def test_lda_fmllr_with_pitch_and_a_mixed_rate_batch(pe, flow):
    """40 x 105 LDA (15 base columns x 7 spliced frames), two-pass speaker adaptation, and an utterance that arrives at
    another sample rate: exactly the results of the same corpus converted beforehand."""
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance

    world, utts = flow["world"], flow["utts"]
    q, _ = np.linalg.qr(np.random.default_rng(9).normal(size=(105, 105)))
    lda = np.ascontiguousarray(q[:40]).astype(np.float32)
    d_lda = torch.from_numpy(lda).to(pe.device)

    def lda_feats(pcm, spk):
        base, fo, own, cm = _base_and_cmvn(pe, pcm)
        return pe.features(base, fo, own, cm, lda=d_lda).cpu().numpy()

    model = synth.train_triphone(world, lda_feats, n_train=24, n_gauss=4)
    assert model.am.dim == 40
    opts = AlignOptions(beam=10.0, retry_beam=40.0, fmllr_min_count=100.0)
    al = CorpusAligner(model.tm, model.am, model.tree, world.lexicon, lda=lda, engine=pe, silence_phones=flow["sil"], options=opts,
                       pitch_options=POPTS)
    res = al.align(utts, speaker_adapted=True, make_ctm=False)
    assert al.failed == [] and all(r is not None for r in res)
    W = al.transforms
    assert W.shape == (2, 40, 41) and np.isfinite(W).all() and np.abs(W[:, :, :40] - np.eye(40)).max() > 1e-3
    feats, _base, _fo, _rows = _device_features(pe, al, utts, lda=lda, fmllr=W)
    fl = dict(flow, model=model, gc=G.TrainingGraphCompiler(model.tm, model.tree, world.lexicon), scaled=model.tm.scaled_log_probs(1.0, 0.1))
    _oracle_agrees(fl, model.am, utts, res, feats)
    # the first utterance recorded at 8 kHz: converted on the device ahead of MFCC and pitch alike
    low = np.ascontiguousarray(utts[0].pcm[::2])
    conv, _ = pe.resample(torch.from_numpy(low).to(pe.device), np.array([0, len(low)], dtype=np.int64), [8000])
    mixed = [CorpusUtterance(utts[0].utt_id, utts[0].speaker, low, utts[0].text, sample_rate=8000)] + utts[1:]
    before = [CorpusUtterance(utts[0].utt_id, utts[0].speaker, conv.cpu().numpy(), utts[0].text)] + utts[1:]
    ra = al.align(mixed, speaker_adapted=False, make_ctm=False)
    rb = al.align(before, speaker_adapted=False, make_ctm=False)
    for a, b in zip(ra, rb):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a.alignment, b.alignment) and a.likelihood == b.likelihood
    assert ra[1] is not None
    # Δ+ΔΔ speaker adaptation with pitch is 45-dimensional: refused by the statistics' limit, loudly
    from montreal_forced_aligner_amd._lib import MfaHipError
    m45 = flow["model"]
    al45 = CorpusAligner(m45.tm, m45.am, m45.tree, world.lexicon, engine=pe, silence_phones=flow["sil"], options=opts, pitch_options=POPTS)
    with pytest.raises(MfaHipError, match="41"):
        al45.align(utts, speaker_adapted=True, make_ctm=False)


def test_kalpy_layer(pe, flow, tmp_path):
    from montreal_forced_aligner_amd import kalpy_api as KA

    pcm = flow["utts"][1].pcm
    mc = KA.MfccComputer(snip_edges=False, allow_upsample=True, allow_downsample=True)
    pc = KA.PitchComputer(**POPTS)
    with pytest.raises(ValueError):
        KA.PitchComputer(**dict(POPTS, add_delta_pitch=True))
    pitch = pc.compute_pitch(pcm)
    so = np.array([0, len(pcm)], dtype=np.int64)
    want = pe.pitch(torch.from_numpy(pcm).to(pe.device), so).cpu().numpy()
    assert pitch.shape == want.shape and pitch.shape[1] == 2 and np.array_equal(pitch, want)
    exported = pc.compute_pitch_for_export(pcm, compress=True)
    assert isinstance(exported, KA.CompressedFeatures) and np.array_equal(np.asarray(exported), want)
    # generate_features with a pitch computer: the aligner's features for a one-utterance speaker
    base, fo, own, cm = _base_and_cmvn(pe, pcm)
    ref = pe.features(base, fo, own, cm).cpu().numpy()
    utt = KA.Utterance(pcm, "")
    utt.generate_mfccs(mc)
    utt.apply_cmvn(KA.CmvnComputer().compute_cmvn_from_features([utt.mfccs]))
    got = utt.generate_features(mc, pc)
    assert got.shape == ref.shape == (fo[1], 45) and np.array_equal(got, ref)
    assert utt.generate_features(mc, None).shape[1] == 39
    # a wav file at another rate: converted on the device for MFCC and pitch alike
    low = np.ascontiguousarray(pcm[::2])
    path = tmp_path / "low.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000); w.writeframes(low.tobytes())
    seg = KA.Segment(path)
    conv, cso = pe.resample(torch.from_numpy(low).to(pe.device), np.array([0, len(low)], dtype=np.int64), [8000])
    assert np.array_equal(pc.compute_pitch(seg), pe.pitch(conv, cso).cpu().numpy())
    u2 = KA.Utterance(seg, "")
    u2.generate_mfccs(mc)
    u2.apply_cmvn(KA.CmvnComputer().compute_cmvn_from_features([u2.mfccs]))
    b2, f2, own2, cm2 = _base_and_cmvn(pe, conv.cpu().numpy())
    assert np.array_equal(u2.generate_features(mc, pc), pe.features(b2, f2, own2, cm2).cpu().numpy())


# ---------------------------------------------------------------------------------------- unequal frame counts: snip_edges
SNIP_META = {"features": {"use_pitch": True, "use_voicing": True}}            # MFA's model default: snip_edges True
SNIP_POPTS = pitch_options(SNIP_META)
SNIP_ROPTS = R.Opts(snip_edges=True)
LONG = 557 + 160 * 297               # 48 077 samples: 298 MFCC frames, 299 pitch frames (557 samples: 1 and 2)


@pytest.fixture()
def snip(pe):
    """The engine under snip_edges on both option sets; the module's options are put back afterwards."""
    pe.configure_mfcc(snip_edges=1)
    pe.configure_pitch(**SNIP_POPTS)
    yield pe
    pe.configure_mfcc()
    pe.configure_pitch(**POPTS)


def _snip_utts(flow):
    from montreal_forced_aligner_amd.aligner import CorpusUtterance

    utts = []
    for i, n in enumerate((LONG, SAMPLES, LONG, SAMPLES + 3)):          # pitch = mfcc + 1, equal, + 1, equal
        pcm, text, _segs, spk = flow["world"].utterance(9300 + i, n_words=9, samples=n, speaker=3 + (i % 2))
        utts.append(CorpusUtterance(f"s{spk}-{i}", f"s{spk}", pcm, text))
    return utts


def test_paste_rule_with_unequal_frame_counts(snip, flow):
    """snip_edges on both option sets: the tracker gives one frame more than the MFCC for two of the four utterances.  The
    pasted matrix has the MFCC's rows; its MFCC columns are the MFCC-only matrix bit for bit, its pitch columns the
    restatement's first rows (the row gather of base_features), the final features' MFCC columns those without pitch, and
    CorpusAligner aligns on them as the oracle does.  (The tracker never gives FEWER frames than the MFCC once it gives any:
    ceil(n / 4) - 100 >= (n - 400) / 4; the one case of an MFCC frame dropped is the test after this one.)"""
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    pe, m, utts = snip, flow["model"], _snip_utts(flow)
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(pe.device)
    mfo, pfo = pe.frame_offsets(so), pe.pitch_frame_offsets(so)
    assert (np.diff(pfo) - np.diff(mfo)).tolist() == [1, 0, 1, 0] and np.diff(mfo)[0] == 298
    base, fo = pe.base_features(pcm, so)
    assert np.array_equal(fo, mfo) and base.shape == (int(mfo[-1]), 15)
    base = base.cpu().numpy()
    full, _ = pe.mfcc(pcm, so)                                            # the MFCC with its own frame counts
    assert np.array_equal(base[:, :13].view(np.uint32), full.cpu().numpy().view(np.uint32))
    yard = 0.0
    for k, u in enumerate(utts):
        raw = R.compute(u.pcm, SNIP_ROPTS, chain=True)["raw"]
        assert raw.shape[0] == pfo[k + 1] - pfo[k]
        want = R.process(raw, SNIP_ROPTS)                                 # over the tracker's own frames, THEN cut
        yard = max(yard, float(np.abs(R.process(raw, SNIP_ROPTS, dt=np.float32).astype(np.float64) - want).max()))
        got = base[fo[k]: fo[k + 1], 13:]
        assert np.abs(got - want[: got.shape[0]]).max() <= 4 * yard, k
        if pfo[k + 1] - pfo[k] > got.shape[0]:                            # a gather off by one row would show: pitch moves per frame
            assert np.abs(got[1:] - want[: got.shape[0] - 1]).max() > 100 * yard
    # through CorpusAligner: same features, the oracle's alignment
    al = CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, engine=pe, silence_phones=flow["sil"], mfcc_options={"snip_edges": 1},
                       options=AlignOptions(beam=10.0, retry_beam=40.0), pitch_options=SNIP_POPTS)
    res = al.align(utts, speaker_adapted=False, make_ctm=False)
    assert al.failed == [] and all(r is not None for r in res)
    assert [r.num_frames for r in res] == np.diff(mfo).tolist()
    feats, base2, fo2, rows = _device_features(pe, al, utts)
    assert np.array_equal(base2.view(np.uint32), base.view(np.uint32))
    _oracle_agrees(flow, m.am, utts, res, feats)
    plain = CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, engine=pe, silence_phones=flow["sil"], mfcc_options={"snip_edges": 1})
    _spk, cmvn13 = plain.speaker_cmvn(utts)
    f39 = pe.features(full, mfo, rows, cmvn13).cpu().numpy()
    assert np.array_equal(np.concatenate(feats)[:, MFCC_COLS].view(np.uint32), f39.view(np.uint32))
    # a difference of more than one frame is refused on the host: pitch at twice the MFCC's frame rate
    pe.configure_pitch(**dict(SNIP_POPTS, frame_shift=5))
    from montreal_forced_aligner_amd._lib import MfaHipError
    with pytest.raises(MfaHipError, match="differ by more than 1"):
        pe.base_features(pcm, so)


def test_paste_rule_drops_the_mfcc_frame_of_an_utterance_too_short_for_pitch(pe, flow):
    """Without snip_edges 230 samples are one MFCC frame and no pitch frame (the resampled signal is shorter than a window):
    the utterance is pasted with no rows — the MFCC kernel is given fewer rows than it would count — and its neighbours are
    what they are alone.  396 samples (99 resampled ones, still no window) are two MFCC frames: refused."""
    from montreal_forced_aligner_amd._lib import MfaHipError

    long = flow["utts"][0].pcm
    parts = [long[:230], long, long[1000:1230]]
    so = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    assert np.diff(pe.frame_offsets(so)).tolist() == [1, 300, 1] and np.diff(pe.pitch_frame_offsets(so)).tolist() == [0, 300, 0]
    base, fo = pe.base_features(torch.from_numpy(np.concatenate(parts)).to(pe.device), so)
    assert fo.tolist() == [0, 0, 300, 300]
    alone, _ = pe.base_features(torch.from_numpy(long).to(pe.device), np.array([0, len(long)], dtype=np.int64))
    assert np.array_equal(base.cpu().numpy().view(np.uint32), alone.cpu().numpy().view(np.uint32))
    with pytest.raises(MfaHipError, match="differ by more than 1"):
        pe.base_features(torch.from_numpy(long[:396].copy()).to(pe.device), np.array([0, 396], dtype=np.int64))


def test_kalpy_layer_with_unequal_frame_counts(snip, flow):
    from montreal_forced_aligner_amd import kalpy_api as KA

    pe, pcm = snip, _snip_utts(flow)[0].pcm
    mc = KA.MfccComputer(snip_edges=True)
    pc = KA.PitchComputer(**SNIP_POPTS)
    pitch = pc.compute_pitch(pcm)
    utt = KA.Utterance(pcm, "")
    utt.generate_mfccs(mc)
    assert (utt.mfccs.shape[0], pitch.shape[0]) == (298, 299)
    utt.apply_cmvn(KA.CmvnComputer().compute_cmvn_from_features([utt.mfccs]))
    got = utt.generate_features(mc, pc)
    base, fo, own, cm = _base_and_cmvn(pe, pcm)
    assert got.shape == (298, 45) and np.array_equal(got, pe.features(base, fo, own, cm).cpu().numpy())
    assert np.array_equal(base[:, 13:].cpu().numpy(), pitch[:298])


def test_corpus_compression_with_pitch(pe, flow):
    """AlignOptions(corpus_compression=True) with pitch: the MFCC columns go through the 8-bit codec twice (raw, then
    CMVN-applied), the pitch columns once and in a table of their own.  The aligner's features equal that chain done by
    hand, and its alignments the oracle's on them."""
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    m, utts = flow["model"], flow["utts"][:2]
    al = CorpusAligner(m.tm, m.am, m.tree, flow["world"].lexicon, engine=pe, silence_phones=flow["sil"],
                       options=AlignOptions(beam=10.0, retry_beam=40.0, corpus_compression=True), pitch_options=POPTS)
    res = al.align(utts, speaker_adapted=False, make_ctm=False)
    assert all(r is not None for r in res)
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    base, fo = pe.base_features(torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(pe.device), so)
    base = base.cpu().numpy()
    once = [np.concatenate([K.compress_round_trip(np.ascontiguousarray(base[fo[k]: fo[k + 1], :13])),
                            K.compress_round_trip(np.ascontiguousarray(base[fo[k]: fo[k + 1], 13:]))], axis=1) for k in range(2)]
    spk_ids, cmvn = al.speaker_cmvn(utts)                 # (mfa_cmvn_stats on the MFCC columns after their first trip, zero-padded)
    rows = np.array([spk_ids[u.speaker] for u in utts], dtype=np.int32)
    stats = cmvn.cpu().numpy()
    assert stats.shape == (2, 2, 16) and not stats[:, :, 13:15].any()
    feats = []
    for k, x in enumerate(once):
        st = stats[rows[k]]
        mean = (st[0, :13] / st[0, -1]).astype(np.float32)
        feats.append(np.concatenate([K.compress_round_trip(x[:, :13] - mean), x[:, 13:]], axis=1))
        assert not np.array_equal(x[:, 13:], base[fo[k]: fo[k + 1], 13:]) and np.abs(x[:, 13:] - base[fo[k]: fo[k + 1], 13:]).max() < 0.05
    host = torch.from_numpy(np.concatenate(feats)).to(pe.device)
    want = pe.features(host, fo, rows, None).cpu().numpy()
    # what the aligner itself forms (its two feature steps, as align() calls them)
    cached, cfo = al._mfcc(utts, [0, 1])
    assert np.array_equal(cached.cpu().numpy(), np.concatenate(once))
    got = al._final_features(cached, cfo, rows, cmvn, None, None).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _oracle_agrees(flow, m.am, utts, res, [want[fo[k]: fo[k + 1]] for k in range(2)])
