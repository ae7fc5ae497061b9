"""Speech-activity segmentation and the feature archive's speech-activity options end to end on the device: the reference's
recording with digital silence spliced in goes through ``segment_utterance_vad`` and has to give the segments the plain
restatement (tests/vad_ref.py) and the frame walk give on the device's MFCCs; ``VadSegmenter`` over a two-rate batch, its
TextGrids, its utterances through ``CorpusAligner``; ``VadComputer.export_vad`` → ``FeatureArchive(vad_file_name=,
subsample_n=, use_sliding_cmvn=)`` against the same stages called by hand."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import segment as S
from tests import vad_ref as R

pytestmark = pytest.mark.gpu

SR = 16000
PAUSES = (6.0, 17.0)          # seconds of the original recording where half a second of zeros goes in


@pytest.fixture(scope="module")
def spliced(fx):
    """(pcm, [(begin, end) of the inserted pauses in the new recording])."""
    parts, pauses, at, shift = [], [], 0, 0.0
    for p in PAUSES:
        cut = int(p * SR)
        parts += [fx.pcm[at:cut], np.zeros(SR // 2, dtype=np.int16)]
        pauses.append((p + shift, p + shift + 0.5))
        at, shift = cut, shift + 0.5
    parts.append(fx.pcm[at:])
    return np.concatenate(parts), pauses


@pytest.fixture(autouse=True)
def default_mfcc_after(engine):
    yield
    engine.configure_mfcc()


def ivs(segments):
    return [(s.begin, s.end) for s in segments]


def by_hand(engine, pcm, seg_opts, adaptive=True):
    """The chain of the reference, stage by stage: the device's MFCCs, then the restatement's VAD, the frame walk, the merge."""
    import torch

    engine.configure_mfcc(use_energy=1, raw_energy=0, energy_floor=0.0)
    mfcc, fo = engine.mfcc(torch.from_numpy(pcm).to(engine.device), np.array([0, len(pcm)], dtype=np.int64))
    e = mfcc[:, 0].cpu().numpy().astype(np.float64)
    o = dict(energy_threshold=0.0, energy_mean_scale=1.0) if adaptive else dict(energy_threshold=5.5, energy_mean_scale=0.5)
    vad, thr = R.vad(e, **o)
    assert np.abs(e - thr).min() > len(e) * 2.0 ** -53 * np.abs(e).sum() + 2.0 ** -23 * abs(thr)     # no frame sits on the threshold
    return S.merge_segments(S.get_initial_segmentation(vad, 0.01), seg_opts["min_pause_duration"], seg_opts["max_segment_length"],
                            seg_opts["min_segment_length"]), vad


def test_segment_utterance_vad_equals_the_chain_by_hand(engine, spliced):
    pcm, pauses = spliced
    for seg_opts, adaptive in ((S.DEFAULT_SEGMENTATION, True), (dict(S.DEFAULT_SEGMENTATION, max_segment_length=8.0), True),
                               (S.DEFAULT_SEGMENTATION, False)):
        got = S.segment_utterance_vad(engine, pcm, SR, {}, {"energy_threshold": 5.5, "energy_mean_scale": 0.5}, dict(seg_opts),
                                      adaptive=adaptive)
        want, vad = by_hand(engine, pcm, seg_opts, adaptive)
        assert ivs(got) == ivs(want) and len(got) >= (3 if adaptive else 1)
        assert all(s.label == "speech" for s in got)
        if adaptive:
            for p0, p1 in pauses:             # both pauses are boundaries: silent inside, and no segment reaches across
                assert vad[int(p0 * 100) + 5: int(p1 * 100) - 5].sum() == 0
                assert not any(s.begin < p0 + 0.1 and s.end > p1 - 0.1 for s in got)
        if seg_opts["max_segment_length"] == 30.0:
            assert all(s.end - s.begin <= 30.0 for s in got)
    engine.configure_mfcc()
    got = S.segment_utterance_vad(engine, pcm, SR, begin=100.0)
    assert all(s.end - s.begin <= 30.0 for s in got) and got[0].begin >= 100.0
    assert engine.mfcc_opts.use_energy == 0          # the segmenter's forced options did not stay on the shared engine


@pytest.fixture(scope="module")
def segmenter(engine, spliced):
    pcm, _ = spliced
    seg = S.VadSegmenter(engine)
    seg.segment([("long", pcm, None), ("half_rate", np.ascontiguousarray(pcm[: 12 * SR: 2]), SR // 2)])
    return seg


def test_vad_segmenter_batch_equals_single_recordings(engine, spliced, segmenter):
    pcm, _ = spliced
    assert seg_defaults(segmenter)
    assert ivs(segmenter.segments["long"]) == ivs(S.segment_utterance_vad(engine, pcm, SR))
    alone = S.segment_utterance_vad(engine, np.ascontiguousarray(pcm[: 12 * SR: 2]), SR // 2)
    assert ivs(segmenter.segments["half_rate"]) == ivs(alone) and len(alone) >= 2


def seg_defaults(seg):
    return seg.segmentation_options == dict(max_segment_length=30.0, min_pause_duration=0.333, min_segment_length=0.333) and \
        seg.vad_options == dict(energy_threshold=5.5, energy_mean_scale=0.5)


def test_export_files_round_trip(segmenter, tmp_path):
    from montreal_forced_aligner_amd import ctm as C

    paths = segmenter.export_files(tmp_path, output_format="short_textgrid")
    assert [p.name for p in paths] == ["long.TextGrid", "half_rate.TextGrid"]
    for (name, pcm, rate), path in zip(segmenter.recordings, paths):
        duration = round(pcm.shape[0] / (rate or SR), 6)
        back = C.read_short_textgrid(path)
        assert list(back) == ["segments"]
        speech = [e for e in back["segments"] if e[2] != ""]
        segs = segmenter.segments[name]
        assert len(speech) == len(segs) and all(e[2] == "speech" for e in speech)
        for k, (e, s) in enumerate(zip(speech, segs)):
            assert e[0] == round(s.begin, 6)
            assert e[1] == round(s.end, 6) or (k == len(segs) - 1 and e[1] == duration)      # the writer's last-interval rule


def test_segments_align_with_the_fixture_model(engine, fx, segmenter):
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    utts = list(segmenter.utterances())
    assert len(utts) == sum(len(s) for s in segmenter.segments.values()) and {u.speaker for u in utts} == {"long", "half_rate"}
    for u in utts:
        u.text = "the"
        assert u.pcm.shape[0] > 0.3 * (u.sample_rate or SR) and u.begin >= 0 and u.file_duration > u.begin
    al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, options=AlignOptions(beam=100.0, retry_beam=400.0), engine=engine)
    res = al.align(utts)
    assert all(r is not None for r in res) and not al.failed
    assert all(r.num_frames > 30 for r in res)


@pytest.mark.parametrize("with_lda", [False, True])
def test_export_vad_then_feature_archive_equals_the_stages_by_hand(engine, fx, tmp_path, monkeypatch, with_lda):
    import torch

    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd import kalpy_api as KA

    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    engine.configure_mfcc(use_energy=1, raw_energy=0)
    pieces = {"s1-a": fx.pcm[: 4 * SR], "s1-b": fx.pcm[4 * SR: 9 * SR], "s2-quiet": np.zeros(2 * SR, dtype=np.int16), "s2-c": fx.pcm[9 * SR: 12 * SR]}
    d_pcm, so = engine.gather_pcm(list(pieces.values()))
    mfcc, fo = engine.mfcc(d_pcm, so)
    host = mfcc.cpu().numpy()
    feats = {k: host[fo[i]: fo[i + 1]] for i, k in enumerate(pieces)}
    K.write_table(tmp_path / "feats.ark", list(feats.items()), "matrix", tmp_path / "feats.scp")
    calls = []
    KA.VadComputer(energy_threshold=0.0, energy_mean_scale=1.0).export_vad(tmp_path / "vad.ark", list(feats.items()), write_scp=True, callback=calls.append)
    assert calls == [4]
    vads = dict(K.read_ark((tmp_path / "vad.ark").read_bytes(), "vector"))
    assert list(vads) == list(pieces) and all(vads[k].dtype == np.float32 and vads[k].shape == (feats[k].shape[0],) for k in pieces)
    assert vads["s2-quiet"].sum() == 0 and 0 < vads["s1-a"].sum() < len(vads["s1-a"])
    assert np.array_equal(KA.VadComputer(energy_threshold=0.0, energy_mean_scale=1.0).compute_vad(feats["s1-b"]), vads["s1-b"])
    assert [k for k, _, _ in K.read_scp(tmp_path / "vad.scp")] == list(pieces)
    kw = dict(deltas=True)
    lda = None
    if with_lda:
        lda = np.random.default_rng(4).standard_normal((40, 91)).astype(np.float32) * 0.1
        with open(tmp_path / "lda.mat", "wb") as f:
            f.write(b"\0B")
            K.write_matrix(f, lda)
        kw = dict(lda_mat_file_name=tmp_path / "lda.mat")
    got = dict(KA.FeatureArchive(tmp_path / "feats.scp", utt2spk={k: k.split("-")[0] for k in pieces}, vad_file_name=tmp_path / "vad.scp",
                                 subsample_n=2, use_sliding_cmvn=True, **kw))
    assert list(got) == ["s1-a", "s1-b", "s2-c"]                      # the utterance without a voiced frame is absent
    keep = [k for k in pieces if k != "s2-quiet"]
    fo2 = np.concatenate([[0], np.cumsum([feats[k].shape[0] for k in keep])]).astype(np.int64)
    d = torch.from_numpy(np.concatenate([feats[k] for k in keep])).to(engine.device)
    x = engine.sliding_cmvn(d, fo2, cmn_window=300, center=1, norm_vars=0)
    noop = torch.from_numpy(KA.FeatureArchive.noop_cmvn_rows(1, 13)).to(engine.device)
    x = engine.features(x, fo2, np.zeros(len(keep), dtype=np.int32), noop, lda=None if lda is None else torch.from_numpy(lda).to(engine.device))
    v = torch.from_numpy(np.concatenate([vads[k] for k in keep])).to(engine.device)
    x, fo3 = engine.select_frames(x, fo2, v, 2)
    x = x.cpu().numpy()
    for i, k in enumerate(keep):
        assert got[k].shape == ((int(vads[k].sum()) + 1) // 2, 40 if with_lda else 39)
        assert np.array_equal(got[k].view(np.uint32), x[fo3[i]: fo3[i + 1]].view(np.uint32))
