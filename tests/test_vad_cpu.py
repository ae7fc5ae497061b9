"""The speech-activity stage without a GPU: the plain restatement of tests/vad_ref.py pinned by answers worked by hand, the
host twins (csrc/vad_host.cpp over csrc/vad_math.hpp) against the restatement — bit for bit where the arithmetic is exact,
within derived bounds on real MFCCs —, the segmentation functions of montreal_forced_aligner_amd/segment.py on a corpus
worked by hand, FeatureArchive's option order on a host stand-in for the stages, and the twins' translation unit under the
host sanitizers as a stand-alone program (nothing is preloaded anywhere)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import frontend as F
from montreal_forced_aligner_amd import segment as S
from montreal_forced_aligner_amd.ctm import CtmInterval
from tests import vad_ref as R

ROOT = Path(__file__).resolve().parent.parent


def offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_vad_known_answers():
    fixed = dict(energy_threshold=5.0, energy_mean_scale=0.0)
    step = [0.0] * 5 + [10.0] * 5
    assert R.vad(step, frames_context=0, **fixed)[0].tolist() == [0] * 5 + [1] * 5
    # ctx 2 on the step: frame 4 sees 2 voiced of 5, frame 5 sees 3 of 5 — the exact tie below — and is voiced
    assert R.vad(step, frames_context=2, **fixed)[0].tolist() == [0] * 5 + [1] * 5
    spike = [0.0] * 4 + [10.0] + [0.0] * 4
    assert R.vad(spike, frames_context=0, **fixed)[0].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert R.vad(spike, frames_context=2, **fixed)[0].tolist() == [0] * 9                 # 1 of 5 (1 of 3 at the ends)
    dip = [10.0] * 4 + [0.0] + [10.0] * 4
    assert R.vad(dip, frames_context=2, **fixed)[0].tolist() == [1] * 9                   # 4 of 5 everywhere it matters
    # the threshold: 5 + 0.5 · mean
    out, thr = R.vad([2.0, 4.0, 12.0], 5.0, 0.5)
    assert thr == 8.0 and out.tolist() == [0, 0, 1]
    assert R.vad([], 5.0, 0.5)[1] == 5.0


def test_restatement_proportion_threshold_at_an_exact_tie():
    """3 voiced of 5 at 0.6: float32(0.6) · 5 lies exactly half way between 3.0 and the next float32 and rounds to even, 3.0, so
    3 >= 3.0 holds — the same float32 threshold multiplied in float64 is just above 3 and the frame would be silent.  Kaldi
    evaluates in float32."""
    assert float(np.float32(5) * np.float32(0.6)) == 3.0 and 5 * float(np.float32(0.6)) > 3.0
    e = [10.0, 10.0, 10.0, 0.0, 0.0]
    fixed = dict(energy_threshold=5.0, energy_mean_scale=0.0, frames_context=2)
    assert R.vad(e, proportion_threshold=0.6, **fixed)[0][2] == 1.0           # frame 2 sees all five frames, three voiced
    assert R.vad(e, proportion_threshold=0.61, **fixed)[0][2] == 0.0
    v, _, _ = F.vad_host(np.asarray(e, dtype=np.float32)[:, None], [0, 5], proportion_threshold=0.6, **fixed)
    assert v[2] == 1.0


def test_restatement_sliding_cmvn_known_answers():
    const = np.full((50, 3), 7.25)
    for center in (False, True):
        for nv in (False, True):
            assert np.array_equal(R.sliding_cmvn(const, 10, 4, center, nv), np.zeros((50, 3)))
    ramp = np.arange(40, dtype=np.float64)[:, None]
    out = R.sliding_cmvn(ramp, 4, 1, True)              # frames t − 2 … t + 1: mean t − 0.5
    assert np.array_equal(out[2:39, 0], np.full(37, 0.5))
    out = R.sliding_cmvn(ramp, 5, 1, True)              # frames t − 2 … t + 2: mean t
    assert np.array_equal(out[2:38, 0], np.zeros(36))
    # a window holding one frame: x − x, the factor 1
    assert np.array_equal(R.sliding_cmvn(np.array([[3.0, -2.0]]), 600, 100, False, True), np.zeros((1, 2)))
    assert np.array_equal(R.sliding_cmvn(np.array([[3.0], [5.0]]), 1, 1, True, True), np.zeros((2, 1)))


def test_restatement_window_rule_at_the_edges():
    w = lambda t, T, **o: R.cmn_window(t, T, **o)        # noqa: E731
    c = dict(cmn_window=4, min_window=2, center=True)
    assert [w(t, 10, **c) for t in (0, 1, 2, 5, 8, 9)] == [(0, 4), (0, 4), (0, 4), (3, 7), (6, 10), (6, 10)]     # T above the window
    assert [w(t, 4, **c) for t in range(4)] == [(0, 4)] * 4                                                      # T equal to it
    assert [w(t, 3, **c) for t in range(3)] == [(0, 3)] * 3                                                      # T below it
    n = dict(cmn_window=4, min_window=2, center=False)
    assert [w(t, 10, **n) for t in (0, 1, 2, 3, 4, 6, 9)] == [(0, 2), (0, 2), (0, 3), (0, 4), (0, 5), (2, 7), (5, 10)]
    assert w(0, 1, **n) == (0, 1)                                                                               # T below min_window
    assert [w(t, 2, **n) for t in range(2)] == [(0, 2), (0, 2)]                                                  # T equal to it
    big = dict(cmn_window=600, min_window=100, center=False)
    assert w(0, 50, **big) == (0, 50) and w(0, 100, **big) == (0, 100) and w(0, 101, **big) == (0, 100) and w(150, 1000, **big) == (0, 151)


# ---------------------------------------------------------------------------------------------- twin against restatement
def eighths(rng, T, D, lo=-40, hi=120):
    return (rng.integers(lo, hi, size=(T, D)) / 8.0).astype(np.float32)


def test_twin_equals_restatement_bit_for_bit_on_exact_data():
    """Multiples of 1/8 of this size: every float64 sum, in any order, is exact, so twin and restatement have to agree in
    every bit of all four outputs."""
    rng = np.random.default_rng(3)
    chunk = F._lib.lib().mfa_vad_sum_chunk_frames()
    lens = [0, 1, 2, 63, 64, 65, 257, 300, chunk + 5]
    fo = offs(lens)
    x = eighths(rng, int(fo[-1]), 4)
    for ctx in (0, 1, 2, 40, 5000):
        for o in (dict(energy_threshold=5.5, energy_mean_scale=0.5), dict(energy_threshold=0.0, energy_mean_scale=1.0)):
            vad, thr, voiced = F.vad_host(x, fo, frames_context=ctx, **o)
            for k in range(len(lens)):
                ref, ref_thr = R.vad(x[fo[k]: fo[k + 1], 0], o["energy_threshold"], o["energy_mean_scale"], ctx, 0.6)
                assert same_bits(np.float32(ref_thr), thr[k]) and same_bits(ref, vad[fo[k]: fo[k + 1]]), (ctx, k)
                assert voiced[k] == int(ref.sum())
    # runs, selection, scan
    vad = F.vad_host(x, fo, frames_context=1)[0]
    b, e, ro = F.vad_runs_host(vad, fo)
    for k in range(len(lens)):
        assert list(zip(b[ro[k]: ro[k + 1]].tolist(), e[ro[k]: ro[k + 1]].tolist())) == R.runs(vad[fo[k]: fo[k + 1]])
    for n in (1, 2, 3, 7):
        for v in (vad, None):
            out, oo = F.select_frames_host(x, fo, v, n)
            r_out, r_oo = R.select_batch(x, fo, v, n)
            assert same_bits(out, r_out) and same_bits(oo, r_oo)
    vals = rng.integers(0, 3, size=int(fo[-1])).astype(np.int32)
    scan, totals = F.vad_scan_host(vals, fo)
    r_scan, r_totals = R.scan(vals, fo)
    assert np.array_equal(scan, r_scan) and np.array_equal(totals, r_totals)
    # sliding CMVN: short utterances, windows below / at / above them, tile edges
    tile = F._lib.lib().mfa_sliding_cmvn_tile_frames()
    lens = [0, 1, 2, tile - 1, tile, tile + 1, 150]
    fo = offs(lens)
    x = eighths(rng, int(fo[-1]), 5, -200, 200)
    for window, min_window in ((1, 1), (2, 1), (64, 10), (150, 100), (600, 100)):
        for center in (0, 1):
            for nv in (0, 1):
                got = F.sliding_cmvn_host(x, fo, dim=3, cmn_window=window, min_window=min_window, center=center, norm_vars=nv)
                assert same_bits(got[:, 3:], x[:, 3:])
                for k in range(len(lens)):
                    ref = R.sliding_cmvn(x[fo[k]: fo[k + 1], :3], window, min_window, bool(center), bool(nv))
                    assert same_bits(ref.astype(np.float32), got[fo[k]: fo[k + 1], :3]), (window, center, nv, k)


@pytest.fixture(scope="module")
def golden_mfcc(fx):
    from tests import helpers

    return helpers.np_mfcc(fx.pcm, use_energy=1, raw_energy=0).astype(np.float32)


def test_twin_vad_equals_restatement_on_real_mfccs(golden_mfcc):
    x = golden_mfcc
    T = x.shape[0]
    e = x[:, 0].astype(np.float64)
    for o in (dict(energy_threshold=5.5, energy_mean_scale=0.5), dict(energy_threshold=0.0, energy_mean_scale=1.0)):
        # A float64 sum of T terms in any order is within T · 2^-53 · Σ|e| of the true sum, so the two means differ by at most
        # that (over T, times the scale <= 1), and one float32 rounding of the threshold adds half an ulp of it.  A frame
        # whose energy is further from the restatement's threshold than that gets the same decision from both.
        ref_thr = R.vad_threshold(e, **o)
        slack = T * 2.0 ** -53 * np.abs(e).sum() + 2.0 ** -23 * abs(ref_thr)
        assert np.abs(e - ref_thr).min() > slack, "an energy too close to the threshold: choose other inputs"
        for ctx in (0, 2, 40):
            vad, thr, voiced = F.vad_host(x, [0, T], frames_context=ctx, **o)
            ref, _ = R.vad(e, frames_context=ctx, proportion_threshold=0.6, **o)
            assert abs(float(thr[0]) - ref_thr) <= slack
            assert np.array_equal(vad, ref) and voiced[0] == int(ref.sum())
            if o["energy_mean_scale"] == 1.0:          # around the mean there are frames on both sides
                assert 0 < voiced[0] < T


def test_twin_sliding_cmvn_within_the_derived_bound_on_real_mfccs(golden_mfcc):
    x = golden_mfcc[:700]
    tile = F._lib.lib().mfa_sliding_cmvn_tile_frames()
    M = float(np.abs(x).max())
    for window, center in ((300, 1), (600, 0), (64, 1)):
        got = F.sliding_cmvn_host(x, [0, x.shape[0]], cmn_window=window, center=center).astype(np.float64)
        ref = R.sliding_cmvn(x, window, 100, bool(center))
        # The restatement's sums are exact (fsum).  The twin's running sum has seen at most ops = window + 1 + 2 · tile float64
        # additions and subtractions, each of a partial sum no larger than ops · M: its error is below ops² · M · 2^-53, and the
        # mean's (a division by n >= 1, one more rounding of a value <= M) below that + M · 2^-53; the subtraction adds
        # 2^-53 · 2M.  Then the one float32 rounding of the output: 2^-24 of its size.
        ops = window + 1 + 2 * tile
        bound = (ops * ops + 3) * M * 2.0 ** -53 + 2.0 ** -24 * np.abs(ref)
        assert (np.abs(got - ref) <= bound).all()
        assert np.abs(got - ref).max() > 0 or window == 1


# ---------------------------------------------------------------------------------------------- segmentation
def ivs(segments):
    return [(s.begin, s.end) for s in segments]


def test_initial_segmentation_and_merge_on_a_corpus_worked_by_hand():
    fs = 0.01
    # the two end-time rules: an interior run ends at the START of its last voiced frame, the last run at the file's end
    seg = S.get_initial_segmentation(np.array([0, 1, 1, 1, 0, 0, 1, 1], dtype=np.float32), fs)
    assert ivs(seg) == [(1 * fs, 3 * fs), (6 * fs, 8 * fs)] and all(s.label == "speech" for s in seg)
    assert ivs(S.get_initial_segmentation(np.array([1, 0], dtype=np.float32), fs)) == [(0.0, 0.0)]       # one frame: empty
    assert S.get_initial_segmentation(np.zeros(5, dtype=np.float32), fs) == []
    iv = lambda *p: [CtmInterval(b, e, "speech") for b, e in p]       # noqa: E731
    mp, mx, mn = 0.333, 30.0, 0.333
    # a pause below min_pause_duration joins, one above it stays a boundary
    assert ivs(S.merge_segments(iv((0, 1), (1.2, 2)), mp, mx, mn)) == [(0, 2)]
    got = ivs(S.merge_segments(iv((0, 1), (1.5, 2)), mp, mx, mn))          # gap 0.5 >= mp / 2: both sides move mp / 4
    assert got == [pytest.approx((0, 1 + mp / 4)), pytest.approx((1.5 - mp / 4, 2))]
    assert ivs(S.merge_segments(iv((0, 1), (1.5, 2)), mp, mx, mn, snap_boundaries=False)) == [(0, 1), (1.5, 2)]
    # max_segment_length splits although the pause is short; gap 0.1 < mp / 2: both sides move half the gap and meet
    got = ivs(S.merge_segments(iv((0, 20), (20.1, 35)), mp, mx, mn))
    assert got == [pytest.approx((0, 20.05)), pytest.approx((20.05, 35))]
    assert ivs(S.merge_segments(iv((0, 20), (20.1, 29)), mp, mx, mn)) == [(0, 29)]
    # three in a row: the first two join, the third would exceed the maximum (gap 0.2 >= mp / 2: mp / 4 each side)
    got = ivs(S.merge_segments(iv((0, 14), (14.2, 28), (28.2, 40)), mp, mx, mn))
    assert got == [pytest.approx((0, 28 + mp / 4)), pytest.approx((28.2 - mp / 4, 40))]
    # the filter comes last, after snapping: 0.2 + mp / 4 is still below the minimum, 0.3 + mp / 4 is not
    got = ivs(S.merge_segments(iv((0, 0.2), (1, 3)), mp, mx, mn))
    assert got == [pytest.approx((1 - mp / 4, 3))]
    got = ivs(S.merge_segments(iv((0, 0.3), (1, 3)), mp, mx, mn))
    assert got == [pytest.approx((0, 0.3 + mp / 4)), pytest.approx((1 - mp / 4, 3))]
    assert S.merge_segments([], mp, mx, mn) == []


def test_segments_from_runs_equals_the_frame_walk():
    rng = np.random.default_rng(5)
    vectors = [np.zeros(7), np.ones(9), np.zeros(1), np.ones(1), np.array([1, 0, 0, 1]), np.array([1, 1, 0, 1, 1])]
    while len(vectors) < 200:
        n = int(rng.integers(1, 80))
        vectors.append((rng.random(n) < rng.random()).astype(np.float64))
    fo = offs([len(v) for v in vectors])
    flat = np.concatenate(vectors).astype(np.float32)
    b, e, ro = F.vad_runs_host(flat, fo)
    for k, v in enumerate(vectors):
        want = S.get_initial_segmentation(v.astype(np.float32), 0.01)
        got = S.segments_from_runs(b[ro[k]: ro[k + 1]], e[ro[k]: ro[k + 1]], len(v), 0.01)
        assert ivs(got) == ivs(want) and all(s.label == "speech" for s in got)
        rr = R.runs(v)
        assert ivs(S.segments_from_runs([r[0] for r in rr], [r[1] for r in rr], len(v), 0.01)) == ivs(want)


# ---------------------------------------------------------------------------------------------- FeatureArchive's order
class HostStages:
    """The engine's stage methods on CPU tensors: the twins for the new stages, a stand-in for the feature kernel that does not
    commute with any of them (it subtracts the CMVN mean and appends the difference of a frame's two neighbours)."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def sliding_cmvn(self, d, fo, **o):
        import torch

        self.calls.append(("sliding_cmvn", o))
        return torch.from_numpy(F.sliding_cmvn_host(d.numpy(), fo, **o))

    def features(self, d, fo, u2s, cm, lda=None, fmllr=None, splice_context=3):
        import torch

        self.calls.append(("features", None if cm is None else cm.numpy().copy()))
        x = d.numpy().astype(np.float64)
        outs = []
        for k in range(len(fo) - 1):
            u = x[fo[k]: fo[k + 1]]
            if cm is not None:
                st = cm.numpy()[u2s[k]]
                u = u - st[0, :-1] / st[0, -1]
            pad = np.concatenate([u[:1], u, u[-1:]])
            outs.append(np.concatenate([u, pad[2:] - pad[:-2]], axis=1))
        return torch.from_numpy(np.concatenate(outs).astype(np.float32))

    def select_frames(self, d, fo, vad=None, subsample_n=1):
        import torch

        self.calls.append(("select_frames", subsample_n))
        out, oo = F.select_frames_host(d.numpy(), fo, None if vad is None else vad.numpy(), subsample_n)
        return torch.from_numpy(np.ascontiguousarray(out)), oo


def test_feature_archive_applies_the_options_in_the_documented_order(tmp_path, caplog):
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd import kalpy_api as KA

    rng = np.random.default_rng(8)
    lens = dict(a=120, b=400, c=50, d=30, e=20)
    feats = {k: eighths(rng, n, 3) for k, n in lens.items()}
    vads = {k: (rng.random(n) < 0.7).astype(np.float32) for k, n in lens.items()}
    vads["c"][:] = 0.0                                   # nothing voiced
    vads["d"] = vads["d"][:-1]                           # another length than the features
    del vads["e"]                                        # no vector at all
    cmvn = np.zeros((2, 4)); cmvn[0] = [30.0, -60.0, 90.0, 10.0]
    K.write_table(tmp_path / "feats.ark", list(feats.items()), "matrix", tmp_path / "feats.scp")
    K.write_table(tmp_path / "vad.ark", list(vads.items()), "vector", tmp_path / "vad.scp")
    K.write_table(tmp_path / "cmvn.ark", [("spk", cmvn)], "matrix")
    u2s = {k: "spk" for k in lens}
    common = dict(utt2spk=u2s, cmvn_file_name=tmp_path / "cmvn.ark", deltas=True)

    st = HostStages()
    with caplog.at_level("WARNING", logger="kalpy.align"):
        got = dict(KA.FeatureArchive(tmp_path / "feats.scp", vad_file_name=tmp_path / "vad.scp", subsample_n=2, use_sliding_cmvn=True,
                                     stages=st, **common))
    assert [c[0] for c in st.calls] == ["sliding_cmvn", "features", "select_frames"]
    assert st.calls[0][1] == dict(cmn_window=300, center=1, norm_vars=0)
    assert np.array_equal(st.calls[1][1], KA.FeatureArchive.noop_cmvn_rows(1, 3))      # sliding CMVN replaces the speaker's
    assert sorted(got) == ["a", "b"]                                                  # c, d, e are skipped, each with a warning
    assert sum(("utterance " + k) in caplog.text for k in "cde") == 3
    # the chain by hand, in the documented order and in two others that give something else
    h = HostStages()
    import torch

    def chain(order, k):
        x, fo, v = torch.from_numpy(feats[k]), offs([lens[k]]), vads[k]
        for step in order:
            if step == "cmvn":
                x = h.sliding_cmvn(x, fo, cmn_window=300, center=1, norm_vars=0)
            elif step == "deltas":
                x = h.features(x, fo, [0], None)
            else:
                x, fo = h.select_frames(x, fo, torch.from_numpy(v), 2)
                v = np.ones(int(fo[-1]), dtype=np.float32)
        return x.numpy()

    for k in ("a", "b"):
        assert same_bits(got[k], chain(("cmvn", "deltas", "select"), k))
        assert not np.array_equal(got[k], chain(("cmvn", "select", "deltas"), k))
        assert not np.array_equal(got[k], chain(("deltas", "cmvn", "select"), k))
        assert got[k].shape == ((int(vads[k].sum()) + 1) // 2, 6)

    # without sliding CMVN the speaker's statistics reach the feature stage, and nothing is selected unless asked for
    st = HostStages()
    plain = dict(KA.FeatureArchive(tmp_path / "feats.scp", stages=st, **common))
    assert [c[0] for c in st.calls] == ["features"] and np.array_equal(st.calls[0][1][0], cmvn)
    assert sorted(plain) == sorted(lens) and plain["a"].shape == (120, 6)
    st = HostStages()
    sub = dict(KA.FeatureArchive(tmp_path / "feats.scp", subsample_n=3, stages=st, **common))
    assert [c[0] for c in st.calls] == ["features", "select_frames"]
    assert all(same_bits(sub[k], plain[k][::3]) for k in lens)
    with pytest.raises(NotImplementedError):
        KA.FeatureArchive(tmp_path / "feats.scp", subsample_n=-2, **common)


def test_vad_options_are_named_and_refused_like_the_others():
    x = np.zeros((4, 2), dtype=np.float32)
    with pytest.raises(KeyError):
        F.vad_host(x, [0, 4], energy_treshold=5.0)
    with pytest.raises(F._lib.MfaHipError):
        F.sliding_cmvn_host(x, [0, 4], cmn_window=0)
    with pytest.raises(F._lib.MfaHipError):
        F.select_frames_host(x, [0, 4], None, 0)
    assert F.vad_host(x, [0, 4], vad_energy_threshold=-1.0, energy_mean_scale=0.0)[2][0] == 4     # Kaldi's option names too


# ---------------------------------------------------------------------------------------------- sanitizers
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "vad_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "vad_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "vad_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
