"""CPU tests of the pitch tracker's restatement (tests/pitch_ref.py) and of the library's host side (pitch_plan.cpp,
resample_plan.cpp).  Kaldi's pitch extractor is not among this project's references, so the restatement is pinned by what a
pitch tracker has to do — follow a harmonic tone and a chirp, call noise unvoiced — and the host tables the kernels read are
then held to the restatement's, rounded once to float32.  tests/test_gpu_pitch.py checks the kernels against the same file."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import pitch_ref as R

FS = 16000
MFA = R.Opts()                     # MFA's option set: max_f0 800, snip_edges True


def harmonic(f0, dur=1.0, amp=8000.0, partials=5):
    t = np.arange(int(round(dur * FS))) / FS
    f0 = np.broadcast_to(np.asarray(f0, dtype=np.float64), t.shape)
    phase = 2.0 * math.pi * np.cumsum(f0) / FS
    x = sum(np.sin((k + 1) * phase) / (k + 1) for k in range(partials))
    return np.round(x / np.abs(x).max() * amp).astype(np.int16)


def buzz(f0, dur, partials, amp=8000.0):
    """Partials 1 .. ``partials`` of f0 (a number or one value per sample) with amplitudes growing as k^2: a pulse-like source
    whose energy sits in its highest harmonics."""
    t = np.arange(int(round(dur * FS))) / FS
    phase = 2.0 * math.pi * np.cumsum(np.broadcast_to(np.asarray(f0, dtype=np.float64), t.shape)) / FS
    x = sum(np.sin(k * phase) * k * k for k in range(1, partials + 1))
    return np.round(x / np.abs(x).max() * amp).astype(np.int16)


def margin_inputs():
    """The tone and the chirp of the float64 check of the state path (tests/test_gpu_pitch.py): 70 Hz for 1 s with 27
    partials, and 55 -> 65 Hz over 2 s with 30 partials (33 state changes), both reaching 1.9 kHz — the band edge of the 4 kHz
    signal the tracker works on, so nothing aliases.  Why these: the check compares the device's path with a float64 argmin
    where the best predecessor leads the second-best by more than 1e-4, and needs 90 % of the frames to be such.  With
    nccf_ballast 7000 the pitch NCCF of a steady signal is the plain NCCF / sqrt(1 + 7000) = NCCF / 84, so the forward
    costs around the peak curve by (NCCF curvature) / 84 per state^2: 1e-5 for a tone of five partials — no frame qualifies —
    and 1e-3 once the peak is as narrow as the band allows, which takes a low pitch (a state is 0.5 % of the lag) and
    strong high harmonics.  During a glide the two best predecessors tie whenever the pitch crosses the middle between two
    states; that takes 3.5 % of the chirp's frames."""
    return [buzz(70.0, 1.0, 27), buzz(np.linspace(55.0, 65.0, 2 * FS), 2.0, 30)]


def _lib():
    from montreal_forced_aligner_amd import _lib as L

    L.build_native()
    return L


def lib_opts(L, o: R.Opts, **kw):
    d = dict(sample_frequency=o.sample_frequency, frame_length_ms=o.frame_length, frame_shift_ms=o.frame_shift, min_f0=o.min_f0,
             max_f0=o.max_f0, soft_min_f0=o.soft_min_f0, penalty_factor=o.penalty_factor, lowpass_cutoff=o.lowpass_cutoff,
             resample_frequency=o.resample_frequency, delta_pitch=o.delta_pitch, nccf_ballast=o.nccf_ballast, preemphasis=0.0,
             pov_scale=o.pov_scale, pov_offset=o.pov_offset, pitch_scale=o.pitch_scale,
             lowpass_filter_width=o.lowpass_filter_width, upsample_filter_width=o.upsample_filter_width,
             snip_edges=int(o.snip_edges), normalization_context=o.normalization_context, add_pov_feature=int(o.add_pov_feature),
             add_normalized_log_pitch=int(o.add_normalized_log_pitch), add_raw_log_pitch=int(o.add_raw_log_pitch), add_delta_pitch=0)
    d.update(kw)
    return L.PitchOpts(**d)


def host_tables(L, opts):
    """The library's host tables for an option set (mfa_debug_pitch_stages without a context), or None when refused."""
    lib = L.lib()
    sizes = np.zeros(8, dtype=np.int32)
    nul = [None] * 6
    tail = [None, None, None, None, None, 0, 0, None, None, None, None, None, None]
    if lib.mfa_debug_pitch_stages(None, C.byref(opts), sizes.ctypes.data, *nul, *tail) != 0:
        return None
    S, taps = int(sizes[0]), int(sizes[3])
    lags, sml, pen = (np.zeros(S, dtype=np.float32) for _ in range(3))
    first, ntap = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    w = np.zeros((S, taps), dtype=np.float32)
    assert lib.mfa_debug_pitch_stages(None, C.byref(opts), sizes.ctypes.data, lags.ctypes.data, sml.ctypes.data, pen.ctypes.data,
                                      first.ctypes.data, ntap.ctypes.data, w.ctypes.data, *tail) == 0
    return dict(sizes=sizes, lags=lags, sml=sml, pen=pen, first=first, taps=ntap, w=w)


# ------------------------------------------------------------------------------------------ what a tracker has to do
@pytest.fixture(scope="module")
def tone_runs():
    return {f0: R.compute(harmonic(float(f0)), MFA) for f0 in (80, 120, 220, 440)}


@pytest.mark.parametrize("f0", [80, 120, 220, 440])
def test_harmonic_tone_is_tracked(tone_runs, f0):
    """Interior frames within 1 % of f0 (half the 0.5 % lag grid plus interpolation error) and clearly voiced."""
    raw = tone_runs[f0]["raw"][5:-5]
    assert raw.shape[0] > 80
    err = np.abs(raw[:, 1] / f0 - 1.0).max()
    print(f"f0 {f0}: worst relative pitch error {err:.5f}, smallest POV NCCF {raw[:, 0].min():.4f}")
    assert err < 0.01
    assert raw[:, 0].min() > 0.9


def test_white_noise_is_unvoiced(tone_runs):
    x = harmonic(120.0)
    rms = math.sqrt(float((x.astype(np.float64) ** 2).mean()))
    noise = np.round(np.random.default_rng(0).standard_normal(FS) * rms).astype(np.int16)
    pov = R.compute(noise, MFA)["raw"][:, 0]
    tone = tone_runs[120]["raw"][:, 0]
    print(f"mean POV NCCF: noise {pov.mean():.4f}, tone {tone.mean():.4f}")
    assert pov.mean() < 0.5 and pov.mean() < tone.mean() - 0.4


def test_chirp_is_tracked_monotonically():
    dur = 2.0
    f = np.linspace(100.0, 200.0, int(dur * FS))
    raw = R.compute(harmonic(f, dur), MFA)["raw"][5:-5]
    tb = R.tables(MFA)
    centre = (np.arange(5, 5 + raw.shape[0]) * tb.shift + tb.N / 2.0) / MFA.resample_frequency     # window centres, seconds
    truth = 100.0 + 100.0 * centre / dur
    err = np.abs(raw[:, 1] / truth - 1.0).max()
    print(f"chirp: worst relative pitch error {err:.5f}")
    assert err < 0.02
    assert np.all(np.diff(raw[:, 1]) >= 0.0)


def test_margin_inputs_have_clear_float64_margins():
    """The restatement alone, before any device is asked: on both inputs at least 90 % of the frames have a float64 margin
    above 1e-4 between the best and second-best predecessor of the chosen state, the float32 chain's path is the float64
    one, and the pitch is tracked."""
    tb = R.tables(MFA)
    for x, (lo, hi) in zip(margin_inputs(), ((70.0, 70.0), (55.0, 65.0))):
        r = R.compute(x, MFA, chain=True)
        path64, margin = R.viterbi(r["nccf_pitch"], MFA, chain=False, want_margin=True)
        share = float((margin > 1e-4).mean())
        print(f"{lo:g} -> {hi:g} Hz: {100 * share:.1f} % of the frames above 1e-4 (median {np.median(margin):.2e})")
        assert share >= 0.9
        assert np.array_equal(r["path"], path64)
        f = 1.0 / tb.lags[path64[5:-5]]
        assert abs(f[0] / lo - 1.0) < 0.03 and abs(f[-1] / hi - 1.0) < 0.03 and np.all(np.diff(f) >= 0.0)


def test_all_zero_signal():
    r = R.compute(np.zeros(FS // 2, dtype=np.int16), MFA)
    assert r["raw"].shape[0] == R.num_frames(FS // 2, MFA) > 0
    assert np.all(r["nccf_pitch"] == 0.0) and np.all(r["nccf_pov"] == 0.0)
    out = R.process(r["raw"], MFA)
    assert np.all(np.isfinite(r["raw"])) and np.all(np.isfinite(out))
    rc = R.compute(np.zeros(FS // 2, dtype=np.int16), MFA, chain=True)
    assert np.all(rc["nccf_pitch"] == 0.0) and np.array_equal(rc["path"], r["path"])


def test_fmaf32_is_a_correctly_rounded_fma():
    """Against exact rational arithmetic, on operands chosen to land on and next to float32 rounding ties."""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    a[:8] = np.float32(1.0) + np.float32(2.0 ** -12); b[:8] = np.float32(1.0) + np.float32(2.0 ** -12)    # 1 + 2^-11 + 2^-24
    c[:8] = np.array([0.0, 2.0 ** -40, -(2.0 ** -40), 2.0 ** -24, -(2.0 ** -24), 1.0, -1.0, 2.0 ** -60], dtype=np.float32)
    got = R.fmaf32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        assert abs(Fraction(g) - exact) <= abs(Fraction(float(lo)) - exact) and abs(Fraction(g) - exact) <= abs(Fraction(float(hi)) - exact)
        if abs(Fraction(g) - exact) == abs(Fraction(float(lo)) - exact) or abs(Fraction(g) - exact) == abs(Fraction(float(hi)) - exact):
            assert (np.float32(g).view(np.uint32) & 1) == 0          # a tie goes to the even neighbour


# ------------------------------------------------------------------------------------------ sizes and frame counts
def test_state_counts_and_measured_lags():
    assert R.tables(MFA).S == 556 and R.tables(R.replace(MFA, max_f0=400.0)).S == 417
    assert (R.tables(MFA).first, R.tables(MFA).last) == (3, 82)
    L = _lib()
    for o, S in ((MFA, 556), (R.replace(MFA, max_f0=400.0), 417)):
        t = host_tables(L, lib_opts(L, o))
        assert int(t["sizes"][0]) == S and tuple(t["sizes"][1:3]) == (R.tables(o).first, R.tables(o).last)
        assert tuple(t["sizes"][4:6]) == (100, 40)


@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts(snip):
    """n resampled samples, N = 100, shift = 40: 0 below one window; then (n - N) // shift + 1 with snip_edges and
    int(n / shift + 0.5) without — stated from the resampled length, which is ceil(samples / 4) at 16 kHz -> 4 kHz."""
    o = R.replace(MFA, snip_edges=snip)
    for samples in (0, 1, 160, 396, 397, 399, 400, 401, 479, 480, 481, 556, 557, 560, 561, 639, 640, 641, 15999, 16000, 16001, 16081):
        n = -(-samples // 4)
        assert R.tables(o).rs.num_out(samples) == n
        want = 0 if n < 100 else ((n - 100) // 40 + 1 if snip else int(n / 40 + 0.5))
        assert R.num_frames(samples, o) == want, samples
    # the MFCC's count (round(samples / 160) without snip_edges, 1 + (samples - 400) // 160 with) is never more than one away
    # once the utterance holds a window
    for samples in range(400, 4000, 7):
        mfcc = 1 + (samples - 400) // 160 if snip else (samples + 80) // 160
        assert abs(R.num_frames(samples, o) - mfcc) <= 1, samples


# ------------------------------------------------------------------------------------------ the library's host side
@pytest.mark.parametrize("o", [MFA, R.replace(MFA, max_f0=400.0), R.replace(MFA, snip_edges=False, min_f0=60.0, delta_pitch=0.01),
                               R.replace(MFA, sample_frequency=22050.0), R.replace(MFA, sample_frequency=8000.0, upsample_filter_width=3)],
                         ids=["mfa", "max400", "coarse", "22050", "8000"])
def test_host_tables_equal_the_restatement(o):
    L = _lib()
    t, tb = host_tables(L, lib_opts(L, o)), R.tables(o)
    assert t is not None and int(t["sizes"][0]) == tb.S and int(t["sizes"][3]) == tb.up_max_taps
    assert np.array_equal(t["lags"], tb.lags32) and np.array_equal(t["sml"], tb.sml32) and np.array_equal(t["pen"], tb.pen32)
    assert np.array_equal(t["first"], tb.up_first) and np.array_equal(t["taps"], tb.up_taps)
    assert np.array_equal(t["w"], tb.up_w32)
    assert (int(t["sizes"][6]), int(t["sizes"][7])) == (tb.rs.phases, tb.rs.max_taps)
    # every up-sampling filter interpolates a constant to (nearly) itself away from the clipped ends
    inner = (tb.up_first > 0) & (tb.up_first + tb.up_taps < tb.L)
    assert np.abs(tb.up_w[inner].sum(axis=1) - 1.0).max() < 0.02


def test_refusals_on_the_host():
    L = _lib()
    assert host_tables(L, lib_opts(L, MFA)) is not None
    for kw in (dict(add_delta_pitch=1), dict(max_f0=1950.0), dict(min_f0=800.0), dict(min_f0=900.0), dict(min_f0=0.0),
               dict(preemphasis=0.5), dict(delta_pitch=0.0005), dict(lowpass_cutoff=2000.0), dict(resample_frequency=4000.5),
               dict(add_pov_feature=0, add_normalized_log_pitch=0, add_raw_log_pitch=0)):
        assert host_tables(L, lib_opts(L, MFA, **kw)) is None, kw


def general_plan(lib, fin, fout, fc, zeros):
    ph, ipu, mt = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert lib.mfa_resample_plan_general(fin, fout, fc, zeros, C.byref(ph), C.byref(ipu), C.byref(mt), None, None, None) == 0
    first, taps = np.zeros(ph.value, dtype=np.int32), np.zeros(ph.value, dtype=np.int32)
    w = np.zeros((ph.value, mt.value), dtype=np.float32)
    assert lib.mfa_resample_plan_general(fin, fout, fc, zeros, None, None, None, first.ctypes.data, taps.ctypes.data, w.ctypes.data) == 0
    return ph.value, ipu.value, first, taps, w


@pytest.mark.parametrize("fin", [44100, 48000, 8000, 12345])
def test_general_plan_reproduces_the_mfcc_plan_bit_for_bit(fin):
    lib = _lib().lib()
    ph, ipu, mt = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert lib.mfa_resample_plan(fin, FS, C.byref(ph), C.byref(ipu), C.byref(mt), None, None, None) == 0
    first, taps = np.zeros(ph.value, dtype=np.int32), np.zeros(ph.value, dtype=np.int32)
    w = np.zeros((ph.value, mt.value), dtype=np.float32)
    assert lib.mfa_resample_plan(fin, FS, None, None, None, first.ctypes.data, taps.ctypes.data, w.ctypes.data) == 0
    g = general_plan(lib, fin, FS, 0.99 * 0.5 * float(min(fin, FS)), 6)
    assert (g[0], g[1]) == (ph.value, ipu.value)
    assert np.array_equal(g[2], first) and np.array_equal(g[3], taps) and g[4].tobytes() == w.tobytes()


def test_general_plan_of_the_pitch_down_sampler():
    lib = _lib().lib()
    ph, ipu, first, taps, w = general_plan(lib, FS, 4000, 1000.0, 1)
    p = R.tables(MFA).rs
    assert (ph, ipu) == (1, 4) == (p.phases, p.in_per_unit)
    assert first.tolist() == p.first and taps.tolist() == p.taps
    assert np.array_equal(w[0, : taps[0]], p.w[0].astype(np.float32))
    # centre tap 2 fc / fin, symmetric, and (one zero crossing only: the Hann window eats into the main lobe) a DC gain of 0.815
    assert p.w[0][8] == 2.0 * 1000.0 / FS and np.allclose(p.w[0], p.w[0][::-1], rtol=0, atol=1e-17)
    assert 0.8 < float(p.w[0].sum()) < 0.83
    assert lib.mfa_resample_plan_general(FS, 4000, 2000.0, 1, None, None, None, None, None, None) < 0     # cutoff at Nyquist
    assert lib.mfa_resample_plan_general(FS, 4000, 1000.0, 0, None, None, None, None, None, None) < 0


# ------------------------------------------------------------------------------------------ ProcessPitch
def test_post_processing_at_hand_computed_points():
    o = R.replace(MFA, add_raw_log_pitch=True)
    raw = np.array([[-1.0, 100.0], [0.0, 200.0], [1.0, 400.0]])
    out = R.process(raw, o)
    # POV feature 2 ((1.0001 - n)^0.15 - 1): n = -1, 0, 1
    want = [2.0 * (2.0001 ** 0.15 - 1.0), 2.0 * (1.0001 ** 0.15 - 1.0), 2.0 * (0.0001 ** 0.15 - 1.0)]
    assert np.allclose(out[:, 0], want, rtol=0, atol=1e-12)              # (1.0001 - 1 is not the double 0.0001)
    assert abs(out[2, 0] - (-1.4976227)) < 1e-5 and abs(out[0, 0] - 0.2191556) < 1e-5    # 2 (10^-0.6 - 1), 2 (2.0001^0.15 - 1)
    # POV weights: a = |n| clipped; sigma(-5.2 + 5.4 e^{-7.5} - 2 + 4.2 e^{-20}) at a = 0, sigma(-5.2 + 5.4 + 4.8 - 2 e^{-10} + 4.2) at 1
    p0 = 1.0 / (1.0 + math.exp(-(-5.2 + 5.4 * math.exp(-7.5) - 2.0 + 4.2 * math.exp(-20.0))))
    p1 = 1.0 / (1.0 + math.exp(-(-5.2 + 5.4 + 4.8 - 2.0 * math.exp(-10.0) + 4.2)))
    p = R.pov_weight(raw[:, 0])
    assert np.allclose(p, [p1, p0, p1], rtol=1e-15, atol=0)
    lf = np.log(raw[:, 1])
    mean = float((p * lf).sum() / p.sum())                                       # one window covers all three frames
    assert np.allclose(out[:, 1], 2.0 * (lf - mean), rtol=0, atol=1e-14)
    assert np.array_equal(out[:, 2], lf)
    # a one-frame utterance: the weighted mean is the frame's own log-pitch
    one = R.process(np.array([[0.3, 150.0]]), o)
    assert one.shape == (1, 3) and one[0, 1] == 0.0 and one[0, 2] == math.log(150.0)
    # the window is clipped, not the whole utterance: context 1 on three frames
    o1 = R.replace(o, normalization_context=1)
    m0 = float((p[:2] * lf[:2]).sum() / p[:2].sum())
    assert abs(R.process(raw, o1)[0, 1] - 2.0 * (lf[0] - m0)) < 1e-14
    # columns by flag
    assert R.process(raw, R.replace(MFA, add_pov_feature=False)).shape == (3, 1)
    assert R.process(raw, R.replace(MFA, add_normalized_log_pitch=False, add_raw_log_pitch=True)).shape == (3, 2)


def test_abi_lists_the_pitch_entry_points():
    L = _lib()
    lib = L.lib()
    names = {"mfa_pitch_configure", "mfa_pitch_num_frames", "mfa_pitch_num_states", "mfa_pitch_num_columns", "mfa_pitch_workspace_bytes",
             "mfa_pitch_batch", "mfa_pitch_process_batch", "mfa_debug_pitch_stages", "mfa_resample_plan_general"}
    assert names <= set(L.SIGNATURES) and all(hasattr(lib, n) for n in names)
    assert lib.mfa_version() >= 2
    assert C.sizeof(L.PitchOpts) == 23 * 4


def test_paste_frame_offsets_min_rule_and_refusal():
    """Host only: min(mfcc, pitch) rows when the counts differ by at most one, either way; anything more is refused."""
    from montreal_forced_aligner_amd._lib import MfaHipError
    from montreal_forced_aligner_amd.engine import AlignmentEngine

    mfo = np.array([0, 1, 299, 299, 305, 306], dtype=np.int64)            # 1, 298, 0, 6, 1
    pfo = np.array([0, 2, 300, 300, 305, 305], dtype=np.int64)            # 2, 298, 0, 5, 0
    out = AlignmentEngine.paste_frame_offsets(mfo, pfo)
    assert out.dtype == np.int64 and np.diff(out).tolist() == [1, 298, 0, 5, 0]
    with pytest.raises(MfaHipError, match="utterance 1: 3 MFCC frames and 1 pitch frames differ by more than 1"):
        AlignmentEngine.paste_frame_offsets(np.array([0, 4, 7]), np.array([0, 4, 5]))
    with pytest.raises(MfaHipError, match="utterance 0"):
        AlignmentEngine.paste_frame_offsets(np.array([0, 2]), np.array([0, 4]))


def test_kalpy_paste_feats():
    from montreal_forced_aligner_amd import kaldi_io, kalpy_api as KA

    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = np.arange(10, dtype=np.float64).reshape(5, 2)
    both = KA.paste_feats([a, b], 1)
    assert both.dtype == np.float32 and both.shape == (4, 5)
    assert np.array_equal(both[:, :3], a) and np.array_equal(both[:, 3:], b[:4])
    assert np.array_equal(KA.paste_feats([b, a], 1), np.concatenate([b[:4], a], axis=1).astype(np.float32))
    assert KA.paste_feats([a, a]).shape == (4, 6)
    with pytest.raises(kaldi_io.KaldiFormatError):
        KA.paste_feats([a, b], 0)
    with pytest.raises(kaldi_io.KaldiFormatError):
        KA.paste_feats([a, b[:2]], 1)


def test_pitch_options_of_a_model():
    """use_pitch adds the normalised log-pitch — the raw one with normalize_pitch off —, use_voicing the POV feature,
    use_delta_pitch the delta-pitch (which the engine then refuses); the rest are the model's values or MFA's defaults."""
    from montreal_forced_aligner_amd.model import pitch_options

    base = dict(frame_shift=10, frame_length=25, min_f0=50, max_f0=800, sample_frequency=16000, penalty_factor=0.1, delta_pitch=0.005,
                snip_edges=True)
    off = dict(add_normalized_log_pitch=False, add_delta_pitch=False, add_pov_feature=False)
    assert pitch_options({}) == pitch_options({"features": {}}) == dict(base, **off)
    assert pitch_options({"features": {"use_pitch": True}}) == dict(base, **dict(off, add_normalized_log_pitch=True, add_raw_log_pitch=False))
    assert pitch_options({"features": {"use_pitch": True, "normalize_pitch": False, "use_voicing": True, "max_f0": 400, "snip_edges": False}}) == \
        dict(base, max_f0=400, snip_edges=False, add_normalized_log_pitch=False, add_raw_log_pitch=True, add_delta_pitch=False, add_pov_feature=True)
    assert pitch_options({"features": {"use_voicing": True, "use_delta_pitch": True, "normalize_pitch": False}}) == \
        dict(base, add_normalized_log_pitch=False, add_delta_pitch=True, add_pov_feature=True)
