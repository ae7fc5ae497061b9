"""GPU tests of the front end away from MFA's operating point (16 kHz, 25 ms / 10 ms, 23 bins, 13 cepstra, ±3 splice, 91→40):
every option of mfa_mfcc_configure, every window class of both mfcc_kernel instantiations, the generic feature kernel, the
delta kernel on utterances shorter than its halo, CMVN statistics with empty speakers, and the front-end fuzzer's batches
at fixed seeds.  Every comparison is against the oracle on the same inputs (oracle.oracle; oracle.np_oracle in float64
stands behind it in tests/test_oracle_cpu.py at the same options and shapes) — the device is compared with itself only where
bit-identity of two device paths is the claim."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import _lib
from oracle import oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu

GRID = helpers.mfcc_option_grid()
SPEECH_BAR, FULL_SCALE_BAR = 2e-3, 5e-3      # tests/test_gpu_parity.py: test_mfcc_matches_oracle, …_digital_silence_and_full_scale
T_LIST = [1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 127, 128, 129, 300]     # every clamp combination, both tile sizes (64, 128)
LDA_SHAPES = [(13, 3, 39), (13, 2, 40), (13, 4, 40), (12, 3, 40), (16, 3, 40), (16, 1, 24), (13, 0, 13), (8, 3, 64)]


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _offsets(arrays):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)


def _matrix_audio(fx):
    """(kind, int16) blocks of the option matrix, in batch order.  The odd-length constant puts everything after it at an
    odd sample offset: the first speech block runs on the aligned fast path, the last one sample by sample (and, with an
    odd shift, on both in turn).  −32768 × 512 = −2^24 is the largest frame sum the kernel's exact row sum must hold."""
    rng = np.random.default_rng(2024)
    return [("speech", fx.pcm[: 16000 * 6]), ("zeros", np.zeros(2000, np.int16)),
            ("full-scale constant", np.full(3001, -32768, np.int16)), ("clipped noise", helpers.clipped_noise(rng, 8000)),
            ("small constant", np.full(2000, 3, np.int16)), ("speech", fx.pcm[16000 * 6: 16000 * 8])]


def _device_mfcc(engine, segs, opts):
    """MFCCs of a batch under ``opts``; the session engine is back at the defaults afterwards."""
    so = _offsets(segs)
    try:
        engine.configure_mfcc(**opts)
        frames = engine.num_frames_array(np.diff(so))
        out, fo = engine.mfcc(_dev(engine, np.concatenate(segs).astype(np.int16)), so)
        out = out.cpu().numpy()
    finally:
        engine.configure_mfcc()
    assert np.array_equal(np.diff(fo), frames)
    return [out[fo[u]: fo[u + 1]] for u in range(len(segs))], frames


@pytest.mark.parametrize("snip", [0, 1])
@pytest.mark.parametrize("name,opts", GRID, ids=[n for n, _ in GRID])
def test_mfcc_option_matrix(engine, fx, name, opts, snip):
    """One option set away from the default, on speech at an even and at an odd sample offset, digital silence, a
    full-scale and a small constant and clipped noise: frame counts equal the oracle's (the window and shift are computed
    in three places: the library and engine.num_frames_array in float32, the oracle) and the cepstra agree to 2e-3 (5e-3 on
    the full-scale synthetic blocks).
    One combination has a reference of its own: without DC removal a full-scale constant is the window's spectrum, whose
    side lobes lie below the float32 rounding noise of ANY 512-point FFT — the oracle itself is 7e-2 away from the float64
    restatement there (constants of 10 and more: > 3e-3; a constant of 3 sinks the side lobes under the mel floor: 2e-4).
    That block is compared with the float64 restatement, at four times the oracle's own distance from it."""
    d = dict(opts, snip_edges=snip)
    blocks = _matrix_audio(fx)
    segs = [s for _, s in blocks]
    so = _offsets(segs)
    assert (so[:-1] % 2 == 1).any() and blocks[-1][0] == "speech" and so[-2] % 2 == 1
    got, frames = _device_mfcc(engine, segs, d)
    oo = helpers.oracle_mfcc_opts(**d)
    assert np.array_equal(frames, [O.mfcc_num_frames(len(s), oo) for s in segs])
    win, shift = helpers.mfcc_window_samples(**d)
    bad = []
    for u, (kind, s) in enumerate(blocks):
        ref = O.mfcc(s.astype(np.float32), oo)
        assert got[u].shape == ref.shape and ref.shape[0] > 0, (kind, got[u].shape, ref.shape)
        bar = FULL_SCALE_BAR if kind in ("full-scale constant", "clipped noise") else SPEECH_BAR
        if kind == "full-scale constant" and not d.get("remove_dc_offset", 1):
            f64 = helpers.np_mfcc(s, **d)
            bar, ref = 4.0 * float(np.abs(ref - f64).max()), f64
        diff = float(np.abs(got[u] - ref).max())
        print(f"{name} snip_edges={snip} window {win} shift {shift}: {kind} at sample {so[u]}: {ref.shape[0]} frames, "
              f"max |device - oracle| {diff:.2e} (bar {bar:.1e})")
        if not diff < bar:
            per_frame = np.abs(got[u] - ref).max(axis=1)
            bad.append(f"{kind} at sample {so[u]}: {diff:.3e} >= {bar:.1e} ({int((per_frame >= bar).sum())} of {ref.shape[0]} frames)")
    assert not bad, f"{name} snip_edges={snip} (window {win}, shift {shift}): " + "; ".join(bad)


@pytest.mark.parametrize("snip", [0, 1])
@pytest.mark.parametrize("win", [320, 400, 448])
def test_mfcc_short_utterances_per_window_class(engine, fx, win, snip):
    """Utterances of no frame, one frame, repeated reflection (shorter than half a window) and the first lengths whose
    frame qualifies for the kernel's aligned 32·kJ-sample load, for a window that leaves whole registers, part of the last
    register and (448: the second instantiation) whole registers beyond its end.  Every length occurs at an even and at an
    odd sample offset of the batch buffer."""
    shift, span = 160, 32 * (13 if win <= 416 else 16)
    lens = [1, shift // 2 - 1, shift // 2, win - 1, win, win + 1, win + shift - 1, win + shift, span - 1, span, span + 1]
    assert sum(lens) % 2 == 1                        # the second round of the same lengths starts one sample off
    segs, at = [], 16000
    for n in lens + lens:
        segs.append(fx.pcm[at: at + n])
        at += n + 37
    so = _offsets(segs)
    assert all((so[k] + so[k + len(lens)]) % 2 == 1 for k in range(len(lens)))
    d = dict(frame_length_ms=win / 16.0, snip_edges=snip)
    got, frames = _device_mfcc(engine, segs, d)
    oo = helpers.oracle_mfcc_opts(**d)
    assert helpers.mfcc_window_samples(**d) == (win, shift)
    assert np.array_equal(frames, [O.mfcc_num_frames(len(s), oo) for s in segs])
    assert 0 in frames and 1 in frames and frames.max() >= 2
    worst = 0.0
    for u, s in enumerate(segs):
        ref = O.mfcc(s.astype(np.float32), oo)
        assert got[u].shape == ref.shape, (len(s), got[u].shape, ref.shape)
        if ref.size:
            diff = float(np.abs(got[u] - ref).max())
            worst = max(worst, diff)
            assert diff < SPEECH_BAR, (len(s), int(so[u]), diff)
    print(f"window {win} snip_edges={snip}: worst {worst:.2e} over {len(segs)} utterances, frames {frames.tolist()}")


def test_mfcc_options_through_the_kalpy_wrapper(fx):
    """kalpy_api.MfccComputer maps MFA's option names (frame_length, frame_shift, …) onto the library's."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from montreal_forced_aligner_amd import kalpy_api as KA

    pcm = fx.pcm[16000: 16000 * 4]
    try:
        got = KA.MfccComputer(frame_length=20, frame_shift=5, num_mel_bins=30, num_coefficients=12, low_frequency=0,
                              high_frequency=-200).compute_mfccs(pcm)
    finally:
        KA.get_engine().configure_mfcc()
    ref = O.mfcc(pcm.astype(np.float32), O.default_mfcc_opts(frame_length_ms=20.0, frame_shift_ms=5.0, num_mel_bins=30,
                                                             num_ceps=12, low_freq=0.0, high_freq=-200.0))
    assert got.shape == ref.shape == (600, 12)
    diff = float(np.abs(got - ref).max())
    print(f"MfccComputer(20 ms / 5 ms, 30 bins, 12 cepstra, 0 … Nyquist-200): max |device - oracle| {diff:.2e}")
    assert diff < SPEECH_BAR


REFUSED = [("33 bins", dict(num_mel_bins=33)), ("17 cepstra", dict(num_mel_bins=23, num_coefficients=17)),
           ("more cepstra than bins", dict(num_mel_bins=12, num_coefficients=13)),
           ("32 x 13 over the 384-entry DCT table", dict(num_mel_bins=32, num_coefficients=13)),
           ("low above high", dict(low_frequency=4000.0, high_frequency=3000.0)),
           ("low equal to high", dict(low_frequency=3000.0, high_frequency=3000.0)),
           ("high above Nyquist", dict(high_frequency=9000.0)),
           ("high below zero from Nyquist", dict(high_frequency=-8000.0)),
           ("256-sample window", dict(frame_length_ms=16.0)), ("513-sample window", dict(frame_length_ms=513 / 16.0)),
           ("an empty mel bin", dict(low_frequency=20.0, high_frequency=400.0, num_mel_bins=23))]


@pytest.mark.parametrize("what,opts", REFUSED, ids=[w for w, _ in REFUSED])
def test_mfcc_configure_refusals_leave_the_engine_usable(engine, fx, what, opts):
    """Every host-side check of mfa_mfcc_configure raises, and the engine goes on computing with the options it had.
    (The check on the number of filterbank pieces has no legal option set that reaches it: the triangles of at most 32 bins
    cover at most 2 × 255 FFT bins, cut into pieces of 8 that is fewer than 510 / 8 + 32 < 96 pieces.)"""
    seg = fx.pcm[16000: 16000 * 2 + 1]
    so = np.array([0, len(seg)], np.int64)
    try:
        engine.configure_mfcc(snip_edges=1)
        with pytest.raises(_lib.MfaHipError):
            engine.configure_mfcc(**opts)
        out, fo = engine.mfcc(_dev(engine, seg), so)           # still at snip_edges=1, 13 cepstra
        out = out.cpu().numpy()
    finally:
        engine.configure_mfcc()
    ref = O.mfcc(seg.astype(np.float32), O.default_mfcc_opts(snip_edges=1))
    assert out.shape == ref.shape and np.abs(out - ref).max() < SPEECH_BAR


# ---- feature kernels ---------------------------------------------------------------------------------------------------
def _feature_batch(rng, dim, n_spk=3):
    mf = [helpers.mfcc_like(rng, T, dim) for T in T_LIST]
    utt2spk = (np.arange(len(mf)) % n_spk).astype(np.int32)
    return mf, _offsets(mf), utt2spk


def _oracle_cmvn(mf, utt2spk, u):
    return O.cmvn_apply(O.cmvn_stats([mf[v] for v in range(len(mf)) if utt2spk[v] == utt2spk[u]]), mf[u])


@pytest.mark.parametrize("cmvn", [True, False], ids=["cmvn", "no_cmvn"])
@pytest.mark.parametrize("dim", [8, 12, 13, 16])
def test_delta_features_at_other_dims_and_short_utterances(engine, dim, cmvn):
    rng = np.random.default_rng(300 + dim)
    mf, fo, utt2spk = _feature_batch(rng, dim)
    d_mf = _dev(engine, np.concatenate(mf))
    if cmvn:
        feats = engine.features(d_mf, fo, utt2spk, engine.cmvn_stats(d_mf, fo, utt2spk, 3)).cpu().numpy()
    else:
        feats = engine.features(d_mf, fo).cpu().numpy()
    assert feats.shape == (fo[-1], 3 * dim)
    exact = total = 0
    worst = 0.0
    for u, x in enumerate(mf):
        ref = O.deltas(_oracle_cmvn(mf, utt2spk, u) if cmvn else x)
        got = feats[fo[u]: fo[u + 1]]
        assert got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
        exact += int((got == ref).sum()); total += ref.size
    print(f"deltas dim {dim} cmvn {cmvn}: max |device - oracle| {worst:.2e}, bit-equal {exact / total:.5f}")
    assert worst < 1e-4
    assert exact / total > 0.999


def _generic_lds_bytes(dim, ctx, rows, cols):
    """The dynamic LDS mfa_feats_batch asks for the generic kernel: the base-feature tile with its halo, the LDA matrix, room
    for an fMLLR matrix and the LDA outputs of a 64-frame tile."""
    return ((64 + 2 * ctx) * dim + rows * cols + rows * (rows + 1) + 64 * rows) * 4


@pytest.mark.parametrize("fmllr", [False, True], ids=["lda", "lda_fmllr"])
@pytest.mark.parametrize("offset", [0, 1], ids=["no_offset", "offset_column"])
@pytest.mark.parametrize("dim,ctx,rows", LDA_SHAPES)
def test_generic_splice_lda_kernel_at_other_shapes(engine, dim, ctx, rows, offset, fmllr):
    sdim = (2 * ctx + 1) * dim
    assert _generic_lds_bytes(dim, ctx, rows, sdim + offset) <= 64 << 10      # what a launch may ask for without an attribute
    rng = np.random.default_rng(1000 * dim + 100 * ctx + rows)
    mf, fo, utt2spk = _feature_batch(rng, dim)
    lda = helpers.random_affine(rng, rows, sdim + offset)
    fm = np.stack([helpers.random_affine(rng, rows, rows + 1) for _ in range(3)])
    d_mf = _dev(engine, np.concatenate(mf))
    stats = engine.cmvn_stats(d_mf, fo, utt2spk, 3)
    got_all = engine.features(d_mf, fo, utt2spk, stats, lda=_dev(engine, lda), fmllr=_dev(engine, fm) if fmllr else None,
                              splice_context=ctx).cpu().numpy()
    assert got_all.shape == (fo[-1], rows)
    exact = total = 0
    worst = 0.0
    for u in range(len(mf)):
        ref = O.affine(O.splice(_oracle_cmvn(mf, utt2spk, u), ctx, ctx), lda)
        if fmllr:
            ref = O.affine(ref, fm[utt2spk[u]])
        got = got_all[fo[u]: fo[u + 1]]
        assert got.shape == ref.shape
        worst = max(worst, float(np.abs(got - ref).max()))
        exact += int((got == ref).sum()); total += ref.size
    print(f"generic kernel ({dim}, ±{ctx}, {rows}) cols {sdim + offset} fmllr {fmllr}: max |device - oracle| {worst:.2e}, "
          f"bit-equal {exact / total:.5f}")
    assert worst < 1e-4


@pytest.mark.parametrize("offset", [0, 1], ids=["no_offset", "offset_column"])
def test_generic_kernel_refuses_a_shape_that_does_not_fit_lds(engine, offset):
    """The limits on the base dim (16) and the LDA rows (64) admit (16, ±3, 64), whose tile is 66 KB: refused on the host with
    a message, never found out by a failed launch; the engine goes on working."""
    dim, ctx, rows = 16, 3, 64
    sdim = (2 * ctx + 1) * dim
    assert _generic_lds_bytes(dim, ctx, rows, sdim + offset) > 64 << 10
    rng = np.random.default_rng(9)
    mf, fo, utt2spk = _feature_batch(rng, dim)
    d_mf = _dev(engine, np.concatenate(mf))
    with pytest.raises(_lib.MfaHipError, match="LDS"):
        engine.features(d_mf, fo, lda=_dev(engine, helpers.random_affine(rng, rows, sdim + offset)), splice_context=ctx)
    torch.cuda.synchronize()
    got = engine.features(d_mf, fo).cpu().numpy()
    assert np.abs(got[fo[-2]:] - O.deltas(mf[-1])).max() < 1e-4


@pytest.mark.parametrize("fmllr", [False, True], ids=["lda", "lda_fmllr"])
@pytest.mark.parametrize("offset", [0, 1], ids=["no_offset", "offset_column"])
def test_generic_kernel_is_bit_identical_to_register_kernel(engine, monkeypatch, offset, fmllr):
    """feats.hip: feats_lda_kernel runs "the same fmaf chains, same order, as feats_kernel and the oracle"."""
    dim, ctx, rows = 13, 3, 40
    rng = np.random.default_rng(77 + 2 * offset + fmllr)
    mf, fo, utt2spk = _feature_batch(rng, dim)
    lda = helpers.random_affine(rng, rows, 91 + offset)
    fm = np.stack([helpers.random_affine(rng, rows, rows + 1) for _ in range(3)])
    d_mf = _dev(engine, np.concatenate(mf))
    stats = engine.cmvn_stats(d_mf, fo, utt2spk, 3)
    args = dict(lda=_dev(engine, lda), fmllr=_dev(engine, fm) if fmllr else None)
    monkeypatch.delenv("MFA_FEATS_GENERIC", raising=False)
    fast = engine.features(d_mf, fo, utt2spk, stats, **args).cpu().numpy()
    monkeypatch.setenv("MFA_FEATS_GENERIC", "1")
    generic = engine.features(d_mf, fo, utt2spk, stats, **args).cpu().numpy()
    monkeypatch.delenv("MFA_FEATS_GENERIC")
    assert np.array_equal(fast, generic)
    for u in range(len(mf)):
        ref = O.affine(O.splice(_oracle_cmvn(mf, utt2spk, u)), lda)
        if fmllr:
            ref = O.affine(ref, fm[utt2spk[u]])
        assert np.abs(generic[fo[u]: fo[u + 1]] - ref).max() < 1e-4


@pytest.mark.parametrize("dim", [8, 16])
def test_cmvn_stats_empty_speakers_and_scrambled_order(engine, dim):
    """Speaker 0: 300 utterances scattered through the batch; 1: a few; 2: none at all; 3: only utterances of zero frames;
    4: both kinds.  Rows of speakers without a frame are all zero and nobody else's sums move."""
    rng = np.random.default_rng(500 + dim)
    spk = np.array([0] * 300 + [1] * 7 + [3] * 5 + [4] * 6, np.int32)
    lens = np.concatenate([rng.integers(1, 40, 300), rng.integers(1, 200, 7), np.zeros(5, np.int64), [0, 17, 0, 1, 64, 0]])
    order = rng.permutation(len(spk))
    spk, lens = spk[order], lens[order]
    mf = [helpers.mfcc_like(rng, int(T), dim) for T in lens]
    fo = _offsets(mf)
    stats = engine.cmvn_stats(_dev(engine, np.concatenate(mf)), fo, spk, 5).cpu().numpy()
    assert stats.shape == (5, 2, dim + 1)
    assert not stats[2].any() and not stats[3].any()
    for s in (0, 1, 4):
        ref = O.cmvn_stats([mf[u] for u in range(len(mf)) if spk[u] == s and mf[u].shape[0] > 0])
        assert np.allclose(stats[s], ref, rtol=1e-13, atol=1e-9), s
        assert stats[s, 0, dim] == lens[spk == s].sum()


# ---- the front-end fuzzer's batches at fixed seeds -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("win,shift", [(400, 160), (320, 80)], ids=["default", "20ms_5ms"])
def test_frontend_fuzz_seeds(engine, win, shift, seed):
    """tools/frontend_fuzz.py's batches (helpers.frontend_fuzz_case) with the lengths laid around the framing boundaries of
    the window in use.  A tone over a weak noise floor leaves most mel bins at the rounding noise of any float32 512-point
    FFT (two implementations differ by up to 7e-3 there; see the generator): 1e-2 for that signal kind, 2e-3 for every
    other one.  No utterance is skipped: one with no frame is an empty array on both sides."""
    import synth_workload as synth

    case = helpers.frontend_fuzz_case(seed, win, shift)
    segs, kinds, rows, n_spk = case["segs"], case["kinds"], case["rows"], case["n_spk"]
    d = dict(frame_length_ms=win / 16.0, frame_shift_ms=shift / 16.0, snip_edges=int(case["snip_edges"]))
    got, frames = _device_mfcc(engine, segs, d)
    oo = helpers.oracle_mfcc_opts(**d)
    worst = {}
    for u, s in enumerate(segs):
        ref = O.mfcc(s.astype(np.float32), oo)
        assert got[u].shape == ref.shape, (u, kinds[u], len(s), got[u].shape, ref.shape)
        diff = float(np.abs(got[u] - ref).max()) if ref.size else 0.0
        worst[kinds[u]] = max(worst.get(kinds[u], 0.0), diff)
        assert diff < (1e-2 if kinds[u] == helpers.FUZZ_TONE else SPEECH_BAR), (u, kinds[u], len(s), diff)
    # CMVN over the speaker groups and both feature kernels, from the DEVICE's MFCCs on both sides
    fo = _offsets(got)
    d_mfcc = _dev(engine, np.concatenate(got))
    stats = engine.cmvn_stats(d_mfcc, fo, rows, n_spk)
    st = stats.cpu().numpy()
    for s_ in range(n_spk):
        mine = [got[u] for u in range(len(segs)) if rows[u] == s_ and got[u].shape[0] > 0]
        if mine:
            assert np.allclose(st[s_], O.cmvn_stats(mine), rtol=1e-12, atol=1e-9), ("cmvn", s_)
        else:
            assert not st[s_].any()
    lda, fm = synth.seeded_lda(), synth.seeded_fmllr(16)
    f_delta = engine.features(d_mfcc, fo, rows, stats).cpu().numpy()
    f_lda = engine.features(d_mfcc, fo, rows, stats, lda=_dev(engine, lda), fmllr=_dev(engine, fm[:n_spk])).cpu().numpy()
    wd = wl = 0.0
    for u in range(len(segs)):
        if got[u].shape[0] == 0:
            continue                                   # (its rows of st may be all zero: nothing to normalise, nothing written)
        base = O.cmvn_apply(st[rows[u]], got[u])
        wd = max(wd, float(np.abs(f_delta[fo[u]: fo[u + 1]] - O.deltas(base)).max()))
        wl = max(wl, float(np.abs(f_lda[fo[u]: fo[u + 1]] - O.affine(O.affine(O.splice(base), lda), fm[rows[u]])).max()))
    print(f"seed {seed} window {win} shift {shift} snip_edges {d['snip_edges']}: {len(segs)} utterances, mfcc worst {worst}, "
          f"deltas {wd:.1e}, lda+fmllr {wl:.1e}")
    assert wd < 1e-3 and wl < 1e-3


def test_delta_scales_reach_every_device(fx):
    """The delta scales are __constant__ data, one copy per device: an engine on a second device of the same process must
    upload its own (a flag per process left them zero there)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from montreal_forced_aligner_amd.engine import AlignmentEngine

    rng = np.random.default_rng(5)
    x = helpers.mfcc_like(rng, 50, 13)
    fo = np.array([0, 50], np.int64)
    for dev in (0, 1):
        with torch.cuda.device(dev):
            e = AlignmentEngine(dev)
            try:
                got = e.features(_dev(e, x), fo).cpu().numpy()
            finally:
                e.close()
        assert np.abs(got - O.deltas(x)).max() < 1e-4, dev
