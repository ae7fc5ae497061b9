"""The speech-activity kernels (csrc/vad.hip) against their host twins (csrc/vad_host.cpp), bit for bit: energy VAD, the
per-utterance integer scan, sliding-window CMVN, voiced-frame selection with subsampling, and voiced runs — over the
smallest shapes that can break them (empty / one-frame utterances, wavefront and workgroup edges, both sides of the scan's
block span, a batch whose block sums need more than one pass of the scanning workgroup, windows below / at / above the
utterance length, tile edges), batch invariance, the capacity redo of the runs, and the refusals.  tests/test_vad_cpu.py
holds the twins to the plain restatement of tests/vad_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import vad_ref as R

pytestmark = pytest.mark.gpu

SMALL = (0, 1, 2, 40, 41, 81, 63, 64, 65, 255, 256, 257)


def offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def energies(rng, T, stride):
    """float32 [T, stride]: column 0 like a log energy with loud and quiet stretches."""
    x = rng.standard_normal((T, stride)).astype(np.float32) * 3.0
    x[:, 0] += 8.0 + 6.0 * np.sign(np.sin(np.arange(T) / 37.0)).astype(np.float32)
    return x


def dev(engine, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_vad(engine, x, fo, **opts):
    from montreal_forced_aligner_amd import frontend as F

    got = [t.cpu().numpy() for t in engine.vad(dev(engine, x), fo, **opts)]
    want = F.vad_host(x, fo, **opts)
    for g, w, name in zip(got, want, ("vad", "threshold", "voiced")):
        assert same_bits(g, w), (name, opts)
    return got


@pytest.fixture(scope="module")
def small_batch(engine):
    rng = np.random.default_rng(11)
    B = engine.vad_scan_block_frames()
    lens = list(SMALL) + [B - 1, B, B + 1]
    fo = offs(lens)
    return energies(rng, int(fo[-1]), 13), fo


@pytest.mark.parametrize("ctx", [0, 1, 2, 40, 100000])
def test_vad_equals_twin_over_lengths_and_contexts(engine, small_batch, ctx):
    x, fo = small_batch
    vad, thr, voiced = check_vad(engine, x, fo, frames_context=ctx, energy_threshold=5.5)
    assert set(np.unique(vad)) <= {0.0, 1.0}
    assert np.array_equal(voiced, [int(vad[a:b].sum()) for a, b in zip(fo[:-1], fo[1:])])
    # a short utterance against the frame-by-frame restatement too (decisions: the thresholds may differ in the last bit)
    k = SMALL.index(81)
    ref, ref_thr = R.vad(x[fo[k]: fo[k + 1], 0], 5.5, 0.5, ctx, 0.6)
    assert abs(ref_thr - thr[k]) <= 2e-6 * abs(ref_thr) and np.array_equal(ref, vad[fo[k]: fo[k + 1]])


def test_vad_adaptive_and_tie_options(engine, small_batch):
    x, fo = small_batch
    check_vad(engine, x, fo, energy_threshold=0.0, energy_mean_scale=1.0)             # the reference's adaptive mode
    check_vad(engine, x, fo, frames_context=2, proportion_threshold=0.6)             # 3 of 5 is an exact tie: 3 >= 5 · 0.6f
    check_vad(engine, x, fo, frames_context=1, proportion_threshold=1.0, energy_mean_scale=0.0)


@pytest.fixture(scope="module")
def long_batch(engine):
    """Empty and one-frame utterances around one whose scan needs more block sums than the scanning workgroup has threads."""
    rng = np.random.default_rng(12)
    B, P = engine.vad_scan_block_frames(), engine.vad_scan_totals_threads()
    lens = [0, 1, B * P + B + 3, 0, 5, 1]
    fo = offs(lens)
    return energies(rng, int(fo[-1]), 1), fo


def test_scan_equals_twin_beyond_one_pass_of_block_sums(engine, long_batch):
    from montreal_forced_aligner_amd import frontend as F

    x, fo = long_batch
    assert (fo[-1] + engine.vad_scan_block_frames() - 1) // engine.vad_scan_block_frames() > engine.vad_scan_totals_threads()
    v = ((x[:, 0] > 8.0) * (1 + (np.arange(x.shape[0]) % 3 == 0))).astype(np.int32)   # values 0, 1, 2
    scan, totals = (t.cpu().numpy() for t in engine.segment_scan(dev(engine, v), fo))
    w_scan, w_totals = F.vad_scan_host(v, fo)
    assert same_bits(scan, w_scan) and same_bits(totals, w_totals)
    assert int(totals[2]) == int(v[fo[2]: fo[3]].sum())
    # lengths on both sides of the block span, one call each
    B = engine.vad_scan_block_frames()
    for T in (B - 1, B, B + 1):
        s, t = (a.cpu().numpy() for a in engine.segment_scan(dev(engine, v[:T]), offs([T])))
        ws, wt = F.vad_scan_host(v[:T], offs([T]))
        assert same_bits(s, ws) and same_bits(t, wt)
        rs, rt = R.scan(v[:T], offs([T]))
        assert np.array_equal(s, rs) and np.array_equal(t, rt)


def test_long_batch_vad_runs_and_selection(engine, long_batch):
    from montreal_forced_aligner_amd import frontend as F

    x, fo = long_batch
    vad, _thr, _cnt = check_vad(engine, x, fo, frames_context=2)
    got = engine.vad_runs(dev(engine, vad), fo)
    want = F.vad_runs_host(vad, fo)
    for g, w in zip(got, want):
        assert same_bits(g, w)
    out, oo = engine.select_frames(dev(engine, x), fo, dev(engine, vad), 3)
    w_out, w_oo = F.select_frames_host(x, fo, vad, 3)
    assert same_bits(out.cpu().numpy(), w_out) and same_bits(oo, w_oo)


def test_runs_of_silent_voiced_and_alternating_utterances(engine):
    from montreal_forced_aligner_amd import frontend as F

    lens = [300, 0, 257, 1, 1, 64, 129]
    fo = offs(lens)
    vad = np.zeros(int(fo[-1]), dtype=np.float32)
    vad[fo[2]: fo[3]] = 1.0                  # all voiced: one run over the whole utterance
    vad[fo[3]: fo[4]] = 1.0                  # one voiced frame
    vad[fo[5]: fo[6]] = 1.0                  # ends where the next utterance, which starts voiced, begins
    vad[fo[6]: fo[7]: 2] = 1.0               # alternating
    b, e, ro = engine.vad_runs(dev(engine, vad), fo)
    wb, we, wro = F.vad_runs_host(vad, fo)
    assert same_bits(b, wb) and same_bits(e, we) and same_bits(ro, wro)
    assert np.diff(ro).tolist() == [0, 0, 1, 1, 0, 1, 65]
    assert (b[0], e[0]) == (0, 257) and (b[1], e[1]) == (0, 1) and (b[2], e[2]) == (0, 64)
    for k in range(len(lens)):
        assert list(zip(b[ro[k]: ro[k + 1]].tolist(), e[ro[k]: ro[k + 1]].tolist())) == R.runs(vad[fo[k]: fo[k + 1]])
    # too little room at first: the call is made again with room for all, and gives the same
    b2, e2, ro2 = engine.vad_runs(dev(engine, vad), fo, capacity=1)
    assert same_bits(b2, wb) and same_bits(e2, we) and same_bits(ro2, wro)


@pytest.mark.parametrize("dim", [1, 13, 40, 45])
def test_sliding_cmvn_equals_twin(engine, dim):
    from montreal_forced_aligner_amd import frontend as F

    rng = np.random.default_rng(13 + dim)
    tile = engine.sliding_cmvn_tile_frames()
    lens = [0, 1, 2, tile - 1, tile, tile + 1, 299, 300, 301, 599, 600, 601, 700]
    fo = offs(lens)
    x = energies(rng, int(fo[-1]), dim + 3)
    d = dev(engine, x)
    for window in (1, 2, 300, 600):
        for center in (0, 1):
            for norm_vars in (0, 1):
                o = dict(cmn_window=window, center=center, norm_vars=norm_vars)
                got = engine.sliding_cmvn(d, fo, dim=dim, **o).cpu().numpy()
                assert same_bits(got, F.sliding_cmvn_host(x, fo, dim=dim, **o)), o
                assert same_bits(got[:, dim:], x[:, dim:])           # pad columns pass through
    # the restatement on a short utterance: window 300 over 301 frames, centred, variance normalised
    k = lens.index(301)
    got = engine.sliding_cmvn(d, fo, dim=dim, cmn_window=300, center=1, norm_vars=1).cpu().numpy()[fo[k]: fo[k + 1], :dim]
    ref = R.sliding_cmvn(x[fo[k]: fo[k + 1], :dim], 300, 100, True, True)
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_selection_equals_twin_and_restatement(engine, n):
    from montreal_forced_aligner_amd import frontend as F

    rng = np.random.default_rng(17)
    lens = [0, 1, 5, 64, 65, 257, 300, 6, 2049]
    fo = offs(lens)
    x = energies(rng, int(fo[-1]), 5)
    vad = (rng.random(int(fo[-1])) < 0.6).astype(np.float32)
    vad[fo[3]: fo[4]: 2] = 1.0; vad[fo[3] + 1: fo[4]: 2] = 0.0      # alternating bits
    vad[fo[4]: fo[5]] = 0.0                                          # nothing voiced
    vad[fo[7]: fo[8]] = [1, 0, 0, 1, 0, 1]                           # three rows kept: fewer than n for n = 7
    for v in (vad, None):
        out, oo = engine.select_frames(dev(engine, x), fo, None if v is None else dev(engine, v), n)
        w_out, w_oo = F.select_frames_host(x, fo, v, n)
        assert same_bits(out.cpu().numpy(), w_out) and same_bits(oo, w_oo)
        r_out, r_oo = R.select_batch(x, fo, v, n)
        assert np.array_equal(out.cpu().numpy(), r_out) and np.array_equal(oo, r_oo)


def test_results_do_not_depend_on_the_batch(engine, small_batch):
    x, fo = small_batch
    rng = np.random.default_rng(19)
    order = rng.permutation(len(fo) - 1)
    xs = np.concatenate([x[fo[k]: fo[k + 1]] for k in order])
    fos = offs([fo[k + 1] - fo[k] for k in order])
    vad, thr, cnt = (t.cpu().numpy() for t in engine.vad(dev(engine, x), fo, frames_context=2))
    vad_s, thr_s, cnt_s = (t.cpu().numpy() for t in engine.vad(dev(engine, xs), fos, frames_context=2))
    cm = engine.sliding_cmvn(dev(engine, x), fo, cmn_window=300, center=1, norm_vars=1).cpu().numpy()
    cm_s = engine.sliding_cmvn(dev(engine, xs), fos, cmn_window=300, center=1, norm_vars=1).cpu().numpy()
    for j, k in enumerate(order):
        a, b, a2, b2 = fo[k], fo[k + 1], fos[j], fos[j + 1]
        assert same_bits(vad[a:b], vad_s[a2:b2]) and same_bits(thr[k], thr_s[j]) and cnt[k] == cnt_s[j]
        assert same_bits(cm[a:b], cm_s[a2:b2])
    k = len(SMALL) + 1                                                # the utterance of one scan block, alone
    one = x[fo[k]: fo[k + 1]]
    v1, t1, c1 = (t.cpu().numpy() for t in engine.vad(dev(engine, one), offs([len(one)]), frames_context=2))
    assert same_bits(v1, vad[fo[k]: fo[k + 1]]) and same_bits(t1[0], thr[k]) and c1[0] == cnt[k]
    assert same_bits(engine.sliding_cmvn(dev(engine, one), offs([len(one)]), cmn_window=300, center=1, norm_vars=1).cpu().numpy(),
                     cm[fo[k]: fo[k + 1]])


def test_refusals_return_the_librarys_error(engine):
    from montreal_forced_aligner_amd import _lib

    lib, ctx = engine.lib, engine.ctx
    x = dev(engine, np.zeros((8, 4), dtype=np.float32))
    out = dev(engine, np.zeros((8, 4), dtype=np.float32))
    vad = dev(engine, np.ones(8, dtype=np.float32))
    src = dev(engine, np.zeros(8, dtype=np.int32))
    fo = dev(engine, offs([8]))
    oo = dev(engine, np.zeros(2, dtype=np.int64))
    p = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    vo = _lib.VadOpts(5.0, 0.5, 0.6, 0)
    co = _lib.SlidingCmvnOpts(300, 100, 1, 0)

    def refused(rc, word):
        assert rc != 0 and word in lib.mfa_last_error(ctx).decode()

    for n in (0, -1):
        refused(lib.mfa_select_frames_count(ctx, p(vad), p(fo), 1, 8, n, p(src), p(oo)), "subsample factor")
    refused(lib.mfa_sliding_cmvn_batch(ctx, p(x), p(fo), 1, 8, 4, 4, C.byref(_lib.SlidingCmvnOpts(0, 100, 1, 0)), p(out)), "cmn_window")
    refused(lib.mfa_sliding_cmvn_batch(ctx, p(x), p(fo), 1, 8, 5, 4, C.byref(co), p(out)), "columns")
    refused(lib.mfa_sliding_cmvn_batch(ctx, None, p(fo), 1, 8, 4, 4, C.byref(co), p(out)), "no input")
    refused(lib.mfa_sliding_cmvn_batch(ctx, p(x), p(fo), 1, 8, 4, 4, C.byref(co), p(x)), "may not be the input")
    refused(lib.mfa_vad_batch(ctx, None, 4, p(fo), 1, 8, 8, C.byref(vo), p(vad), p(vad), None), "no input")
    refused(lib.mfa_vad_batch(ctx, p(x), 4, None, 1, 8, 8, C.byref(vo), p(vad), p(vad), None), "frame offsets")
    refused(lib.mfa_vad_batch(ctx, p(x), 4, p(fo), 1, 8, 8, C.byref(_lib.VadOpts(5.0, 0.5, 0.6, -1)), p(vad), p(vad), None), "frames_context")
    refused(lib.mfa_select_frames_batch(ctx, p(x), 3, 4, p(src), 8, p(out), 4), "columns")
    refused(lib.mfa_select_frames_batch(ctx, p(x), 4, 4, None, 8, p(out), 4), "no row map")
    refused(lib.mfa_vad_runs_batch(ctx, None, p(fo), 1, 8, 4, p(src), p(src), p(oo)), "no input")
    with pytest.raises(_lib.MfaHipError):
        engine.select_frames(x, offs([8]), vad, 0)
    with pytest.raises(KeyError):
        engine.vad(x, offs([8]), no_such_option=1)
    # and the engine is still good for the next call
    assert engine.vad(x, offs([8]))[0].shape == (8,)
