"""The pitch kernels (pitch.hip) against tests/pitch_ref.py, stage by stage, then the layers above them.

Stages 1 and 2 are exact contracts: the resampled signal, both up-sampled NCCF matrices, the state path and the raw output
must equal the restatement's float32 chain bit for bit.  The processed columns (ProcessPitch) use the device's logf / expf /
powf and carry a tolerance:

    the largest absolute difference between a float32 numpy evaluation of ProcessPitch and the float64 restatement on these
    inputs — a quantity that does not involve the kernel — is 1.25e-5 (POV feature 1.25e-5: the 0.15th power of 1.0001 - n
    where n is within 1e-4 of 1; normalised log-pitch 1.14e-5; raw log-pitch 2.6e-7); the device is allowed 4 x the figure
    the test measures at run time, 5.0e-5.  The device measured 1.24e-5, 1.1e-6 and 4.9e-7.

The float64 check of the state path runs on inputs chosen for it (tests/test_pitch_cpu.py: margin_inputs, and the reason):
with nccf_ballast 7000 the pitch NCCF of a steady signal is the plain NCCF / 84, so a tone or chirp of a few partials has
margins of 1e-5 between neighbouring predecessors (1 % of the frames above 1e-4); a low-pitched buzz whose harmonics reach
the resampled signal's band edge has a peak a few states wide and margins of 3e-4 - 1e-3: 100 % of the tone's frames and
96.5 % of the chirp's exceed 1e-4 — on the restatement alone (test_pitch_cpu) and, the NCCF being bit-identical, here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import pitch_ref as R
from tests.test_pitch_cpu import FS, MFA, harmonic, margin_inputs

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def pe():
    """An engine of this module's own: the tests below change its pitch options."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from montreal_forced_aligner_amd.engine import AlignmentEngine

    e = AlignmentEngine(0)
    yield e
    e.close()


def configure(e, o: R.Opts, **kw):
    e.configure_pitch(sample_frequency=o.sample_frequency, frame_length=o.frame_length, frame_shift=o.frame_shift, min_f0=o.min_f0,
                      max_f0=o.max_f0, soft_min_f0=o.soft_min_f0, penalty_factor=o.penalty_factor, lowpass_cutoff=o.lowpass_cutoff,
                      resample_frequency=o.resample_frequency, delta_pitch=o.delta_pitch, nccf_ballast=o.nccf_ballast,
                      lowpass_filter_width=o.lowpass_filter_width, upsample_filter_width=o.upsample_filter_width,
                      snip_edges=o.snip_edges, pov_scale=o.pov_scale, pov_offset=o.pov_offset, pitch_scale=o.pitch_scale,
                      normalization_context=o.normalization_context, add_pov_feature=o.add_pov_feature,
                      add_normalized_log_pitch=o.add_normalized_log_pitch, add_raw_log_pitch=o.add_raw_log_pitch, **kw)


def stages(e, utts, o: R.Opts):
    """mfa_debug_pitch_stages on a batch: per utterance dicts like pitch_ref.compute's (device results)."""
    configure(e, o)
    tb = R.tables(o)
    so = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    fo = e.pitch_frame_offsets(so)
    ro = np.concatenate([[0], np.cumsum([tb.rs.num_out(len(u)) for u in utts])]).astype(np.int64)
    assert np.diff(fo).tolist() == [R.num_frames(len(u), o) for u in utts]
    dev, F, S = e.device, int(fo[-1]), tb.S
    pcm = torch.from_numpy(np.concatenate(utts).astype(np.int16)).to(dev)
    d_so, d_fo, d_ro = (torch.from_numpy(a).to(dev) for a in (so, fo, ro))
    rs = torch.full((int(ro[-1]) + 64,), np.nan, dtype=torch.float32, device=dev)
    npi = torch.full((F * S + 64,), np.nan, dtype=torch.float32, device=dev)
    nv = torch.full((F * S + 64,), np.nan, dtype=torch.float32, device=dev)
    path = torch.full((F + 64,), -7, dtype=torch.int32, device=dev)
    raw = torch.full((F * 2 + 64,), np.nan, dtype=torch.float32, device=dev)
    rc = e.lib.mfa_debug_pitch_stages(e.ctx, None, None, None, None, None, None, None, None, _p(pcm), _p(d_so), _p(d_fo),
                                      so.ctypes.data, fo.ctypes.data, len(utts), int(np.diff(fo).max()), _p(rs), _p(d_ro), _p(npi),
                                      _p(nv), _p(path), _p(raw))
    assert rc == 0, e.lib.mfa_last_error(e.ctx)
    torch.cuda.synchronize()
    rs, npi, nv, path, raw = (t.cpu().numpy() for t in (rs, npi, nv, path, raw))
    # nothing written past the batch's end
    assert np.all(np.isnan(rs[ro[-1]:])) and np.all(np.isnan(npi[F * S:])) and np.all(np.isnan(nv[F * S:]))
    assert np.all(path[F:] == -7) and np.all(np.isnan(raw[2 * F:]))
    out = []
    for u in range(len(utts)):
        a, b = int(fo[u]), int(fo[u + 1])
        out.append(dict(resampled=rs[ro[u]: ro[u + 1]], nccf_pitch=npi[a * S: b * S].reshape(-1, S), nccf_pov=nv[a * S: b * S].reshape(-1, S),
                        path=path[a:b].astype(np.int64), raw=raw[2 * a: 2 * b].reshape(-1, 2)))
    return out, dict(pcm=pcm, so=so, fo=fo)


def _signals():
    rng = np.random.default_rng(11)
    block = 1024                                     # mfa_resample_block_outputs: resampled samples per workgroup (checked below)
    lens = [int(0.03 * FS), int(0.26 * FS), FS]
    utts, kinds = [], []
    for n in lens + [4 * block - 4, 4 * block, 4 * block + 1]:          # resampled lengths block - 1, block, block + 1
        utts.append(harmonic(140.0, n / FS)[:n]); kinds.append("tone")
        utts.append(np.round(rng.standard_normal(n) * 3000.0).astype(np.int16)); kinds.append("noise")
    for n in lens:
        utts.append(np.zeros(n, dtype=np.int16)); kinds.append("silence")
        utts.append(np.where((np.arange(n) // 53) % 2 == 0, 32767, -32768).astype(np.int16)); kinds.append("square")
    return utts, kinds


_CASE = {}


def _case(pe):
    """The stage-1 batch on the device and through the float32 chain, computed once."""
    if not _CASE:
        utts, kinds = _signals()
        dev, info = stages(pe, utts, MFA)
        _CASE.update(utts=utts, kinds=kinds, dev=dev, info=info, ref=[R.compute(u, MFA, chain=True) for u in utts])
    return _CASE


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_stage1_resample_nccf_upsampling_bit_identical(pe):
    c = _case(pe)
    assert pe.resample_block_outputs() == 1024
    assert {R.tables(MFA).rs.num_out(len(u)) for u in c["utts"]} >= {1023, 1024, 1025}
    for u, kind, d, r in zip(c["utts"], c["kinds"], c["dev"], c["ref"]):
        what = (kind, len(u))
        assert _same_bits(d["resampled"], r["resampled"]), what
        assert d["nccf_pitch"].shape[0] == R.num_frames(len(u), MFA) > 0
        assert _same_bits(d["nccf_pitch"], r["nccf_pitch"]), what
        assert _same_bits(d["nccf_pov"], r["nccf_pov"]), what
        if kind == "silence":
            assert not d["nccf_pitch"].any() and not d["nccf_pov"].any()
    # the inputs exercise what they are there for
    tone = c["dev"][c["kinds"].index("tone") + 4]["nccf_pov"]          # the 1 s tone
    assert tone.max() > 0.95
    sq = [d for d, k in zip(c["dev"], c["kinds"]) if k == "square"][-1]
    assert np.abs(sq["resampled"]).max() > 20000.0 and np.isfinite(sq["nccf_pitch"]).all()


def test_stage2_state_path_bit_identical(pe):
    """Given the device's own NCCF, the path and the raw output are the chain's."""
    c = _case(pe)
    for u, kind, d in zip(c["utts"], c["kinds"], c["dev"]):
        path = R.viterbi(d["nccf_pitch"], MFA, chain=True)
        assert np.array_equal(d["path"], path), (kind, len(u))
        assert _same_bits(d["raw"], R.raw_output(d["nccf_pov"], path, MFA, chain=True)), (kind, len(u))
    tone = c["dev"][c["kinds"].index("tone") + 4]["raw"][5:-5]
    assert np.abs(tone[:, 1] / 140.0 - 1.0).max() < 0.01 and tone[:, 0].min() > 0.9


_MARGIN = {}


def _margin_case(pe):
    if not _MARGIN:
        dev, _ = stages(pe, margin_inputs(), MFA)
        res = []
        for d in dev:
            path64, margin = R.viterbi(d["nccf_pitch"], MFA, chain=False, want_margin=True)
            res.append((d["path"], path64, margin))
        _MARGIN["res"] = res
    return _MARGIN["res"]


def test_state_path_equals_float64_argmin_where_the_margin_is_clear(pe):
    """O(S^2) float64 recursion on the device's NCCF: wherever both paths stand on the same state at frame t and the float64
    margin between its best and second-best predecessor exceeds 1e-4, they came from the same state."""
    for path, path64, margin in _margin_case(pe):
        assert np.array_equal(path, path64)                   # on these inputs the float32 path IS the float64 one
        t = np.flatnonzero(margin[1:] > 1e-4) + 1
        assert np.array_equal(path[t - 1], path64[t - 1])
        # and the two paths as wholes never part by more than a state: the float32 roundings are 1e-7, the margins 1e-4
        assert np.abs(path - path64).max() <= 1


def test_state_path_float64_margin_share(pe):
    """The share of frames whose margin exceeds 1e-4 must be >= 90 % on the tone and on the chirp."""
    tracked = []
    for path, path64, margin in _margin_case(pe):
        share = float((margin > 1e-4).mean())
        print(f"frames with a float64 margin above 1e-4: {100 * share:.1f} % (median margin {np.median(margin):.2e})")
        assert share >= 0.9
        tracked.append(1.0 / R.tables(MFA).lags[path[5:-5]])
    # they are what they are called: the tone stays at 70 Hz, the chirp glides from 55 to 65 Hz
    assert np.abs(tracked[0] / 70.0 - 1.0).max() < 0.01
    assert abs(tracked[1][0] / 55.0 - 1.0) < 0.03 and abs(tracked[1][-1] / 65.0 - 1.0) < 0.03 and np.all(np.diff(tracked[1]) >= 0.0)


def _ragged():
    rng = np.random.default_rng(5)
    frames = [1, 2, 300, 299, 1] + rng.integers(1, 301, 28).tolist()
    utts = []
    for k, t in enumerate(frames):
        n = 4 * (100 + 40 * (t - 1)) + int(rng.integers(0, 160))
        x = harmonic(90.0 + 7.0 * k, n / FS)[:n].astype(np.float64) + rng.standard_normal(n) * (200.0 + 100.0 * (k % 5))
        utts.append(np.round(x).astype(np.int16))
    return frames, utts


def test_ragged_batch_equals_each_alone_under_any_budget(pe):
    frames, utts = _ragged()
    assert len(utts) == 33 and min(frames) == 1 and max(frames) == 300
    configure(pe, MFA)
    so = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate(utts)).to(pe.device)
    raw, fo = pe.pitch_raw(pcm, so)
    assert np.diff(fo).tolist() == frames
    torch.cuda.synchronize()
    whole = raw.cpu().numpy()
    assert np.isfinite(whole).all()
    for u in range(len(utts)):                                    # alone (each its own call)
        alone, _ = pe.pitch_raw(pcm[int(so[u]): int(so[u + 1])], np.array([0, len(utts[u])], dtype=np.int64))
        assert np.array_equal(alone.cpu().numpy().view(np.uint32), whole[fo[u]: fo[u + 1]].view(np.uint32)), u
    full = pe.pitch_workspace_bytes(so, fo)
    old = os.environ.get("MFA_PITCH_WORKSPACE_MB")
    try:
        for mb in ("0.95", "0.001"):          # two 300-frame utterances (469 KB each) per sub-launch; every utterance alone
            os.environ["MFA_PITCH_WORKSPACE_MB"] = mb
            assert pe.pitch_workspace_bytes(so, fo) < full
            again, _ = pe.pitch_raw(pcm, so)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), whole.view(np.uint32)), mb
    finally:
        if old is None:
            os.environ.pop("MFA_PITCH_WORKSPACE_MB", None)
        else:
            os.environ["MFA_PITCH_WORKSPACE_MB"] = old
    # the stage check on three of them: ragged offsets, odd sample offsets
    dev, _ = stages(pe, utts[:3], MFA)
    for u in range(3):
        assert _same_bits(dev[u]["raw"], whole[fo[u]: fo[u + 1]])
        assert _same_bits(dev[u]["raw"], R.compute(utts[u], MFA, chain=True)["raw"])


@pytest.mark.parametrize("o", [R.replace(MFA, max_f0=400.0), R.replace(MFA, snip_edges=False),
                               R.replace(MFA, snip_edges=False, max_f0=400.0, sample_frequency=8000.0)], ids=["max400", "nosnip", "8k"])
def test_option_sets(pe, o):
    rng = np.random.default_rng(2)
    fs = int(o.sample_frequency)
    n = int(0.31 * fs) + 3
    t = np.arange(n) / fs
    x = np.round(6000.0 * np.sin(2 * np.pi * 180.0 * t) + 2500.0 * np.sin(2 * np.pi * 360.0 * t + 1.0) + 300.0 * rng.standard_normal(n))
    utts = [x.astype(np.int16), x[: n // 3].astype(np.int16)]
    dev, _ = stages(pe, utts, o)
    assert pe.lib.mfa_pitch_num_states(pe.ctx) == R.tables(o).S
    for u, d in zip(utts, dev):
        r = R.compute(u, o, chain=True)
        assert _same_bits(d["resampled"], r["resampled"]) and _same_bits(d["nccf_pitch"], r["nccf_pitch"])
        assert _same_bits(d["nccf_pov"], r["nccf_pov"]) and np.array_equal(d["path"], r["path"]) and _same_bits(d["raw"], r["raw"])
    assert np.abs(dev[0]["raw"][5:-5, 1] / 180.0 - 1.0).max() < 0.01


def test_refusals_leave_the_previous_options_in_force(pe):
    from montreal_forced_aligner_amd._lib import MfaHipError

    o = R.replace(MFA, max_f0=400.0)
    x = harmonic(150.0, 0.2)
    so = np.array([0, len(x)], dtype=np.int64)
    configure(pe, o)
    pcm = torch.from_numpy(x).to(pe.device)
    before = pe.pitch_raw(pcm, so)[0].cpu().numpy()
    for kw in (dict(add_delta_pitch=True), dict(max_f0=1950.0), dict(min_f0=800.0), dict(min_f0=900.0), dict(preemphasis=0.97)):
        with pytest.raises(MfaHipError):
            configure(pe, R.replace(MFA, **{k: v for k, v in kw.items() if k in ("max_f0", "min_f0")}),
                      **{k: v for k, v in kw.items() if k not in ("max_f0", "min_f0")})
        assert pe.lib.mfa_pitch_num_states(pe.ctx) == 417 and pe.num_pitch_cols == 2
    after = pe.pitch_raw(pcm, so)[0].cpu().numpy()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert _same_bits(after, R.compute(x, o, chain=True)["raw"])


# the add_* combinations MFA's pitch_options can produce (use_pitch x normalize_pitch x use_voicing, at least one column)
_COLUMNS = [(False, True, False), (False, False, True), (True, True, False), (True, False, True), (True, False, False)]


def test_processed_columns(pe):
    """ProcessPitch on the device's raw output against the float64 restatement, every column set; the tolerance is 4 x the
    float32-numpy-against-float64 difference on the same inputs (module docstring)."""
    c = _case(pe)
    pick = [k for k, (kind, u) in enumerate(zip(c["kinds"], c["utts"])) if len(u) >= int(0.26 * FS)]
    fo, so = c["info"]["fo"], c["info"]["so"]
    all_cols = R.replace(MFA, add_pov_feature=True, add_normalized_log_pitch=True, add_raw_log_pitch=True)
    # the long chirp exercises a clipped window on both sides and a full one in the middle
    chirp = harmonic(np.linspace(100.0, 200.0, 2 * FS), 2.0)
    cd, cinfo = stages(pe, [chirp], MFA)
    raws = [c["dev"][k]["raw"] for k in pick] + [cd[0]["raw"]]
    ref64 = [R.process(r, all_cols) for r in raws]
    ref32 = [R.process(r, all_cols, dt=np.float32) for r in raws]
    yard = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(ref32, ref64))
    per_col = [max(float(np.abs(a.astype(np.float64) - b)[:, j].max()) for a, b in zip(ref32, ref64)) for j in range(3)]
    print(f"float32 numpy against float64, largest absolute difference per column (POV, normalised, raw): {per_col}; bound {4 * yard:.3e}")
    assert 0.0 < yard < 1e-4
    for pov, norm, rawlog in _COLUMNS:
        o = R.replace(MFA, add_pov_feature=pov, add_normalized_log_pitch=norm, add_raw_log_pitch=rawlog)
        configure(pe, o)
        keep = [j for j, on in enumerate((pov, norm, rawlog)) if on]
        assert pe.num_pitch_cols == len(keep)
        d_raw = torch.from_numpy(np.concatenate([d["raw"] for d in c["dev"]])).to(pe.device)
        got = pe.pitch_process(d_raw, fo).cpu().numpy()
        got_chirp = pe.pitch_process(torch.from_numpy(cd[0]["raw"]).to(pe.device), cinfo["fo"]).cpu().numpy()
        worst = 0.0
        for k, want in zip(pick, ref64):
            worst = max(worst, float(np.abs(got[fo[k]: fo[k + 1]] - want[:, keep]).max()))
        worst = max(worst, float(np.abs(got_chirp - ref64[-1][:, keep]).max()))
        print(f"columns {keep}: device against float64 {worst:.3e}")
        assert worst <= 4 * yard, (keep, worst, yard)
        # engine.pitch is the two calls in a row
        whole = pe.pitch(c["info"]["pcm"], so).cpu().numpy()
        assert np.array_equal(whole.view(np.uint32), got.view(np.uint32))
    # written into a wider matrix: the other columns stay untouched
    configure(pe, MFA)
    wide = torch.full((int(fo[-1]), 16), 9.0, dtype=torch.float32, device=pe.device)
    pe.pitch_process(d_raw, fo, wide, 13)
    w = wide.cpu().numpy()
    assert np.all(w[:, :13] == 9.0) and np.all(w[:, 15] == 9.0)
    assert np.array_equal(w[:, 13:15], pe.pitch_process(d_raw, fo).cpu().numpy())
