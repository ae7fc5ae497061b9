"""The device resampler (resample.hip, mfa_resample_batch) against the float64 restatement of tests/test_resample_cpu.py,
then through every layer above it: engine.resample on mixed batches, CorpusAligner on a corpus of mixed rates (exactly the
results of the same corpus converted beforehand) and the kalpy layer (Segment, MfccComputer, export_feats).

Error model of the kernel test.  The device sums acc = fmaf(w_j, x_j, acc) in float32 over float32 weights, the
restatement in float64 over float64 weights.  For output k with taps_k taps, b_k = (taps_k + 2)·2⁻²⁴·Σ_j |w_j·x_j| bounds the
difference: taps_k roundings of the running sum plus one for each weight (standard forward bound, unit round-off 2⁻²⁴).
The stored sample is rint(acc), so |d_k − clip(y_k)| ≤ 0.5 + b_k always, and d_k = rint(y_k) exactly unless y_k lies within
b_k of a half-integer.  At most 3 % of a rate pair's samples may lie in that band (on these signals the device, and a float32
emulation of its chain on the CPU, put 0.35 – 1.56 % there; the test prints the share of each rate pair)."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.test_resample_cpu import MODEL_HZ, RATES, num_out, plan, resample_ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345


def _signal(rng, n, fin):
    t = np.arange(n) / fin
    x = 3000.0 * np.sin(2 * np.pi * 310.0 * t + 0.3) + 1500.0 * np.sin(2 * np.pi * 2210.0 * t + 1.1) + 400.0 * rng.normal(size=n)
    return np.rint(x).astype(np.int16)


def _inputs_for(count, fin):
    """Fewest input samples that give at least ``count`` outputs (exactly ``count`` when downsampling; upsampling by two
    reaches every other count only)."""
    n = max(0, (count * fin) // MODEL_HZ - 2)
    while num_out(n, fin) < count:
        n += 1
    return n


_CASES = {}


def _case(engine, fin):
    """The utterances of one rate pair — every length class, back to back — with the restatement's outputs and the
    device's (one mfa_resample_batch call into a buffer that carries 64 sentinel samples past its end).  Computed once."""
    if fin in _CASES:
        return _CASES[fin]
    rng = np.random.default_rng(fin)
    p = plan(fin)
    block = engine.resample_block_outputs()
    around = list(dict.fromkeys(_inputs_for(block + d, fin) for d in (-2, -1, 0, 1, 2)))   # a workgroup's share − 1, exact, + 1
    assert {block - 1, block, block + 1} <= {num_out(n, fin) + d for n in around for d in (-1, 0, 1)}
    assert min(num_out(n, fin) for n in around) < block < max(num_out(n, fin) for n in around)
    lens = [0, 1, 2, p.max_taps - 1, p.in_per_unit] + around + [int(0.3 * fin) + 1]
    utts = [_signal(rng, n, fin) for n in lens]
    utts.append(np.zeros(777, dtype=np.int16))                                        # silence stays silence
    sq = np.where((np.arange(1501) // 37) % 2 == 0, 32767, -32767).astype(np.int16)   # full scale: the filter overshoots, the store clamps
    utts.append(sq)
    kinds = ["signal"] * len(lens) + ["zero", "clamp"]
    so = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    assert {int(o) % 2 for o in so[:-1]} == {0, 1}                                    # input offsets of both parities
    oo = np.concatenate([[0], np.cumsum([num_out(len(u), fin) for u in utts])]).astype(np.int64)
    d_in = torch.from_numpy(np.concatenate(utts)).to(engine.device)
    d_out = torch.full((int(oo[-1]) + 64,), SENTINEL, dtype=torch.int16, device=engine.device)
    d_so, d_oo = torch.from_numpy(so).to(engine.device), torch.from_numpy(oo).to(engine.device)
    d_sel = torch.arange(len(utts), dtype=torch.int32, device=engine.device)
    engine.configure_mfcc()
    rc = engine.lib.mfa_resample_batch(engine.ctx, fin, MODEL_HZ, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_so.data_ptr()),
                                       C.c_void_p(d_out.data_ptr()), C.c_void_p(d_oo.data_ptr()), C.c_void_p(d_sel.data_ptr()),
                                       len(utts), int(np.diff(oo).max()))
    assert rc == 0, engine.lib.mfa_last_error(engine.ctx)
    torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    got = [flat[oo[k]: oo[k + 1]].copy() for k in range(len(utts))]
    ref = [resample_ref(u, fin) for u in utts]
    _CASES[fin] = dict(utts=utts, kinds=kinds, so=so, oo=oo, got=got, ref=ref, tail=flat[oo[-1]:].copy(), d_in=d_in)
    return _CASES[fin]


@pytest.mark.parametrize("fin", RATES)
def test_kernel_matches_restatement(engine, fin):
    c = _case(engine, fin)
    assert np.all(c["tail"] == SENTINEL) and c["tail"].shape[0] == 64          # nothing written past the batch's end
    in_band = total = 0
    for u, kind, got, (y, mag, taps) in zip(c["utts"], c["kinds"], c["got"], c["ref"]):
        assert got.shape[0] == y.shape[0] == num_out(len(u), fin)
        if not y.shape[0]:
            continue
        b = (taps + 2) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - np.clip(y, -32768.0, 32767.0))
        assert np.all(err <= 0.5 + b), (fin, kind, len(u), float((err - b).max()))
        if kind == "zero":
            assert not got.any()
        if kind == "clamp":
            assert got.max() == 32767 and got.min() == -32768 and np.abs(y).max() > 32768.0   # the clamp was needed
            continue
        frac = np.abs(y - np.floor(y) - 0.5)
        clear = frac > b
        assert np.array_equal(got[clear].astype(np.float64), np.rint(y[clear])), (fin, kind, len(u))
        in_band += int((~clear).sum()); total += int(y.shape[0])
    share = in_band / total
    print(f"resample {fin} Hz -> {MODEL_HZ} Hz: {in_band} of {total} samples ({100 * share:.2f} %) within b_k of a half-integer")
    assert share <= 0.03, share
    # the engine's call allocates its own buffer and gives the same samples
    out, oo = engine.resample(c["d_in"], c["so"], [fin] * len(c["utts"]))
    assert np.array_equal(oo, c["oo"]) and np.array_equal(out.cpu().numpy(), np.concatenate(c["got"]))
    assert [engine.num_resampled(len(u), fin) for u in c["utts"]] == np.diff(c["oo"]).tolist()


def test_refusals_on_the_device_entry(engine):
    lib, ctx = engine.lib, engine.ctx
    z = torch.zeros(8, dtype=torch.int64, device=engine.device)
    p = C.c_void_p(z.data_ptr())
    for fin, fout, n_sel, word in [(999, 16000, 1, "1000"), (16000, 384001, 1, "384000"), (16000, 16000, 1, "both"),
                                   (44100, 16000, 65536, "65535")]:
        assert lib.mfa_resample_batch(ctx, fin, fout, p, p, p, p, p, n_sel, 1) != 0
        assert word in lib.mfa_last_error(ctx).decode()
    with pytest.raises(Exception):
        engine.num_resampled(10, 500)


def test_mixed_rates_in_one_call(engine):
    """16 k, 44.1 k and 8 k utterances interleaved: the converted ones equal the single-rate batches' results, the 16 k ones
    come back bit for bit, and a second run gives the same bytes."""
    a, b = _case(engine, 44100), _case(engine, 8000)
    rng = np.random.default_rng(5)
    utts, rates, want = [], [], []
    for k in range(max(len(a["utts"]), len(b["utts"]))):
        own = rng.integers(-32768, 32768, size=(0, 1, 5000, 333)[k % 4]).astype(np.int16)
        utts.append(own); rates.append(None if k % 2 else MODEL_HZ); want.append(own)
        for c, r in ((a, 44100), (b, 8000)):
            if k < len(c["utts"]):
                utts.append(c["utts"][k]); rates.append(r); want.append(c["got"][k])
    so = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    d = torch.from_numpy(np.concatenate(utts)).to(engine.device)
    out, oo = engine.resample(d, so, rates)
    host = out.cpu().numpy()
    for k, w in enumerate(want):
        assert np.array_equal(host[oo[k]: oo[k + 1]], w), (k, rates[k], len(utts[k]))
    out2, oo2 = engine.resample(d, so, rates)
    assert np.array_equal(oo, oo2) and torch.equal(out, out2)
    # nothing to convert: the batch comes back as it is
    same, so_same = engine.resample(d, so, [None] * len(utts))
    assert same is d and np.array_equal(so_same, so)


CUTS = [("spkA", 0.0, 4.0, "this is the acoustic corpus i'm talking pretty fast here"),
        ("spkA", 4.0, 6.5, "there's nothing going else going on"),
        ("spkB", 23.5, 26.72, "um and that should be all thanks")]


def _at_rate(x16, rate):
    """A host-made input at another rate (its fidelity does not matter: it is merely an input)."""
    from math import gcd
    from scipy.signal import resample_poly

    g = gcd(rate, MODEL_HZ)
    y = resample_poly(x16.astype(np.float64), rate // g, MODEL_HZ // g)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def test_corpus_of_mixed_rates_equals_the_converted_corpus(engine, fx, tmp_path):
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance

    engine.configure_mfcc()
    native = []
    for k, (spk, a, b, text) in enumerate(CUTS):
        x16 = fx.pcm[int(a * MODEL_HZ): int(b * MODEL_HZ)]
        for rate in ((None, 44100), (44100, 8000), (8000, MODEL_HZ))[k]:
            x = x16 if rate in (None, MODEL_HZ) else _at_rate(x16, rate)
            if rate == 44100:
                x = x[: len(x) // 441 * 441]                    # a whole number of units: both runs see the same duration
            native.append(CorpusUtterance(f"{spk}-{k}-{rate}", spk, x, text, sample_rate=rate))
    odd = _at_rate(fx.pcm[int(4.0 * MODEL_HZ): int(6.5 * MODEL_HZ)], 44100)
    odd = odd[: len(odd) // 441 * 441 - 100]                    # not a whole number of units
    native.append(CorpusUtterance("spkB-odd", "spkB", odd, CUTS[1][3], sample_rate=44100))
    assert len(native) == 7 and len(odd) % 441
    converted = []
    for u in native:
        d = torch.from_numpy(u.pcm.copy()).to(engine.device)
        out, _ = engine.resample(d, np.array([0, len(u.pcm)], dtype=np.int64), [u.sample_rate])
        converted.append(CorpusUtterance(u.utt_id, u.speaker, out.cpu().numpy(), u.text))
    al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=engine,
                       options=AlignOptions(beam=100.0, retry_beam=400.0, batch_frames=900))
    assert al._batches(native) == al._batches(converted) and len(al._batches(native)) > 1
    res_n = al.align(native)
    failed_n = list(al.failed)
    paths_n = al.export_textgrids(native, res_n, tmp_path / "native")
    res_c = al.align(converted)
    paths_c = al.export_textgrids(converted, res_c, tmp_path / "converted")
    assert failed_n == al.failed == []
    for u, rn, rc in zip(native, res_n, res_c):
        assert np.array_equal(rn.alignment, rc.alignment) and np.array_equal(rn.words, rc.words), u.utt_id
        assert np.float32(rn.likelihood).tobytes() == np.float32(rc.likelihood).tobytes() and rn.num_frames == rc.num_frames
    by_name = {p.name: p for p in paths_c}
    assert sorted(p.name for p in paths_n) == sorted(by_name) and len(paths_n) == 7
    for p in paths_n:
        if p.name.startswith("spkB-odd"):
            assert "xmax = %s" % round(len(odd) / 44100, 6) in p.read_text(encoding="utf8")
        else:
            assert p.read_bytes() == by_name[p.name].read_bytes(), p.name


def _write_wav(path, x, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(x, dtype="<i2").tobytes())
    return path


def test_kalpy_layer_converts_segments(engine, fx, tmp_path):
    from montreal_forced_aligner_amd import kaldi_io, kalpy_api as K

    x16 = fx.pcm[: 3 * MODEL_HZ]
    x44, x8 = _at_rate(x16, 44100), _at_rate(x16, 8000)
    w44, w8, w16 = (_write_wav(tmp_path / f"a{r}.wav", x, r) for x, r in ((x44, 44100), (x8, 8000), (x16, MODEL_HZ)))
    eng = K.get_engine()
    eng.configure_mfcc()

    def converted(x, rate):
        out, _ = eng.resample(torch.from_numpy(x.copy()).to(eng.device), np.array([0, len(x)], dtype=np.int64), [rate])
        return out.cpu().numpy()

    mc = K.MfccComputer(allow_downsample=True, allow_upsample=True)
    seg = K.Segment(w44)
    got = mc.compute_mfccs(seg)
    assert seg.sample_rate == 44100
    y = converted(x44, 44100)
    ref = O.mfcc(y.astype(np.float32), O.default_mfcc_opts())
    assert got.shape == ref.shape and float(np.abs(got - ref).max()) < 2e-3        # the tolerance of test_gpu_parity's MFCC test
    assert np.array_equal(got, mc.compute_mfccs(y))
    # begin / end cut at the file's own rate, then the cut is converted
    cut = K.Segment(w44, begin=0.5, end=1.5)
    assert np.array_equal(cut.load_audio(), converted(x44[round(0.5 * 44100): round(1.5 * 44100)], 44100))
    assert np.array_equal(K.Segment(w16, begin=0.5, end=1.5).load_audio(), x16[8000:24000])
    assert np.array_equal(K.Segment(w8).load_audio(), converted(x8, 8000))
    # one batch of mixed rates through export_feats = the per-segment calls
    segs = [("u44", K.Segment(w44)), ("u16", K.Segment(w16)), ("u8", K.Segment(w8, begin=0.25)), ("ucut", cut), ("uarr", x16[:5000])]
    mc.export_feats(tmp_path / "feats.ark", segs, compress=False)
    table = dict(kaldi_io.read_ark((tmp_path / "feats.ark").read_bytes(), "matrix"))
    assert list(table) == [k for k, _ in segs]
    for key, s in segs:
        assert np.array_equal(table[key], mc.compute_mfccs(s)), key
