"""The device feature codec (csrc/compress.hip, mfa_compress_batch) against its specification, kaldi_io's
write_compressed_matrix / _read_compressed: Kaldi's CompressedMatrix, method kOneByteWithColHeaders.  Everything here is
bit identity (np.array_equal on values, == on records), never a tolerance: the round-tripped matrix, the record assembled
from the device's headers and bytes, the fused CMVN trip — over ragged batches whose lengths sit on the small-matrix rule,
on wavefront and workgroup edges and on both sides of the LDS-resident bound, over widths that take one to twelve rounds of
the workgroup's four wavefronts, and over the value patterns where the clamps, ties and branch edges of the codec live.
Then the layers above: CorpusAligner(corpus_compression=True) and MfccComputer.export_feats never reach the host codec."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def mfcc_like(rng, rows, dim):
    """float32 [rows, dim] scaled like MFCCs: column 0 around ±50, the others ±15."""
    m = rng.standard_normal((rows, dim)) * 15.0
    m[:, 0] *= 50.0 / 15.0
    return m.astype(np.float32)


def host_record(m):
    from montreal_forced_aligner_amd import kaldi_io as K

    buf = io.BytesIO()
    with np.errstate(all="ignore"):            # (a piece whose percentile floats coincide divides by zero on the host, too)
        K.write_compressed_matrix(buf, np.ascontiguousarray(m, dtype=np.float32))
    return buf.getvalue()


def host_round_trip(m):
    from montreal_forced_aligner_amd import kaldi_io as K

    with np.errstate(all="ignore"):
        return K.compress_round_trip(np.ascontiguousarray(m, dtype=np.float32))


def batch_of(tables, dim):
    lens = [t.shape[0] for t in tables]
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = np.concatenate([t.reshape(-1, dim) for t in tables]).astype(np.float32) if fo[-1] else np.zeros((0, dim), np.float32)
    return x, fo


def check_batch(engine, x, fo, cols=None):
    """Round trip and record of every utterance of the batch, columns ``cols``, against the host codec."""
    import torch
    from montreal_forced_aligner_amd import kaldi_io as K

    c0, c1 = (0, x.shape[1]) if cols is None else cols
    nc = c1 - c0
    d = torch.from_numpy(x).to(engine.device)
    got = engine.compress_round_trip(d, fo, cols=cols).cpu().numpy()
    glob, colhdr, data = (t.cpu().numpy() for t in engine.compress(d, fo, cols=cols))
    assert np.array_equal(d.cpu().numpy(), x)                                     # the input is left alone
    assert colhdr.dtype == np.uint16 and data.dtype == np.uint8 and glob.dtype == np.float32
    outside = np.ones(x.shape[1], dtype=bool)
    outside[c0:c1] = False
    assert np.array_equal(got[:, outside].view(np.uint32), x[:, outside].view(np.uint32))
    for k in range(len(fo) - 1):
        a, b = int(fo[k]), int(fo[k + 1])
        if b == a:
            continue
        table = np.ascontiguousarray(x[a:b, c0:c1])
        want = host_round_trip(table)
        assert np.array_equal(got[a:b, c0:c1], want), (k, b - a, int((got[a:b, c0:c1] != want).sum()))
        buf = io.BytesIO()
        K.write_compressed_parts(buf, glob[k], colhdr[k], data[a * nc: b * nc], b - a, nc)
        assert buf.getvalue() == host_record(table), (k, b - a)
    return got


def test_row_counts_in_one_ragged_batch(engine):
    """The small-matrix rule (1-4 rows), q = 1 and 2, wavefront and workgroup edges, the resident bound − 1, the bound, + 1 and
    a table well past it, all in one batch with an utterance without rows in the middle."""
    dim = 13
    bound = engine.compress_resident_values() // dim
    assert bound >= 1000                     # a ten-second utterance is resident
    lens = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 0, 255, 256, 257, 1000, bound - 1, bound, bound + 1, bound + bound // 2 + 3]
    rng = np.random.default_rng(7)
    x, fo = batch_of([mfcc_like(rng, n, dim) for n in lens], dim)
    check_batch(engine, x, fo)


@pytest.mark.parametrize("dim,ranges", [(1, [None]), (13, [None]), (16, [(0, 13), (13, 16)]), (40, [None, (5, 18)]), (45, [None])])
def test_widths_and_column_ranges(engine, dim, ranges):
    """One to twelve rounds of the four wavefronts; 40 × 1000 is past the resident bound.  Columns outside the range are the
    input's, bit for bit."""
    rng = np.random.default_rng(100 + dim)
    x, fo = batch_of([mfcc_like(rng, n, dim) for n in (300, 0, 7, 1000, 4)], dim)
    for cols in ranges:
        check_batch(engine, x, fo, cols)


def value_tables():
    rng = np.random.default_rng(11)
    rows, dim = 200, 5
    out = {}
    out["constant table"] = np.full((rows, dim), -7.25, dtype=np.float32)           # max == min: range 1 + |min|
    out["constant table of zeros"] = np.zeros((9, 2), dtype=np.float32)
    t = mfcc_like(rng, rows, dim)
    t[:, 2] = 3.5                                                                    # the +1 clamps of p25, p75, p100
    t[:, 4] = t[:, 0].max()                                                          # … against the top of the range
    out["constant columns"] = t
    t = mfcc_like(rng, rows, dim)
    t[:, 1] = rng.choice(np.array([-4.0, 0.5, 9.0], dtype=np.float32), size=rows, p=[0.6, 0.3, 0.1])
    t[:, 3] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=rows)
    out["ties"] = t
    # a column whose values ARE its percentile floats (the branch edges x < f25, x < f75); column 0 owns the global range
    t = mfcc_like(rng, rows, dim)
    t[0, 0], t[1, 0] = -80.0, 80.0
    rec = host_record(t)
    mn, rg = np.frombuffer(rec[3:11], dtype="<f4")
    hdr = np.frombuffer(rec[19: 19 + 8 * dim], dtype="<u2").reshape(dim, 4)
    inc = np.float32(rg * np.float32(1.0 / 65535.0))
    f = np.array([np.float32(mn + inc * np.float32(c)) for c in hdr[2]], dtype=np.float32)
    col = np.repeat(f, [30, 80, 60, 30])                                             # sorted[50] = f25, sorted[150] = f75
    t[:, 2] = rng.permutation(col)
    out["values on the percentile floats"] = t
    t = mfcc_like(rng, rows, dim)
    t[:, 1] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], dtype=np.float32), size=rows)
    t[:, 3] = np.where(rng.random(rows) < 0.5, np.float32(-0.0), np.float32(0.0))
    assert np.signbit(t[:, 3]).any() and not np.signbit(t[:, 3]).all()
    out["signed zeros"] = t
    out["range 1e-3"] = rng.uniform(0.0, 1e-3, (rows, dim)).astype(np.float32)
    out["range 1e-3 at 50"] = (50.0 + rng.uniform(0.0, 1e-3, (rows, dim))).astype(np.float32)   # percentile floats coincide
    out["range 1e4"] = rng.uniform(-5e3, 5e3, (rows, dim)).astype(np.float32)
    for name, m in out.items():                                                      # (the host codec accepts each of them)
        assert host_round_trip(m).shape == m.shape, name
    return out


def test_value_patterns(engine):
    for name, m in value_tables().items():
        fo = np.array([0, m.shape[0]], dtype=np.int64)
        try:
            check_batch(engine, m, fo)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


def test_fused_cmvn_second_trip(engine):
    """compress_round_trip(x − mean) with the mean as CorpusAligner._final_features has it: (sum / count) in float64 rounded to
    float32, per speaker; once with the MFCC's own statistics, once with the zero-padded statistics of a use_pitch model
    (16-wide base matrix, the MFCC columns alone make the trip)."""
    import torch

    rng = np.random.default_rng(5)
    lens = [300, 64, 0, 1000, 5, 2, 1100]
    u2s = np.array([0, 1, 1, 0, 1, 0, 1], dtype=np.int32)
    for dim, n_pitch in ((13, 0), (16, 3)):
        nc = dim - n_pitch
        x, fo = batch_of([mfcc_like(rng, n, dim) + np.float32(3.0) for n in lens], dim)
        d = torch.from_numpy(x).to(engine.device)
        stats = engine.cmvn_stats(d[:, :nc].contiguous(), fo, u2s, 2)
        if n_pitch:
            stats = engine.pad_cmvn_stats(stats, n_pitch)
        got = engine.compress_round_trip(d, fo, cols=(0, nc), cmvn=stats, utt2spk=u2s).cpu().numpy()
        st = stats.cpu().numpy()
        assert np.array_equal(got[:, nc:].view(np.uint32), x[:, nc:].view(np.uint32))
        for k in range(len(lens)):
            a, b = int(fo[k]), int(fo[k + 1])
            if b > a:
                mean = (st[u2s[k]][0, :nc] / st[u2s[k]][0, -1]).astype(np.float32)
                assert np.array_equal(got[a:b, :nc], host_round_trip(x[a:b, :nc] - mean)), (dim, k)


def test_refusals_leave_the_context_usable(engine):
    import torch
    from montreal_forced_aligner_amd._lib import MfaHipError

    rng = np.random.default_rng(3)
    x, fo = batch_of([mfcc_like(rng, n, 16) for n in (40, 9)], 16)
    d = torch.from_numpy(x).to(engine.device)
    u2s = np.zeros(2, dtype=np.int32)
    stats13 = engine.cmvn_stats(d[:, :13].contiguous(), fo, u2s, 1)

    def good():
        got = engine.compress_round_trip(d, fo, cols=(0, 13), cmvn=stats13, utt2spk=u2s).cpu().numpy()
        mean = (stats13.cpu().numpy()[0][0, :13] / stats13.cpu().numpy()[0][0, -1]).astype(np.float32)
        assert np.array_equal(got[:40, :13], host_round_trip(x[:40, :13] - mean))

    with pytest.raises(MfaHipError, match="may not be the input"):
        engine.compress_round_trip(d, fo, out=d)
    good()
    for cols in ((5, 20), (7, 7), (-1, 4), (9, 3)):
        with pytest.raises(MfaHipError, match="do not lie inside a row"):
            engine.compress_round_trip(d, fo, cols=cols)
        with pytest.raises(MfaHipError, match="do not lie inside a row"):
            engine.compress(d, fo, cols=cols)
    good()
    with pytest.raises(MfaHipError, match="do not cover columns"):       # statistics of 13 columns for a 16-wide table
        engine.compress_round_trip(d, fo, cmvn=stats13, utt2spk=u2s)
    good()
    assert np.array_equal(d.cpu().numpy(), x)


def two_utterances(fx):
    from montreal_forced_aligner_amd.aligner import CorpusUtterance

    sr = 16000
    cuts = [("spkA", 0.0, 4.2, "this is the acoustic corpus i'm talking pretty fast here"),
            ("spkA", 4.0, 6.5, "there's nothing going else going on")]
    return [CorpusUtterance(f"{s}-{k}", s, fx.pcm[int(a * sr): int(b * sr)], t) for k, (s, a, b, t) in enumerate(cuts)]


def test_corpus_aligner_never_reaches_the_host_codec(engine, fx, monkeypatch):
    """corpus_compression=True with kaldi_io.compress_round_trip made to raise: the same alignments and likelihoods as before
    the patch, and the features the aligner decodes are those of the host detour (computed here before the patch), bit for bit."""
    import torch
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner

    utts = two_utterances(fx)

    def aligner():
        return CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=engine,
                             options=AlignOptions(beam=100.0, retry_beam=400.0, corpus_compression=True))

    before = aligner().align(utts, make_ctm=False)
    assert all(r is not None for r in before)
    # the host detour on the same MFCCs: round trip, CMVN statistics of the result, mean off, second round trip
    so = np.concatenate([[0], np.cumsum([len(u.pcm) for u in utts])]).astype(np.int64)
    mfcc, fo = engine.mfcc(torch.from_numpy(np.concatenate([u.pcm for u in utts])).to(engine.device), so)
    host = mfcc.cpu().numpy().copy()
    for k in range(2):
        host[fo[k]: fo[k + 1]] = K.compress_round_trip(host[fo[k]: fo[k + 1]])
    u2s = np.zeros(2, dtype=np.int32)
    stats = engine.cmvn_stats(torch.from_numpy(host).to(engine.device), fo, u2s, 1)
    st = stats.cpu().numpy()[0]
    mean = (st[0, :13] / st[0, -1]).astype(np.float32)
    twice = host.copy()
    for k in range(2):
        twice[fo[k]: fo[k + 1]] = K.compress_round_trip(host[fo[k]: fo[k + 1]] - mean)
    want = engine.features(torch.from_numpy(twice).to(engine.device), fo, u2s, None).cpu().numpy()

    def refuse(*a, **k):
        raise AssertionError("the host codec was called on the corpus path")

    monkeypatch.setattr(K, "compress_round_trip", refuse)
    monkeypatch.setattr(K, "write_compressed_matrix", refuse)
    al = aligner()
    after = al.align(utts, make_ctm=False)
    for a, b in zip(before, after):
        assert b is not None and np.array_equal(a.alignment, b.alignment) and np.array_equal(a.words, b.words)
        assert a.per_frame_likelihood == b.per_frame_likelihood
    once, fo2 = al._mfcc(utts, [0, 1])
    assert np.array_equal(fo2, fo) and np.array_equal(once.cpu().numpy(), host)
    got = al._final_features(once, fo2, u2s, stats, None, None).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(once.cpu().numpy(), host)          # the once-compressed matrix survives the second trip


def test_export_feats_writes_the_host_codecs_ark(engine, fx, tmp_path, monkeypatch):
    from montreal_forced_aligner_amd import kaldi_io as K
    from montreal_forced_aligner_amd import kalpy_api as KA

    mc = KA.MfccComputer(sample_frequency=16000, frame_length=25, frame_shift=10, num_mel_bins=23, num_coefficients=13,
                         snip_edges=False, dither=0.0, use_energy=False)
    segs = [(f"utt{k}", u.pcm) for k, u in enumerate(two_utterances(fx))]
    with open(tmp_path / "host.ark", "wb") as f:
        for key, pcm in segs:
            K.write_ark_entry(f, key, mc.compute_mfccs(pcm), "compressed_matrix")

    def refuse(*a, **k):
        raise AssertionError("the host codec was called by export_feats")

    monkeypatch.setattr(K, "write_compressed_matrix", refuse)
    mc.export_feats(tmp_path / "dev.ark", segs, write_scp=True, compress=True)
    assert (tmp_path / "dev.ark").read_bytes() == (tmp_path / "host.ark").read_bytes()
    monkeypatch.undo()
    lines = (tmp_path / "dev.scp").read_text(encoding="utf8").split("\n")[:-1]
    data = (tmp_path / "dev.ark").read_bytes()
    for line, (key, pcm) in zip(lines, segs):
        k, where = line.split(" ")
        off = int(where.rsplit(":", 1)[1])
        assert k == key and data[off: off + 5] == b"\0BCM "
