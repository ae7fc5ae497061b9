"""Host side of the feature codec: kaldi_io.write_compressed_parts against write_compressed_matrix, the ABI's entry
points, the library's host restatement of the kernel's arithmetic (csrc/compress_math.hpp, the very functions the kernel
runs, compiled for the host) against kaldi_io bit for bit — and the specification itself pinned where it is asymmetric:
the writer's percentile floats use f32(range · f32(1/65535)), the reader's f32(double(range) · double(1/65535))."""
import io
import struct

import numpy as np
import pytest

from montreal_forced_aligner_amd import kaldi_io as K


def record(m):
    buf = io.BytesIO()
    with np.errstate(all="ignore"):
        K.write_compressed_matrix(buf, m)
    return buf.getvalue()


def split(raw, rows, cols):
    """The writer's record cut into its parts: token, global header, column headers, bytes."""
    assert raw[:3] == b"CM " and struct.unpack("<ii", raw[11:19]) == (rows, cols)
    glob = np.frombuffer(raw[3:11], dtype="<f4")
    colhdr = np.frombuffer(raw[19: 19 + 8 * cols], dtype="<u2").reshape(cols, 4)
    data = np.frombuffer(raw[19 + 8 * cols:], dtype=np.uint8).reshape(cols, rows)
    return glob, colhdr, data


def mfcc_like(rng, rows, dim):
    m = rng.standard_normal((rows, dim)) * 15.0
    m[:, 0] *= 50.0 / 15.0
    return m.astype(np.float32)


def test_write_compressed_parts_reproduces_the_writer():
    rng = np.random.default_rng(0)
    for rows, cols in ((1, 1), (4, 3), (5, 13), (257, 13), (1000, 16)):
        m = mfcc_like(rng, rows, cols)
        raw = record(m)
        glob, colhdr, data = split(raw, rows, cols)
        buf = io.BytesIO()
        K.write_compressed_parts(buf, glob, colhdr, data, rows, cols)
        assert buf.getvalue() == raw
        buf = io.BytesIO()                                   # flat bytes, as the device hands them over
        K.write_compressed_parts(buf, glob.copy(), colhdr.reshape(-1).copy(), data.reshape(-1).copy(), rows, cols)
        assert buf.getvalue() == raw
        r = K.BinaryReader(raw)
        assert np.array_equal(K._read_compressed(r, r.token()), K.compress_round_trip(m))
    m = mfcc_like(rng, 8, 2)
    glob, colhdr, data = split(record(m), 8, 2)
    for bad in (dict(rows=0), dict(cols=0), dict(rows=7), dict(cols=3), dict(colhdr=colhdr.astype(np.int32)),
                dict(data=data.astype(np.int16)), dict(glob=np.zeros(3, np.float32))):
        kw = dict(glob=glob, colhdr=colhdr, data=data, rows=8, cols=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.write_compressed_parts(io.BytesIO(), kw["glob"], kw["colhdr"], kw["data"], kw["rows"], kw["cols"])


def _lib():
    from montreal_forced_aligner_amd import _lib as L

    L.build_native()
    return L


def test_abi_lists_the_codec_entry_points():
    L = _lib()
    lib = L.lib()
    names = {"mfa_compress_batch", "mfa_compress_resident_values", "mfa_debug_compress_host"}
    assert names <= set(L.SIGNATURES) and all(hasattr(lib, n) for n in names)
    assert len(L.SIGNATURES["mfa_compress_batch"][1]) == 14
    assert lib.mfa_compress_resident_values() >= 1000 * 13          # a ten-second utterance's MFCC table is LDS resident
    assert "compress.hip" in L._SOURCES


def host_restatement(lib, m):
    m = np.ascontiguousarray(m, dtype=np.float32)
    rows, cols = m.shape
    glob, colhdr = np.zeros(2, np.float32), np.zeros((cols, 4), np.uint16)
    data, out = np.zeros((cols, rows), np.uint8), np.zeros((rows, cols), np.float32)
    assert lib.mfa_debug_compress_host(m.ctypes.data, rows, cols, glob.ctypes.data, colhdr.ctypes.data, data.ctypes.data,
                                       out.ctypes.data) == 0
    return glob, colhdr, data, out


def test_kernel_arithmetic_on_the_host_is_the_codecs():
    """The functions the kernel runs (header codes, both sets of percentile floats, byte, value), compiled for the host and
    fed order statistics from a sort: the writer's record and the reader's matrix, bit for bit, over the row counts of the
    small-matrix rule, scales from 1e-4 to 1e4, constant tables and columns, ties, and ranges so narrow at their offset that
    percentile floats coincide (the writer then divides by zero)."""
    lib = _lib().lib()
    rng = np.random.default_rng(0)
    tables = [mfcc_like(rng, rows, cols) for rows in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257, 1000) for cols in (1, 13)]
    for t in range(120):
        rows, cols = int(rng.integers(1, 300)), int(rng.integers(1, 6))
        m = (rng.standard_normal((rows, cols)) * 10.0 ** rng.uniform(-4, 4) + rng.choice([0.0, 50.0, -1e3, 1e-3])).astype(np.float32)
        if t % 5 == 0:
            m[:, 0] = m[0, 0]
        if t % 7 == 0:
            m = np.round(m) + np.float32(0.5)          # heavy ties (the offset keeps signed zeros out of the table minimum)
        if t % 11 == 0:
            m[:] = m[0, 0]
        tables.append(m)
    tables.append((50.0 + rng.uniform(0.0, 1e-3, (200, 5))).astype(np.float32))
    tables.append(rng.uniform(-5e3, 5e3, (200, 5)).astype(np.float32))
    for m in tables:
        glob, colhdr, data, out = host_restatement(lib, m)
        buf = io.BytesIO()
        K.write_compressed_parts(buf, glob, colhdr, data, *m.shape)
        assert buf.getvalue() == record(m), m.shape
        with np.errstate(all="ignore"):
            assert np.array_equal(out, K.compress_round_trip(m)), m.shape
    assert lib.mfa_debug_compress_host(None, 0, 3, None, None, None, None) != 0


def test_writer_and_reader_increments_stay_asymmetric():
    """One constructed range on which f32(range · f32(1/65535)) and f32(double(range) · double(1/65535)) differ in the last
    bit, a header code of 2^15 (the product with either increment is exact), and one value whose byte is 2 with the writer's
    increment and 1 with the reader's.  A "clean-up" of kaldi_io that makes the two sides agree moves the specification the
    device codec is held to, and fails here."""
    f32 = np.float32
    rng_v, x = f32(129.4984588623047), f32(1.5175831317901611)
    inc_w, inc_r = f32(rng_v * f32(1.0 / 65535.0)), f32(float(rng_v) * (1.0 / 65535.0))
    assert inc_w != inc_r and abs(float(inc_w) - float(inc_r)) <= float(np.spacing(inc_w))
    v = f32(float(rng_v) * 0.500012)
    m = np.array([[0], [x], [v], [v], [v], [v], [rng_v], [rng_v]], dtype=np.float32)
    glob, colhdr, data = split(record(m), 8, 1)
    assert glob[0] == 0 and glob[1] == rng_v and colhdr.tolist() == [[0, 32768, 65534, 65535]]

    def low_piece_byte(inc):
        f25 = f32(inc * f32(32768))
        return int(np.int64(f32(f32(f32(x / f25) * f32(64)) + f32(0.5))))

    assert (low_piece_byte(inc_w), low_piece_byte(inc_r)) == (2, 1)
    assert data[0].tolist() == [0, 2, 64, 64, 64, 64, 255, 255]                    # the writer: f32 · f32
    # the reader: byte 64 gives back p25 = 0 + inc · 32768 with ITS increment
    back = K.compress_round_trip(m)
    assert back[2, 0] == f32(inc_r * f32(32768)) and back[2, 0] != f32(inc_w * f32(32768))
