"""GPU test that pins the MFCC kernel's output bits: a small seeded batch against tests/golden/mfcc_bits.npy.

The golden file holds the float32 bit patterns (uint32) that the build of commit b2a5780 ("Test training statistics at real
key counts and long segments") produced on an MI355X for `_configs()` × `_batch()`, in that order, frames concatenated.  It
was written by `python tests/test_gpu_mfcc_bits.py --write` with that commit's library.  Correctness is what the
oracle-tolerance tests check (tests/test_gpu_parity.py, tests/test_gpu_frontend_options.py); this file pins "unchanged", for
changes to mfcc.hip that claim to keep every rounding and every summation order.

The batch, per option set: utterances of 1, 3, 4, 5, 15, 16, 17, 127, 128 and 129 frames (a wavefront takes four frames at a
pass, a workgroup's passes and the last partial one are all hit), an utterance of odd length, so that the speech-like
utterance after it starts at an odd sample offset (the unaligned load path; the utterances before it start at even
offsets), one all-zero and one full-scale utterance.  Option sets: snip_edges 1 and 0 without energy (mfcc_kernel<13,false>),
and with energy, raw_energy 1 and 0 (mfcc_kernel<13,true>)."""
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "mfcc_bits.npy"
FRAMES = [1, 3, 4, 5, 15, 16, 17, 127, 128, 129]
WIN, SHIFT = 400, 160          # 25 ms / 10 ms at 16 kHz


def _configs():
    return [dict(snip_edges=1, use_energy=0), dict(snip_edges=0, use_energy=0),
            dict(snip_edges=1, use_energy=1, raw_energy=1), dict(snip_edges=0, use_energy=1, raw_energy=0)]


def _samples(frames, snip):
    return WIN + SHIFT * (frames - 1) if snip else SHIFT * frames


def _batch(snip):
    """(segments, expected frame counts)"""
    rng = np.random.default_rng(20260 + snip)
    segs = [rng.normal(0, 3000, _samples(f, snip)).astype(np.int16) for f in FRAMES]
    want = list(FRAMES)
    segs.append(rng.normal(0, 3000, _samples(7, snip) + 1).astype(np.int16)); want.append(7)          # odd length
    t = np.arange(_samples(5, snip))
    segs.append((8000 * np.sin(2 * np.pi * 220 * t / 16000) + rng.normal(0, 500, len(t))).astype(np.int16)); want.append(5)
    segs.append(np.zeros(_samples(3, snip), np.int16)); want.append(3)
    segs.append(np.where(rng.random(_samples(3, snip)) < 0.5, -32768, 32767).astype(np.int16)); want.append(3)
    return segs, np.array(want)


def _device_bits(engine):
    import torch
    out = []
    try:
        for opts in _configs():
            segs, want = _batch(opts["snip_edges"])
            so = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
            assert so[len(FRAMES)] % 2 == 0 and so[len(FRAMES) + 1] % 2 == 1       # even starts, then the odd one
            engine.configure_mfcc(**opts)
            m, fo = engine.mfcc(torch.from_numpy(np.concatenate(segs)).to(engine.device), so)
            assert np.array_equal(np.diff(fo), want), (opts, np.diff(fo))
            out.append(m.cpu().numpy().view(np.uint32))
    finally:
        engine.configure_mfcc()
    return np.concatenate(out)


@pytest.mark.gpu
def test_mfcc_bits_are_those_of_the_golden_file(engine):
    got = _device_bits(engine)
    want = np.load(GOLDEN)
    assert GOLDEN.stat().st_size < 100_000 and want.dtype == np.uint32
    assert got.shape == want.shape
    rows = np.flatnonzero((got != want).any(axis=1))
    print(f"{len(rows)} of {len(got)} frames differ from the golden file" + (f", first at row {rows[0]}" if len(rows) else ""))
    assert np.array_equal(got, want)


if __name__ == "__main__" and "--write" in sys.argv:
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from montreal_forced_aligner_amd.engine import AlignmentEngine
    out_path = Path(sys.argv[sys.argv.index("--write") + 1]) if len(sys.argv) > sys.argv.index("--write") + 1 else GOLDEN
    e = AlignmentEngine(0)
    try:
        bits = _device_bits(e)
    finally:
        e.close()
    np.save(out_path, bits)
    print(f"wrote {out_path}: {bits.shape}, {out_path.stat().st_size} bytes")
