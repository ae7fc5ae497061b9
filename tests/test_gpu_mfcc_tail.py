"""GPU test of the MFCC kernel's specialised tail (mfcc.hip, `mfcc_kernel<·,·,true>`: compile-time trip counts over
zero-padded tables, the reads of a stage batched, per-lane tables in [lane][entry] order) against the generic tail in the same
process: `mfa_mfcc_batch` reads MFA_MFCC_GENERIC at every call, and the two must agree bit for bit — every fmaf chain and every
summation order is the generic kernel's, an absent piece adds +0.0 to a sum that is never −0.0, a zero DCT weight multiplies a
finite value.

The batch is that of tests/test_gpu_mfcc_bits.py (1 … 129 frames, an odd sample offset, silence, full scale).  Option sets:
the four of that file, then sets that change the filterbank plan (pieces, rounds, pieces per bin), the table sizes or the
instantiation (13 or 16 sample pairs per lane, with and without energy).  Plans with more than eight pieces in a bin are
beyond the specialised tail's bound and must come back through the generic one with the same bits as under the switch.

40 mel bins: `mfa_mfcc_configure` refuses more than 32 (a lane finishes bins i and i + 16) and 40 × 13 DCT entries do not fit
its table of 384 either — before this kernel as after it.  The case stays here as what it is, a refusal that is the same
under both settings; 32 bins × 12 coefficients (72 pieces, 5 in a bin) is the widest filterbank the kernel takes."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from tests.test_gpu_mfcc_bits import _batch, _configs

pytestmark = pytest.mark.gpu

FIRST = [(f"bits_file_{k}", o) for k, o in enumerate(_configs())]
SECOND = [
    ("10_coefficients", dict(num_coefficients=10)),
    ("0_to_8000_hz", dict(low_frequency=0.0, high_frequency=8000.0)),               # 70 pieces
    ("20_ms_window", dict(frame_length_ms=20.0)),                                   # 320 samples: clear_tail
    ("30_ms_window", dict(frame_length_ms=30.0)),                                   # 16 sample pairs per lane
    ("30_ms_window_energy", dict(frame_length_ms=30.0, use_energy=1)),
    ("30_ms_window_energy_after_window", dict(frame_length_ms=30.0, use_energy=1, raw_energy=0)),
    ("no_lifter", dict(cepstral_lifter=0.0)),
    ("keep_dc_offset", dict(remove_dc_offset=0)),
    ("32_bins_12_coefficients", dict(num_mel_bins=32, num_coefficients=12)),        # 72 pieces, 5 in a bin, every DCT column
    ("20_bins", dict(num_mel_bins=20)),                                             # 8 pieces in a bin: at the bound
    ("snip_edges_20_bins", dict(num_mel_bins=20, snip_edges=1)),
]
BEYOND = [
    ("16_bins", dict(num_mel_bins=16)),                                             # 9 pieces in a bin
    ("5_bins_5_coefficients", dict(num_mel_bins=5, num_coefficients=5)),            # 19 pieces in a bin, 4 rounds
    ("5_bins_30_ms_energy", dict(num_mel_bins=5, num_coefficients=5, frame_length_ms=30.0, use_energy=1)),
]


def _run(engine, pcm, so):
    m, fo = engine.mfcc(pcm, so)
    return m.cpu().numpy().view(np.uint32), fo


def _both(engine, monkeypatch, opts):
    """(path taken without the switch, its bits, the bits under MFA_MFCC_GENERIC=1, frame offsets)"""
    segs, _ = _batch(opts.get("snip_edges", 0))
    so = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate(segs)).to(engine.device)
    try:
        engine.configure_mfcc(**opts)
        monkeypatch.delenv("MFA_MFCC_GENERIC", raising=False)
        path = engine.mfcc_path()
        got, fo = _run(engine, pcm, so)
        monkeypatch.setenv("MFA_MFCC_GENERIC", "1")
        assert engine.mfcc_path() == "generic"
        ref, fo_ref = _run(engine, pcm, so)
        monkeypatch.delenv("MFA_MFCC_GENERIC")
    finally:
        engine.configure_mfcc()
    assert np.array_equal(fo, fo_ref)
    return path, got, ref, fo


def _compare(name, path, got, ref, fo):
    assert got.shape == ref.shape and got.shape[0] == fo[-1] > 0
    rows = np.flatnonzero((got != ref).any(axis=1))
    print(f"{name}: {path} path, {len(rows)} of {len(got)} frames differ from MFA_MFCC_GENERIC=1"
          + (f", first at frame {rows[0]} (utterance {np.searchsorted(fo, rows[0], 'right') - 1})" if len(rows) else ""))
    assert np.array_equal(got, ref)
    assert np.isfinite(got.view(np.float32)).all() and np.any(got)


@pytest.mark.parametrize("name,opts", FIRST + SECOND, ids=[n for n, _ in FIRST + SECOND])
def test_specialised_tail_is_bit_identical_to_generic_tail(engine, monkeypatch, name, opts):
    path, got, ref, fo = _both(engine, monkeypatch, opts)
    _compare(name, path, got, ref, fo)
    assert path == "specialised"         # every plan here is within the bounds, the default one (bits_file_1) among them


@pytest.mark.parametrize("name,opts", BEYOND, ids=[n for n, _ in BEYOND])
def test_plan_beyond_the_bound_takes_the_generic_tail(engine, monkeypatch, name, opts):
    path, got, ref, fo = _both(engine, monkeypatch, opts)
    _compare(name, path, got, ref, fo)
    assert path == "generic"


def test_40_mel_bins_are_refused_under_both_settings(engine, monkeypatch):
    said = []
    engine.configure_mfcc()
    for generic in (False, True):
        monkeypatch.setenv("MFA_MFCC_GENERIC", "1") if generic else monkeypatch.delenv("MFA_MFCC_GENERIC", raising=False)
        with pytest.raises(MfaHipError) as err:
            engine.configure_mfcc(num_mel_bins=40)
        said.append(str(err.value))
    monkeypatch.delenv("MFA_MFCC_GENERIC")
    print(f"40 mel bins: {said[0]}")
    assert said[0] == said[1] and "num_mel_bins" in said[0]
    assert engine.mfcc_path() == "specialised"          # the refusal left the default options in force
