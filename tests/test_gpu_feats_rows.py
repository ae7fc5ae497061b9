"""GPU test of the frame-per-lane splice + LDA + fMLLR kernel (feats.hip: feats_rows_kernel, MFA's standard shape 13 × ±3 →
91 → 40) against the generic feats_kernel in the same process: mfa_feats_batch reads MFA_FEATS_GENERIC at every call, and
the two must agree bit for bit — the packed FMAs of the new kernel are two IEEE fused multiply-adds each, in the generic
kernel's order.  One ragged batch holds every utterance length at which the geometry changes: shorter than the halo (1–4),
around a wavefront's 64 frames, around two and three of them, around the 256-frame tile, and a second tile that fills one
wavefront and part of the next (321)."""
import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

DIM, CTX, ROWS = 13, 3, 40
T_LIST = [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 321]
SPK = np.array([u % 2 for u in range(len(T_LIST))], np.int32)      # two speakers: CMVN statistics and fMLLR matrices of their own


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("scale", [1.0, 1e-40], ids=["normal", "denormal_inputs"])
@pytest.mark.parametrize("fmllr", [False, True], ids=["lda", "lda_fmllr"])
@pytest.mark.parametrize("offset", [0, 1], ids=["91_columns", "offset_column"])
def test_frame_lane_kernel_is_bit_identical_to_generic_kernel(engine, monkeypatch, offset, fmllr, scale):
    rng = np.random.default_rng(4100 + 4 * offset + 2 * fmllr + (scale != 1.0))
    fo = np.concatenate([[0], np.cumsum(T_LIST)]).astype(np.int64)
    # each speaker has a mean of its own, so a wrong speaker's CMVN row shows
    mf = (rng.standard_normal((fo[-1], DIM)) * 3.0 + np.repeat(SPK, T_LIST)[:, None] * 5.0).astype(np.float32)
    mf = (mf * np.float32(scale)).astype(np.float32)
    if scale != 1.0:
        assert 0 < np.abs(mf).max() < np.finfo(np.float32).tiny          # every input is a denormal
    lda = helpers.random_affine(rng, ROWS, (2 * CTX + 1) * DIM + offset)
    fm = np.stack([helpers.random_affine(rng, ROWS, ROWS + 1) for _ in range(2)])
    assert not np.array_equal(fm[0], fm[1])
    d_mf = _dev(engine, mf)
    stats = engine.cmvn_stats(d_mf, fo, SPK, 2)
    args = dict(lda=_dev(engine, lda), fmllr=_dev(engine, fm) if fmllr else None)
    monkeypatch.delenv("MFA_FEATS_GENERIC", raising=False)
    fast = _bits(engine.features(d_mf, fo, SPK, stats, **args))
    monkeypatch.setenv("MFA_FEATS_GENERIC", "1")
    generic = _bits(engine.features(d_mf, fo, SPK, stats, **args))
    monkeypatch.delenv("MFA_FEATS_GENERIC")
    assert fast.shape == generic.shape == (fo[-1], ROWS)
    differ = np.flatnonzero((fast != generic).any(axis=1))
    print(f"offset {offset} fmllr {fmllr} scale {scale}: {len(differ)} of {fo[-1]} frames differ"
          + (f", first at frame {differ[0]} (utterance {np.searchsorted(fo, differ[0], 'right') - 1})" if len(differ) else ""))
    assert np.array_equal(fast, generic)
    assert np.isfinite(fast.view(np.float32)).all() and np.any(fast)


def test_frame_lane_kernel_without_cmvn(engine, monkeypatch):
    """No CMVN statistics: the inputs go through untouched (a −0.0 stays −0.0, so nothing is added to them)."""
    rng = np.random.default_rng(4200)
    fo = np.concatenate([[0], np.cumsum(T_LIST)]).astype(np.int64)
    mf = rng.standard_normal((fo[-1], DIM)).astype(np.float32)
    mf[::7] = -0.0
    lda = helpers.random_affine(rng, ROWS, (2 * CTX + 1) * DIM + 1)
    d_mf, d_lda = _dev(engine, mf), _dev(engine, lda)
    monkeypatch.delenv("MFA_FEATS_GENERIC", raising=False)
    fast = _bits(engine.features(d_mf, fo, lda=d_lda))
    monkeypatch.setenv("MFA_FEATS_GENERIC", "1")
    generic = _bits(engine.features(d_mf, fo, lda=d_lda))
    monkeypatch.delenv("MFA_FEATS_GENERIC")
    assert np.array_equal(fast, generic)
