"""Per-speaker fMLLR on the Δ+ΔΔ feature path (mfa_feats_batch mode 0 with transforms): CMVN → deltas → transform in one
launch, the chain of MFA/db.py:2101-2136 for a model without LDA.

The kernel's claim is bit-identity: its output equals the oracle's affine chain (acc = 0, fmaf over ascending d, offset
last) applied to the kernel's own Δ output.  Against the oracle's whole chain the bar is 1e-4, the bar of the LDA+fMLLR
tests with the same generators (the float32 oracle chain is within 1.7e-5 of a float64 restatement at these shapes)."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from oracle import oracle as O
from tests import delta_fmllr_helpers as H

pytestmark = pytest.mark.gpu


def _device(engine, dim, cmvn, fmllr=None, utt2spk=True):
    mats, fo, u2s, _W, stats = H.kernel_case(dim)
    d = torch.from_numpy(np.concatenate(mats)).to(engine.device)
    cm = torch.from_numpy(stats.copy()).to(engine.device) if cmvn else None
    fm = None if fmllr is None else torch.from_numpy(np.array(fmllr)).to(engine.device)      # (a writable, contiguous copy)
    return engine.features(d, fo, u2s if utt2spk else None, cm, fmllr=fm).cpu().numpy()


@pytest.mark.parametrize("cmvn", [False, True], ids=["raw", "cmvn"])
@pytest.mark.parametrize("dim", H.DIMS)
def test_delta_fmllr_parity(engine, dim, cmvn):
    mats, fo, u2s, W, _stats = H.kernel_case(dim)
    plain = _device(engine, dim, cmvn)
    got = _device(engine, dim, cmvn, W)
    assert plain.shape == got.shape == (int(fo[-1]), 3 * dim)
    ref = H.oracle_chain(dim, cmvn)
    worst, equal, total, worst_plain = 0.0, 0, 0, 0.0
    identical = True
    for u, (d_ref, f_ref) in enumerate(ref):
        a, b = int(fo[u]), int(fo[u + 1])
        own = O.affine(plain[a:b], W[u2s[u]])            # the oracle's affine chain on the device's own Δ rows
        identical &= np.array_equal(got[a:b], own)
        equal += int((got[a:b] == f_ref).sum()); total += f_ref.size
        worst = max(worst, float(np.abs(got[a:b] - f_ref).max()))
        worst_plain = max(worst_plain, float(np.abs(plain[a:b] - d_ref).max()))
    print(f"dim {dim} cmvn {cmvn}: worst |device - oracle chain| {worst:.3e}, bit-equal share {equal / total:.4f}, "
          f"plain deltas worst {worst_plain:.3e}")
    assert worst_plain < 1e-4                             # without transforms: what the kernel computed before
    assert identical, "the transform is not the oracle's fmaf chain on the kernel's own Δ output"
    assert worst < 1e-4


@pytest.mark.parametrize("cmvn", [False, True], ids=["raw", "cmvn"])
def test_generic_switch_leaves_delta_fmllr_unchanged(engine, monkeypatch, cmvn):
    """Δ+fMLLR has one path, inside the generic kernel: MFA_FEATS_GENERIC=1, which takes the LDA shape off its register-row
    kernel, must not change it (a special-case kernel for 13 → 39 would be held to the generic path here)."""
    W = H.kernel_case(13)[3]
    default = _device(engine, 13, cmvn, W)
    monkeypatch.setenv("MFA_FEATS_GENERIC", "1")
    generic = _device(engine, 13, cmvn, W)
    assert np.array_equal(default, generic)
    assert not np.array_equal(default, _device(engine, 13, cmvn))     # and a transform was applied at all


@pytest.mark.parametrize("dim", [8, 13])
def test_one_transform_row_without_utt2spk(engine, dim):
    mats, fo, _u2s, W, _stats = H.kernel_case(dim)
    plain = _device(engine, dim, False, utt2spk=False)
    got = _device(engine, dim, False, W[1:2], utt2spk=False)          # one row: every utterance takes row 0 of what it is given
    assert np.array_equal(got, O.affine(plain, W[1]))
    for u, (d_ref, _f) in enumerate(H.oracle_chain(dim, False)):
        assert np.abs(O.affine(d_ref, W[1]) - got[int(fo[u]): int(fo[u + 1])]).max() < 1e-4


def _bad_transforms():
    W = H.kernel_case(13)[3]
    rng = np.random.default_rng(5)
    return {"lda_sized": rng.normal(size=(3, 40, 41)).astype(np.float32),
            "no_offset_column": np.ascontiguousarray(W[:, :, :39]),
            "too_few_rows": np.ascontiguousarray(W[:2]),
            "float64": W.astype(np.float64)}


@pytest.mark.parametrize("kind", ["lda_sized", "no_offset_column", "too_few_rows", "float64"])
def test_host_refuses_transforms_that_do_not_fit(engine, monkeypatch, kind):
    mats, fo, u2s, _W, _stats = H.kernel_case(13)
    bad = _bad_transforms()[kind]
    assert (kind == "too_few_rows") == (bad.shape[0] <= int(u2s.max()))
    counting = H.CountingLib(engine.lib)
    monkeypatch.setattr(engine, "lib", counting)
    with pytest.raises(MfaHipError):
        _device(engine, 13, True, bad)
    assert counting.feats_calls == 0                      # refused on the host: nothing was launched
    plain = _device(engine, 13, True)                     # and the engine goes on computing plain deltas
    assert counting.feats_calls == 1
    for u, (d_ref, _f) in enumerate(H.oracle_chain(13, True)):
        assert np.abs(plain[int(fo[u]): int(fo[u + 1])] - d_ref).max() < 1e-4


def test_non_contiguous_transforms_are_refused(engine):
    W = H.kernel_case(13)[3]
    mats, fo, u2s, _W, _stats = H.kernel_case(13)
    d = torch.from_numpy(np.concatenate(mats)).to(engine.device)
    wide = torch.from_numpy(np.concatenate([W, W], axis=2)).to(engine.device)
    with pytest.raises(MfaHipError):
        engine.features(d, fo, u2s, None, fmllr=wide[:, :, :40])


def test_pipeline_front_applies_delta_transforms(engine, fx):
    """Pipeline(lda=None, fmllr=W).front() fills ``feats`` with what engine.features gives on the same batch."""
    from montreal_forced_aligner_amd.engine import Pipeline

    engine.configure_mfcc()
    engine.load_gmm(fx.mono_am)
    sr = 16000
    cuts = [(0.0, 2.1, "this is the acoustic corpus"), (4.0, 6.5, "there's nothing going else going on"),
            (23.5, 26.72, "um and that should be all thanks")]
    segs = [fx.pcm[int(a * sr): int(b * sr)] for a, b, _ in cuts]
    sample_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    graphs = engine.pack_graphs([fx.mono_graph(t) for _a, _b, t in cuts], fx.mono_tm)
    u2s = np.array([7, 2, 7], dtype=np.int32)             # the pipeline renumbers speakers in ascending order: 2 → 0, 7 → 1
    W = torch.from_numpy(H.seeded_delta_fmllr(2)).to(engine.device)
    pcm = torch.from_numpy(np.concatenate(segs)).to(engine.device)
    pipe = Pipeline(engine, pcm, sample_off, u2s, graphs, lda=None, fmllr=W, beam=100.0, retry_beam=400.0)
    pipe.front()
    rows = np.array([1, 0, 1], dtype=np.int32)
    want = engine.features(pipe.mfcc, pipe.frame_off, rows, pipe.cmvn, fmllr=W)
    plain = engine.features(pipe.mfcc, pipe.frame_off, rows, pipe.cmvn)
    assert pipe.feats.shape == (int(pipe.frame_off[-1]), 39)
    assert torch.equal(pipe.feats, want)
    assert not torch.equal(pipe.feats, plain)
    with pytest.raises(MfaHipError):                      # one row for two speakers
        Pipeline(engine, pcm, sample_off, u2s, graphs, lda=None, fmllr=W[:1].contiguous(), beam=100.0, retry_beam=400.0)
