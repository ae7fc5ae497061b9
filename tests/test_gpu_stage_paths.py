"""The two drivers of the hot path's entry points — the engine's public stage methods (fresh outputs and uploaded offsets
per call) and ``Pipeline.step()`` (persistent tensors) — launch through the same helpers: on the same batch they run the same
kernels on the same data, so everything they produce is compared bit for bit, with no tolerance."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd.engine import Pipeline, offsets
from tests import helpers, synth

pytestmark = pytest.mark.gpu

SR = 16000
CUTS = [(0.0, 1.0, "this is the"), (4.0, 5.0, "there's nothing"), (23.5, 25.5, "um and that should be")]     # 1 s, 1 s, 2 s
U2S = np.array([4, 1, 4], dtype=np.int32)             # two speakers; the pipeline numbers them in ascending order
ROWS = np.array([1, 0, 1], dtype=np.int32)            # … which the stage methods are handed as dense rows


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("transforms", [False, True], ids=["deltas", "lda_fmllr"])
def test_stage_methods_and_pipeline_steps_agree_bit_for_bit(engine, fx, transforms):
    """``transforms``: splice + LDA [40, 91] and per-speaker fMLLR [2, 40, 41] (the other form of the feature launch), over a
    seeded 40-dimensional model with pdfs of 1 to 32 Gaussians on the fixture's transition model; without: Δ+ΔΔ and the
    fixture's own model."""
    dev = engine.device
    engine.configure_mfcc()
    tm = fx.mono_tm
    if transforms:
        rng = np.random.default_rng(77)
        engine.load_gmm(helpers.random_gmm(rng, 40, [int(g) for g in rng.choice([1, 4, 8, 16, 32], size=tm.num_pdfs)]))
        lda = torch.from_numpy(synth.seeded_lda()).to(dev)
        fmllr = torch.from_numpy(np.ascontiguousarray(synth.seeded_fmllr(2), dtype=np.float32)).to(dev)
        assert tuple(lda.shape) == (40, 91) and tuple(fmllr.shape) == (2, 40, 41)
        beams = dict(beam=1.0e4, retry_beam=0.0)
    else:
        engine.load_gmm(fx.mono_am)
        lda = fmllr = None
        beams = dict(beam=100.0, retry_beam=400.0)
    segs = [fx.pcm[int(a * SR): int(b * SR)] for a, b, _ in CUTS]
    so = offsets([len(s) for s in segs])
    pcm = torch.from_numpy(np.concatenate(segs)).to(dev)
    graphs = engine.pack_graphs([fx.mono_graph(t) for _a, _b, t in CUTS], tm)
    kw = dict(max_tokens=graphs.max_states, bp_tokens_per_frame=graphs.max_states, **beams)

    # the public stage methods
    mfcc, fo = engine.mfcc(pcm, so)
    assert list(np.diff(fo)) == [100, 100, 200]
    cmvn = engine.cmvn_stats(mfcc, fo, ROWS, 2)
    feats = engine.features(mfcc, fo, ROWS, cmvn, lda=lda, fmllr=fmllr)
    lazy = engine.align_features(graphs, feats, fo, **kw)
    ll, ll_off, ll_cols = engine.score(feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts,
                                       pdf_first_frame=graphs.pdf_first_frame)
    dense = engine.align(graphs, ll, ll_off, ll_cols, fo, **kw)
    torch.cuda.synchronize(dev)
    print("status: lazy", lazy["status"].tolist(), "dense", dense["status"].tolist())
    assert any(s in (0, 1) for s in lazy["status"].tolist())            # (alignments to compare, not three failures)

    for want, is_lazy in ((lazy, True), (dense, False)):
        pipe = Pipeline(engine, pcm, so, U2S, graphs, lda=lda, fmllr=fmllr, lazy=is_lazy, **kw)
        assert pipe.lazy == is_lazy
        pipe.step()
        torch.cuda.synchronize(dev)
        assert np.array_equal(pipe.frame_off, fo)
        assert torch.equal(pipe.mfcc, mfcc), is_lazy
        assert _bytes(pipe.cmvn) == _bytes(cmvn), is_lazy
        assert pipe.feats.shape == feats.shape and _bytes(pipe.feats) == _bytes(feats), is_lazy
        assert torch.equal(pipe.status, want["status"]) and torch.equal(pipe.n_words, want["n_words"]), is_lazy
        assert torch.equal(pipe.ali, want["ali"]), is_lazy
        assert _bytes(pipe.like) == _bytes(want["like"]), is_lazy
        for u, nw in enumerate(want["n_words"].tolist()):
            a = int(fo[u])
            assert torch.equal(pipe.words[a: a + nw], want["words"][a: a + nw]), (is_lazy, u)
        if not is_lazy:       # the score matrix too, where the kernel wrote it (the pipeline's scratch is not zero-filled)
            written = ll != 0
            assert torch.equal(pipe.loglikes[written], ll[written])
