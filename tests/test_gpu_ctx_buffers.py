"""The device memory a context owns, across calls: regrowth, model and option reloads, and teardown.

Every buffer of a context grows on demand and is reused by the next call (csrc/dev_buf.hpp), and the tables of a model or
an option set are replaced as a whole.  What a call computes must therefore not depend on what the engine has seen before:
  * regrowth — one engine runs a small batch, a big one and the small one again through every stage that keeps a buffer in
    the context; each output equals, element for element, what a fresh engine gives that has seen only that batch;
  * reload — scores and fMLLR statistics after ``load_gmm`` of another model (other pdf count, other row width) and back
    equal the first ones and those of a fresh engine, and an option set the library refuses changes nothing;
  * lifetime — engines created, used and closed in a row give the same result.
The engines here are the module's own: the order of calls on each of them is the test.

Shapes.  Small batch: 2 utterances of 0.55 s and 0.9 s (53 and 88 frames), one speaker, graphs of 40 and 150 states.  Big
batch: 5 utterances of 0.75–3 s (up to 298 frames: five 64-frame tiles, two scoring windows of 256), three speakers, graphs
of up to 1 100 states — more frames, score columns, arcs and states than the small one in every buffer.  The model has
pdfs of every slot class (1, 4, 8, 16, 17–32 and more than 32 Gaussians) over 39-dimensional Δ+ΔΔ features.

The general decoder's second tier — utterances whose 256-entries-per-frame token pool overflowed are decoded again with
the full pool, from a device list that grows with their number — is not reached by those shapes and has a case of its
own: graphs of 1 100 states under a beam of 50 keep most of their states alive, as in the fuzz test of
tests/test_gpu_general.py; one such utterance in the first call, three in the second.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd.engine import AlignmentEngine, fmllr_statistics
from tests import helpers
from tests.test_gpu_parity import _random_graph

pytestmark = pytest.mark.gpu

DIM = 39
KEYS = ("status", "ali", "words", "n_words", "like", "frame_like")
ALIGN = dict(beam=10.0, retry_beam=40.0, max_tokens=2048, bp_tokens_per_frame=1100, want_frame_likes=True)


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


class World:
    """The model and the two batches (seeded), shared by the tests of this module and never changed."""

    def __init__(self, fx):
        rng = np.random.default_rng(9100)
        self.tm = fx.mono_tm
        sizes = [int(x) for x in rng.choice([1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 26, 32, 40, 70], size=self.tm.num_pdfs)]
        assert {1, 4, 8, 16, 26, 70} <= set(sizes)
        self.am = helpers.random_gmm(rng, DIM, sizes)
        self.stats_am = helpers.fmllr_second_model(rng, self.am)
        self.batches = dict(small=self._batch(rng, [8800, 14400], [0, 0], [40, 150], [40, 40]),
                            big=self._batch(rng, [48000, 30000, 20000, 41000, 12000], [0, 1, 1, 2, 0], [400, 1100, 150, 400, 40],
                                            [150, 400, 40, 150, 40]))

    def _batch(self, rng, samples, utt2spk, states, general_states):
        return dict(pcm=[helpers.clipped_noise(rng, n) for n in samples], utt2spk=np.asarray(utt2spk, dtype=np.int32),
                    fsts=[_random_graph(rng, self.tm, s) for s in states],
                    eps_fsts=[helpers.with_eps(rng, _random_graph(rng, self.tm, s)) for s in general_states])


@pytest.fixture(scope="module")
def world(fx):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return World(fx)


def _engine(world):
    e = AlignmentEngine(0)
    e.configure_mfcc()
    e.configure_pitch()
    e.load_gmm(world.am)
    return e


def _run(e, world, name):
    """Every stage that keeps a buffer in the context, on one batch: {output name: numpy array}."""
    b = world.batches[name]
    so = _offsets([len(p) for p in b["pcm"]])
    pcm = _dev(e, np.concatenate(b["pcm"]))
    n_spk = int(b["utt2spk"].max()) + 1
    out = {}
    mfcc, fo = e.mfcc(pcm, so)
    stats = e.cmvn_stats(mfcc, fo, b["utt2spk"], n_spk)
    feats = e.features(mfcc, fo, b["utt2spk"], stats)
    out.update(mfcc=mfcc, cmvn=stats, feats=feats)
    graphs = e.pack_graphs(b["fsts"], world.tm)
    lazy = e.align_features(graphs, feats, fo, window=256, **ALIGN)
    out.update({f"lazy_{k}": lazy[k] for k in KEYS + ("loglikes",)})
    ll, ll_off, ll_cols = e.score(feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts)
    dense = e.align(graphs, ll, ll_off, ll_cols, fo, **ALIGN)
    out.update(dense_loglikes=ll, **{f"dense_{k}": dense[k] for k in KEYS})
    gen = e.align_general(e.pack_graphs_general(b["eps_fsts"], world.tm), feats, fo, want_frame_likes=True)
    out.update({f"general_{k}": gen[k] for k in KEYS})
    for form, stats_am in (("one", None), ("two", world.stats_am)):
        _, beta, K, G = fmllr_statistics(e, feats, fo, dense["ali"], world.tm, b["utt2spk"], [], stats_model=stats_am)
        out.update({f"fmllr_{form}_beta": beta, f"fmllr_{form}_K": K, f"fmllr_{form}_G": G})
    out["pitch"] = e.pitch(pcm, so)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def _assert_same(got, ref, what):
    """Bit for bit: same keys, shapes, types and bytes (stricter than ``array_equal``: a NaN must be the same NaN)."""
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), \
            f"{k} differs {what}"


@pytest.fixture(scope="module")
def fresh(world):
    """Per batch: the outputs of an engine that has seen nothing else."""
    ref = {}
    for name in world.batches:
        e = _engine(world)
        ref[name] = _run(e, world, name)
        e.close()
    return ref


def test_the_batches_reach_what_they_are_meant_to(fresh):
    small, big = fresh["small"], fresh["big"]
    print("statuses:", {k: (small[k].tolist(), big[k].tolist()) for k in ("lazy_status", "dense_status", "general_status")})
    assert big["mfcc"].shape[0] > 4 * small["mfcc"].shape[0] and big["dense_loglikes"].size > small["dense_loglikes"].size
    for r in (small, big):                          # arrays that never hold a NaN or an infinity
        for k in r:
            if k in ("mfcc", "cmvn", "feats", "dense_loglikes", "lazy_loglikes", "pitch") or k.startswith("fmllr_"):
                assert np.isfinite(r[k]).all(), k
    for path in ("lazy", "dense", "general"):       # the decoders did real work: some utterance of each batch was aligned
        for r in (small, big):
            assert np.isin(r[f"{path}_status"], (0, 1)).any()
    assert np.array_equal(big["lazy_ali"], big["dense_ali"])
    assert big["fmllr_one_beta"].sum() > 0 and not np.array_equal(big["fmllr_one_K"], big["fmllr_two_K"])


def test_regrowth_small_big_small(world, fresh):
    e = _engine(world)
    try:
        for step, name in enumerate(("small", "big", "small")):
            _assert_same(_run(e, world, name), fresh[name], f"at step {step} ({name}) from an engine that saw only that batch")
    finally:
        e.close()


def _scores(e, am, feats):
    """Dense scores of every pdf of the loaded model for one utterance."""
    pdfs, counts = e.sort_pdf_list(np.arange(am.num_pdfs, dtype=np.int32))
    fo = np.array([0, feats.shape[0]], np.int64)
    ll, _, _ = e.score(_dev(e, feats), fo, _dev(e, pdfs), np.array([0, am.num_pdfs], np.int64), _dev(e, counts[None, :]))
    torch.cuda.synchronize()
    return ll.cpu().numpy()


def _fmllr(e, case, stats_am):
    _, beta, K, G = fmllr_statistics(e, _dev(e, case["feats"]), case["fo"], _dev(e, case["ali"]), case["tm"], case["u2s"], [],
                                     stats_model=stats_am)
    return dict(beta=beta, K=K, G=G)


def _fmllr_as_left(e, case):
    """The accumulation alone, with whatever statistics model the context holds (``fmllr_statistics`` always names the form
    it wants first).  Two utterances, a speaker each."""
    dev = e.device
    feats, ali, fo = _dev(e, case["feats"]), _dev(e, case["ali"]), case["fo"]
    id2pdf = _dev(e, np.maximum(case["tm"].id2pdf, 0).astype(np.int32))
    w = np.ones(id2pdf.shape[0], np.float32)
    w[0] = 0.0
    pdf = torch.empty(ali.shape[0], dtype=torch.int32, device=dev)
    weight = torch.empty(ali.shape[0], dtype=torch.float32, device=dev)
    D = case["am"].dim
    beta = torch.zeros(2, dtype=torch.float64, device=dev)
    K = torch.zeros((2, D, D + 1), dtype=torch.float64, device=dev)
    G = torch.zeros((2, D, D + 1, D + 1), dtype=torch.float64, device=dev)
    # (every device array has a name here: the library reads them after this call returns, on the stream)
    d_fo, d_w = _dev(e, fo), _dev(e, w)
    d_spk_off, d_spk_utt = _dev(e, np.array([0, 1, 2], np.int32)), _dev(e, np.array([0, 1], np.int32))
    rc = e.lib.mfa_fmllr_acc_ali_batch(e.ctx, _ptr(feats), _ptr(d_fo), 2, int(fo[-1]), _ptr(ali), _ptr(id2pdf), _ptr(d_w),
                                       int(id2pdf.shape[0]), _ptr(pdf), _ptr(weight), _ptr(d_spk_off), _ptr(d_spk_utt), 2,
                                       _ptr(beta), _ptr(K), _ptr(G))
    assert rc == 0, e.lib.mfa_last_error(e.ctx)
    torch.cuda.synchronize()
    return dict(beta=beta.cpu().numpy(), K=K.cpu().numpy(), G=G.cpu().numpy())


@pytest.fixture(scope="module")
def two_models(world):
    """m1: the module's model (39 dimensions: rows of 80 floats).  m2: another pdf count, 41 dimensions (rows of 96 floats),
    other slot classes.  With frames and transition-ids for the fMLLR statistics of each (two utterances, two speakers)."""
    rng = np.random.default_rng(9200)
    m2 = helpers.random_gmm(rng, 41, [int(x) for x in rng.choice([1, 3, 8, 16, 30, 40], size=37)])
    cases = []
    for am in (world.am, m2):
        T = 150
        pdfs = rng.integers(0, am.num_pdfs, size=T)
        cases.append(dict(am=am, tm=helpers.fmllr_tm(am.num_pdfs), feats=helpers.fmllr_draw(rng, am, pdfs), fo=np.array([0, 70, T], np.int64),
                          ali=(2 * pdfs + 1).astype(np.int32), u2s=np.array([0, 1], np.int32)))
    return cases


def _fresh_model_results(case, stats_am):
    e = AlignmentEngine(0)
    e.load_gmm(case["am"])
    r = (_scores(e, case["am"], case["feats"]), _fmllr(e, case, None), _fmllr(e, case, stats_am) if stats_am is not None else None)
    e.close()
    return r


def test_reload_of_another_model_and_back(world, two_models):
    c1, c2 = two_models
    stats1 = world.stats_am
    ref_scores, ref_one, ref_two = _fresh_model_results(c1, stats1)
    ref2_scores, ref2_one, _ = _fresh_model_results(c2, None)
    assert not np.array_equal(ref_one["K"], ref_two["K"])
    e = AlignmentEngine(0)
    try:
        e.load_gmm(c1["am"])
        assert np.array_equal(_scores(e, c1["am"], c1["feats"]), ref_scores)
        _assert_same(_fmllr(e, c1, stats1), ref_two, "before the reload")    # leaves a statistics model and row counts behind
        e.load_gmm(c2["am"])
        assert np.array_equal(_scores(e, c2["am"], c2["feats"]), ref2_scores)
        _assert_same(_fmllr_as_left(e, c2), ref2_one, "with the second model (no statistics model of the first survives)")
        e.load_gmm(c1["am"])
        assert np.array_equal(_scores(e, c1["am"], c1["feats"]), ref_scores)
        _assert_same(_fmllr_as_left(e, c1), ref_one, "right after the reload (nothing stale: the single-model form)")
        _assert_same(_fmllr(e, c1, stats1), ref_two, "after the reload (two-model form)")
        with pytest.raises(_lib.MfaHipError):                                # another layout: refused …
            _fmllr(e, c1, c2["am"])
        _assert_same(_fmllr_as_left(e, c1), ref_two, "after a refused statistics model (the previous one stays in force)")
        _assert_same(_fmllr(e, c1, None), ref_one, "back in the single-model form")
    finally:
        e.close()


def test_refused_options_leave_the_previous_ones_in_force(world):
    b = world.batches["small"]
    so = _offsets([len(p) for p in b["pcm"]])
    e = AlignmentEngine(0)
    try:
        pcm = _dev(e, np.concatenate(b["pcm"]))
        e.configure_mfcc()
        before, fo = e.mfcc(pcm, so)
        with pytest.raises(_lib.MfaHipError):
            e.configure_mfcc(frame_length_ms=40.0)
        after, fo2 = e.mfcc(pcm, so)
        assert np.array_equal(fo, fo2) and np.array_equal(before.cpu().numpy(), after.cpu().numpy())
        e.configure_pitch()
        before = e.pitch(pcm, so).cpu().numpy()
        with pytest.raises(_lib.MfaHipError):
            e.configure_pitch(add_delta_pitch=1)
        after = e.pitch(pcm, so).cpu().numpy()
        assert np.isfinite(before).all() and np.array_equal(before, after)
    finally:
        e.close()


def _general_batches(world):
    """Two calls for the general decoder: the wide-beam utterances (1 100 states, 100 frames) overflow the first tier's pool,
    the others (40 states) cannot."""
    rng = np.random.default_rng(9300)
    calls = []
    for states in ([1100, 40, 40], [1100, 1100, 40, 1100, 40]):
        fsts = [helpers.with_eps(rng, _random_graph(rng, world.tm, s), frac=0.2) for s in states]
        feats = [rng.normal(0, 3.0, size=(100 if s > 40 else int(rng.integers(20, 60)), DIM)).astype(np.float32) for s in states]
        calls.append((fsts, feats))
    return calls


def _general(e, world, fsts, feats):
    fo = _offsets([x.shape[0] for x in feats])
    r = e.align_general(e.pack_graphs_general(fsts, world.tm), _dev(e, np.concatenate(feats)), fo, beam=50.0, retry_beam=0.0,
                        want_frame_likes=True)
    torch.cuda.synchronize()
    return {k: r[k].cpu().numpy() for k in KEYS}


def test_general_decoder_second_tier_with_a_growing_list(world):
    calls = _general_batches(world)
    ref = []
    for fsts, feats in calls:
        e = _engine(world)
        ref.append(_general(e, world, fsts, feats))
        e.close()
    print("general statuses:", [r["status"].tolist() for r in ref])
    for r in ref:       # the second tier finished what the first gave up: no pool overflow (4) is left, something aligned
        assert not np.isin(r["status"], (-1, 3, 4, 5, 6)).any() and (r["status"] == 0).any()
    e = _engine(world)
    try:
        for turn, (fsts, feats) in enumerate(calls):
            _assert_same(_general(e, world, fsts, feats), ref[turn], f"in call {turn} from an engine that made only that call")
    finally:
        e.close()


def test_three_engines_in_a_row(world, fresh):
    for turn in range(3):
        e = _engine(world)
        got = _run(e, world, "small")
        e.close()
        _assert_same(got, fresh["small"], f"on engine {turn} of three created and closed in a row")
