"""The sweep's fourth consumer on the device: the neighbour bit matrix against the host twin bit for bit on operands where every
sum is exact (all three metrics; point counts around the tile and word sizes; rectangular shapes), against the matrix the
same call stored on random data, under forced column passes, with NaN rows and columns, at the infinite thresholds; the
padding bits; determinism; the refusals; and the k-nearest consumer for the two new metrics."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError, _ptr, check
from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.stats import knn, knn_host, metric_sweep, metric_sweep_host, neighbor_bits, plda_scores
from tests import dbscan_ref as G
from tests import plda_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)
DIMS = (1, 3, 4, 5, 40)
PASS_COLS = ("64", "128")


def words(t) -> np.ndarray:
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint64)


def shapes():
    """(rows, columns): every size square, and against 130 on either side."""
    return sorted({(a, a) for a in SIZES} | {(a, 130) for a in SIZES} | {(130, a) for a in SIZES})


def integer_vectors(D, nt, ns, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (nt, D)).astype(np.float64), rng.integers(-3, 4, (ns, D)).astype(np.float64)


@pytest.mark.parametrize("D", DIMS)
def test_bits_equal_the_twin_on_exact_operands(engine, D):
    """plda: the debug entry on dyadic operands (tests/plda_ref.py exact_case); euclidean and dot: integer vectors, on which the
    prepare step and every sum of the sweep are exact.  The threshold is the median score, so ties with it are common."""
    for nt, ns in shapes():
        test, A, B, c = R.exact_case(D, nt, ns, seed=D * 977 + nt * 5 + ns)
        want = np.asarray(R.exact_scores(test, A, B, c), dtype=np.float64)
        thr = float(np.median(want))
        hs, _, _, hb = metric_sweep_host(None, test, None, thr, want_scores=True, operands=(A, B, c))
        assert np.array_equal(hs, want) and np.array_equal(G.unpack(hb, ns), want >= thr) and not G.padding_bits(hb, ns).any()
        ds, _, _, db = metric_sweep(engine, None, test, None, thr, want_scores=True, operands=(A, B, c))
        assert np.array_equal(words(db), hb), ("plda", D, nt, ns)
        assert np.array_equal(ds.cpu().numpy(), want)
        x, y = integer_vectors(D, nt, ns, seed=D * 31 + nt + 3 * ns)
        for metric, exact in (("euclidean", -((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)), ("dot", x @ y.T)):
            thr = float(np.median(exact))
            hs, _, _, hb = metric_sweep_host(metric, x, y, thr, want_scores=True)
            assert np.array_equal(hs, exact) and np.array_equal(G.unpack(hb, ns), exact >= thr)
            db = metric_sweep(engine, metric, x, y, thr)[3]
            assert np.array_equal(words(db), hb), (metric, D, nt, ns)


@pytest.mark.parametrize("metric", ["plda", "euclidean", "cosine"])
def test_bits_are_the_threshold_on_the_matrix_the_same_call_stored(engine, monkeypatch, metric):
    """Random data: no exactness, but the bits are a plain comparison on the very values output (a) stores — whatever the passes."""
    for D, nt, ns, seed in ((5, 70, 130, 1), (40, 129, 200, 2), (16, 200, 63, 3)):
        psi, train, n, test = R.random_case(D, nt, ns, seed=seed)
        model = P.PldaModel(np.zeros(D), np.eye(D), psi)
        first = None
        for cols in (None,) + PASS_COLS:
            if cols is None:
                monkeypatch.delenv("MFA_PLDA_PASS_COLS", raising=False)
            else:
                monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
            probe = metric_sweep(engine, metric, test, train, None, model, n, want_scores=True, want_bits=False)[0].cpu().numpy()
            thr = float(np.median(probe))
            scores, _, _, db = metric_sweep(engine, metric, test, train, thr, model, n, want_scores=True)
            scores = scores.cpu().numpy()
            assert np.array_equal(G.unpack(words(db), ns), scores >= thr), (metric, D, nt, ns, cols)
            assert not G.padding_bits(words(db), ns).any()
            assert 0 < (scores >= thr).sum() < scores.size
            alone = metric_sweep(engine, metric, test, train, thr, model, n)[3]           # the bits as the only output
            assert np.array_equal(words(alone), words(db))
            if first is None:
                first = (words(db).copy(), scores.copy())
            else:                                          # the words do not depend on the passes
                assert np.array_equal(words(db), first[0]) and np.array_equal(scores.view(np.uint64), first[1].view(np.uint64))
        if metric == "plda":                               # the old entry point stores the same matrix
            monkeypatch.delenv("MFA_PLDA_PASS_COLS", raising=False)
            assert np.array_equal(plda_scores(engine, model, test, train, n).view(np.uint64), first[1].view(np.uint64))
    monkeypatch.delenv("MFA_PLDA_PASS_COLS", raising=False)


def test_forced_passes_give_the_same_words_on_exact_operands(engine, monkeypatch):
    test, A, B, c = R.exact_case(5, 129, 200, seed=4)
    want = np.asarray(R.exact_scores(test, A, B, c), dtype=np.float64)
    thr = float(np.median(want))
    for cols in PASS_COLS:
        monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
        _, _, dk, db = metric_sweep(engine, None, test, None, thr, k=5, want_knn=True, operands=(A, B, c))
        assert np.array_equal(G.unpack(words(db), 200), want >= thr), cols
        ref_i, ref_s = R.stable_topk(want, 5)
        assert np.array_equal(dk[0].cpu().numpy(), ref_i) and np.array_equal(dk[1].cpu().numpy(), ref_s)
    monkeypatch.delenv("MFA_PLDA_PASS_COLS")


@pytest.mark.parametrize("metric", ["plda", "euclidean", "dot"])
def test_nan_sets_no_bit_and_the_infinite_thresholds(engine, metric):
    rng = np.random.default_rng(8)
    D, nt, ns = 6, 70, 131
    x, y = rng.standard_normal((nt, D)), rng.standard_normal((ns, D))
    x[3, 2] = np.nan
    y[65, 0] = np.nan
    model = P.PldaModel(np.zeros(D), np.eye(D), rng.uniform(0.5, 2.0, D))
    clean = np.ones((nt, ns), dtype=bool)
    clean[3, :] = False
    clean[:, 65] = False
    for thr in (-np.inf, 0.0):
        scores, _, _, db = metric_sweep(engine, metric, x, y, thr, model, want_scores=True)
        got, scores = G.unpack(words(db), ns), scores.cpu().numpy()
        assert not got[3].any() and not got[:, 65].any() and not G.padding_bits(words(db), ns).any()
        assert np.isnan(scores[3]).all() and np.isnan(scores[:, 65]).all()
        if thr == -np.inf:
            assert np.array_equal(got, clean)              # every score that is a number
    none = metric_sweep(engine, metric, x, y, np.inf, model)[3]
    assert not words(none).any()
    y[7] = 1e200                                           # an infinite score is a score: -inf only passes threshold -inf
    if metric == "euclidean":
        got = G.unpack(words(metric_sweep(engine, metric, x, y, -np.inf, model)[3]), ns)
        assert got[:, 7].sum() == nt - 1 and not got[3, 7]


def test_two_runs_give_identical_words(engine):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((200, 40))
    a = words(neighbor_bits(engine, "cosine", x, x, 0.9)).copy()
    b = words(neighbor_bits(engine, "cosine", x, x, 0.9))
    assert np.array_equal(a, b) and a.any()
    with pytest.raises(MfaHipError, match="bytes"):
        neighbor_bits(engine, "cosine", x, x, 0.9, max_bytes=1000)


def test_refusals_leave_the_context_usable(engine):
    dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=engine.device)
    x, y = integer_vectors(4, 3, 5, seed=1)
    d_x, d_y, d_psi = dev(x), dev(y), dev(np.ones(4))
    bits = torch.zeros((3, 1), dtype=torch.int64, device=engine.device)
    call = lambda **kw: engine._launch_neighbor_bits(**{**dict(test=d_x, train=d_y, metric=1, train_n=None, psi=None, exclude_diagonal=False, k=1,
                                                               threshold=0.0, scores=None, best=None, knn=None, bits=bits), **kw})
    call()
    good = bits.cpu().numpy().copy()
    for metric in (-1, 3):
        with pytest.raises(MfaHipError, match="metric"):
            call(metric=metric)
    with pytest.raises(MfaHipError, match="not a number"):
        call(threshold=float("nan"))
    with pytest.raises(MfaHipError, match="every output"):
        call(bits=None)
    with pytest.raises(MfaHipError, match="NULL model"):
        call(metric=0)
    with pytest.raises(MfaHipError, match="NULL model"):                   # train vectors counted but not given
        check(engine.ctx, engine.lib.mfa_neighbor_bits_batch(engine.ctx, _ptr(d_x), 3, None, 5, 4, 1, None, None, 0, 1, 0.0, None, None, None,
                                                             None, None, _ptr(bits)), "mfa_neighbor_bits_batch")
    with pytest.raises(MfaHipError, match="come together"):                # an index output without its scores
        check(engine.ctx, engine.lib.mfa_neighbor_bits_batch(engine.ctx, _ptr(d_x), 3, _ptr(d_y), 5, 4, 1, None, None, 0, 1, 0.0, None,
                                                             _ptr(torch.empty(3, dtype=torch.int32, device=engine.device)), None, None, None,
                                                             _ptr(bits)), "mfa_neighbor_bits_batch")
    with pytest.raises(MfaHipError, match="dimension"):
        call(test=d_x[:, :0].contiguous(), train=d_y[:, :0].contiguous())
    wide = torch.zeros((1, 1025), dtype=torch.float64, device=engine.device)
    with pytest.raises(MfaHipError, match="dimension"):
        call(test=wide, train=wide)
    knn_out = lambda k: (torch.empty((3, max(k, 1)), dtype=torch.int32, device=engine.device),
                         torch.empty((3, max(k, 1)), dtype=torch.float64, device=engine.device))
    for k in (0, 65):
        with pytest.raises(MfaHipError, match="lists of"):
            call(k=k, knn=knn_out(k))
    with pytest.raises(MfaHipError, match="psi"):
        call(metric=0, psi=dev(np.array([1.0, 0.0, 1.0, 1.0])))
    with pytest.raises(MfaHipError, match="NULL operands"):
        engine._launch_neighbor_bits(d_x, None, 0, None, None, False, 1, 0.0, None, None, None, bits, operands=(None, d_y, dev(np.zeros(5))))
    call()
    assert np.array_equal(bits.cpu().numpy(), good)
    # no test vectors: nothing is written; no train vectors: no words
    untouched = torch.full((3, 1), 5, dtype=torch.int64, device=engine.device)
    call(test=d_x[:0], bits=untouched)
    assert (untouched.cpu().numpy() == 5).all()
    assert metric_sweep(engine, "euclidean", x, y[:0], 0.0)[3].shape == (3, 0)


@pytest.mark.parametrize("metric", ["euclidean", "dot", "cosine"])
def test_knn_for_the_new_metrics_equals_the_twin(engine, metric):
    for D, n, k, seed in ((3, 65, 1, 1), (5, 129, 7, 2), (40, 200, 64, 3)):
        x, _ = integer_vectors(D, n, 1, seed)
        x[n // 2] = x[0]                                   # duplicates: ties go to the lower index
        if metric == "cosine":
            x[(x == 0).all(axis=1)] = 1.0                  # a zero row has no direction
        for excl in (False, True):
            hi, hs = knn_host(metric, x, x, k, exclude_diagonal=excl)
            di, ds = knn(engine, metric, x, x, k, exclude_diagonal=excl)
            di, ds = di.cpu().numpy(), ds.cpu().numpy()
            if metric == "cosine":
                # unit rows are not exact, and torch and numpy may round them differently: a score is a sum of D products of
                # numbers up to 1, each side within (D + 5) roundings of 2^-53 of it — below 1e-14 at D = 40; indices may swap
                # where two scores tie that closely, the scores may not move further
                np.testing.assert_allclose(ds, hs, rtol=0, atol=2e-14)
            else:
                assert np.array_equal(di, hi) and np.array_equal(ds.view(np.uint64), hs.view(np.uint64)), (metric, D, n, k, excl)
                ref_i, ref_s = R.stable_topk(-((x[:, None] - x[None]) ** 2).sum(axis=2) if metric == "euclidean" else x @ x.T, k, excl)
                assert np.array_equal(di, ref_i) and np.array_equal(ds, ref_s)
