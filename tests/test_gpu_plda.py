"""The PLDA stage on the device (csrc/plda.hip) against its host twins and the longdouble restatement (tests/plda_ref.py):
the sweep on operands where every sum is exact, the scores under the bound derived in plda_ref's docstring, the fused
selections against the matrix the same call wrote, the column passes, NaN isolation, repeatability, the refusals, the
transform.

Shapes: D ∈ {1, 3, 4, 5, 16, 17, 192} (below, at and past the matrix instruction's K = 4 and its padding, past one block of 16,
the production dimension); rows and columns ∈ {1, 15, 16, 17, 63, 64, 65, 130} (around the instruction's 16, the workgroup's
64 rows and the step's 64 columns, more than one block of each); k ∈ {1, 5, 64}, more than the columns included; column
passes of 64, 128 and 192 columns: 3, 2 and 1 passes at 130 columns.
"""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd._lib import MfaHipError, _ptr, check
from montreal_forced_aligner_amd.stats import (plda_classify, plda_knn, plda_scores, plda_scores_host, plda_sweep, plda_sweep_host,
                                               plda_transform, plda_transform_host, _plda_score_call)
from tests import plda_ref as R

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 5, 16, 17, 192)
SIZES = (1, 15, 16, 17, 63, 64, 65, 130)
KS = (1, 5, 64)
PASS_COLS = ("192", "128", "64")          # 1, 2 and 3 passes at 130 columns


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32).tolist()


def host(t):
    return None if t is None else tuple(x.cpu().numpy() for x in t) if isinstance(t, tuple) else t.cpu().numpy()


def flat(outs):
    """The arrays of a scoring call's (scores, (best index, score), (k-NN indices, scores)) as one list of bit patterns."""
    s, b, q = (host(t) for t in outs)
    return [bits(a) for a in (s, *b, *q)]


def model_of(psi):
    D = psi.shape[0]
    return P.PldaModel(np.zeros(D), np.eye(D), psi)


def pairs(D):
    """(rows, columns) pairs: every size on each side against 130 and against itself."""
    return sorted({(a, 130) for a in SIZES} | {(130, a) for a in SIZES} | {(a, a) for a in SIZES})


# ---- exact tier ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_sweep_is_exact_on_dyadic_operands(engine, monkeypatch, D):
    """Every product and sum exact: the device equals the twin and the restatement bit for bit, indices and ties included,
    for every k and every pass split."""
    for nt, ns in pairs(D):
        test, A, B, c = R.exact_case(D, nt, ns, seed=D * 1000 + nt * 7 + ns)
        want = np.asarray(R.exact_scores(test, A, B, c), dtype=np.float64)
        for k in KS:
            for excl in ((False, True) if nt == ns else (False,)):
                ref_i, ref_s = R.stable_topk(want, k, excl)
                hs, hb, hk = plda_sweep_host(test, A, B, c, excl, k)
                assert bits(hs) == bits(want) and bits(hk[0]) == bits(ref_i) and bits(hk[1]) == bits(ref_s)
                assert bits(hb[0]) == bits(ref_i[:, 0]) and bits(hb[1]) == bits(ref_s[:, 0])
                for cols in (PASS_COLS if k != 5 else PASS_COLS[:1]):
                    monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
                    ds, db, dk = (host(t) for t in plda_sweep(engine, test, A, B, c, excl, k))
                    where = (D, nt, ns, k, excl, cols)
                    assert bits(ds) == bits(want), where
                    assert bits(dk[0]) == bits(ref_i) and bits(dk[1]) == bits(ref_s), where
                    assert bits(db[0]) == bits(ref_i[:, 0]) and bits(db[1]) == bits(ref_s[:, 0]), where
    monkeypatch.delenv("MFA_PLDA_PASS_COLS")
    test, A, B, c = R.exact_case(D, 65, 130, seed=D)                       # the automatic split
    ds, db, dk = (host(t) for t in plda_sweep(engine, test, A, B, c, False, 5))
    want = np.asarray(R.exact_scores(test, A, B, c), dtype=np.float64)
    assert bits(ds) == bits(want) and bits(dk[0]) == bits(R.stable_topk(want, 5)[0])


# ---- bounded tier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_scores_within_the_derived_bound(engine, monkeypatch, D):
    """|device − restatement| ≤ γ_m·(|c_j| + Σ|p²A| + Σ|pB|), m = 6 D + 92 (tests/plda_ref.py); the twin under the same bound;
    and the selections: exactly those of the matrix the same call wrote, and the restatement's wherever its gap is clear."""
    left_out = total = 0
    for nt, ns in pairs(D):
        psi, train, n, test = R.random_case(D, nt, ns, seed=D * 100 + nt + 3 * ns)
        R.check_case(psi, train, n, test)
        model, ref, bound = model_of(psi), R.llr(psi, train, n, test), R.error_bound(psi, train, n, test)
        ref64 = np.asarray(ref, dtype=np.float64)
        err_h = np.abs(np.asarray(R.LD(plda_scores_host(model, test, train, n)) - ref, dtype=np.float64))
        for k in KS:
            excl = nt == ns and k == 5
            for cols in PASS_COLS:
                monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
                s, b, q = (host(t) for t in _plda_score_call(engine, model, test, train, n, excl, k, True, True, True))
                err = np.abs(np.asarray(R.LD(s) - ref, dtype=np.float64))
                print(f"D={D} {nt}x{ns} k={k} cols={cols}: max err/bound device {np.max(err / bound):.3g} twin {np.max(err_h / bound):.3g}")
                assert (err <= bound).all() and (err_h <= bound).all(), (D, nt, ns, k, cols)
                own_i, own_s = R.stable_topk(s, k, excl)                 # self-consistency: exact
                assert bits(q[0]) == bits(own_i) and bits(q[1]) == bits(own_s), (D, nt, ns, k, cols)
                assert bits(b[0]) == bits(own_i[:, 0]) and bits(b[1]) == bits(own_s[:, 0]), (D, nt, ns, k, cols)
            # against the restatement: only rows whose ranks are clear of one another by twice the bound
            clear, order, kk = R.clear_rows(ref64, bound, k, excl)
            total += nt
            left_out += int((~clear).sum())
            assert (q[0][clear, :kk] == order[clear, :kk]).all(), (D, nt, ns, k)
    monkeypatch.delenv("MFA_PLDA_PASS_COLS")
    assert left_out <= 0.05 * total, (left_out, total)


def test_public_calls_agree_with_one_another(engine):
    psi, train, n, test = R.random_case(17, 65, 130, seed=5)
    model = model_of(psi)
    full = plda_scores(engine, model, test, train, n)
    blocks = plda_scores(engine, model, test, train, n, block_bytes=130 * 8 * 7)        # 7 rows a block
    assert bits(full) == bits(blocks)
    bi, bs = host(plda_classify(engine, model, test, train, n))
    ki, ks = host(plda_knn(engine, model, test, train, 5, n))
    own_i, own_s = R.stable_topk(full, 5)
    assert bits(ki) == bits(own_i) and bits(ks) == bits(own_s) and bits(bi) == bits(own_i[:, 0]) and bits(bs) == bits(own_s[:, 0])
    with pytest.raises(MfaHipError, match="plda_knn or plda_classify"):
        plda_scores(engine, model, test, train, n, max_bytes=65 * 130 * 8 - 1)


def test_a_nan_stays_in_its_row_or_column(engine):
    psi, train, n, test = R.random_case(5, 65, 130, seed=9)
    model = model_of(psi)
    clean = _plda_score_call(engine, model, test, train, n, False, 5, True, True, True)
    cs, cb, ck = (host(t) for t in clean)
    t2, r2 = test.copy(), train.copy()
    t2[17, 2] = np.nan
    t2[40, 0] = np.inf
    r2[66, 4] = np.nan
    s, b, q = (host(t) for t in _plda_score_call(engine, model, t2, r2, n, False, 5, True, True, True))
    bad = np.zeros_like(cs, dtype=bool)
    bad[17, :] = bad[40, :] = bad[:, 66] = True
    assert bits(s[~bad]) == bits(cs[~bad])
    assert np.isnan(s[17]).all() and not np.isfinite(s[40]).any() and np.isnan(s[:, 66]).all()
    assert (b[0][[17, 40]] == -1).all() and np.isneginf(b[1][[17, 40]]).all() and (q[0][[17, 40]] == -1).all()
    assert (q[0] != 66).all()                                                # a NaN is never selected
    own_i, own_s = R.stable_topk(s, 5)
    assert bits(q[0]) == bits(own_i) and bits(q[1]) == bits(own_s) and bits(b[0]) == bits(own_i[:, 0])


def test_two_runs_give_identical_bits(engine):
    psi, train, n, test = R.random_case(192, 130, 130, seed=2)
    model = model_of(psi)
    run = lambda: flat(_plda_score_call(engine, model, test, train, n, True, 64, True, True, True))
    assert run() == run()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((130, 192))
    tm = P.PldaModel(x[0], rng.standard_normal((192, 192)) * 0.1, psi)
    assert bits(host(plda_transform(engine, tm, x))) == bits(host(plda_transform(engine, tm, x)))


def test_refusals_leave_the_context_usable(engine):
    psi, train, n, test = R.random_case(4, 3, 5, seed=1)
    model = model_of(psi)
    ok = lambda: plda_classify(engine, model, test, train, n)
    ok()
    dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=engine.device)
    d_test, d_train, d_psi = dev(test), dev(train), dev(psi)
    best = (torch.empty(3, dtype=torch.int32, device=engine.device), torch.empty(3, dtype=torch.float64, device=engine.device))
    knn = lambda k: (torch.empty((3, max(k, 1)), dtype=torch.int32, device=engine.device),
                     torch.empty((3, max(k, 1)), dtype=torch.float64, device=engine.device))
    with pytest.raises(MfaHipError, match="every output"):
        engine._launch_plda_score(d_test, d_train, None, d_psi, False, 1, None, None, None)
    for k in (0, 65, -1):
        with pytest.raises(MfaHipError, match="lists of"):
            engine._launch_plda_score(d_test, d_train, None, d_psi, False, k, None, None, knn(k))
    wide = torch.zeros((1, 1025), dtype=torch.float64, device=engine.device)
    with pytest.raises(MfaHipError, match="dimension"):
        engine._launch_plda_score(wide, wide, None, torch.ones(1025, dtype=torch.float64, device=engine.device), False, 1, None, best, None)
    with pytest.raises(MfaHipError, match="dimension"):
        engine._launch_plda_score(d_test[:, :0], d_train[:, :0], None, d_psi[:0], False, 1, None, best, None)
    for bad in (0.0, -1.0, np.inf, np.nan):
        p2 = psi.copy()
        p2[2] = bad
        with pytest.raises(MfaHipError, match="psi"):
            engine._launch_plda_score(d_test, d_train, None, dev(p2), False, 1, None, best, None)
    for bad in (0, -3):
        n2 = n.copy()
        n2[4] = bad
        with pytest.raises(MfaHipError, match="examples below 1"):
            engine._launch_plda_score(d_test, d_train, dev(n2, torch.int32), d_psi, False, 1, None, best, None)
    with pytest.raises(MfaHipError, match="come together"):                  # an index output without its scores
        check(engine.ctx, engine.lib.mfa_plda_score_batch(engine.ctx, _ptr(d_test), 3, _ptr(d_train), 5, 4, None, _ptr(d_psi), 0, 1, None,
                                                          _ptr(best[0]), None, None, None), "mfa_plda_score_batch")
    with pytest.raises(MfaHipError, match="normalisation"):
        engine._launch_plda_transform(d_test, (torch.eye(4, dtype=torch.float64, device=engine.device), d_psi, d_psi), None, 3,
                                      torch.empty_like(d_test))
    with pytest.raises(MfaHipError, match="may not be the input"):
        engine._launch_plda_transform(d_test, (torch.eye(4, dtype=torch.float64, device=engine.device), d_psi, d_psi), None, 1, d_test)
    b = host(ok())
    assert bits(b[0]) == bits(R.stable_topk(plda_scores(engine, model, test, train, n), 1)[0][:, 0])
    # no train vectors: empty lists, no fault
    e = host(plda_knn(engine, model, test, train[:0], 3, n[:0]))
    assert (e[0] == -1).all() and np.isneginf(e[1]).all()
    assert plda_scores(engine, model, test[:0], train, n).shape == (0, 5)


# ---- the transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_transform_product_is_exact_on_integer_data(engine, D):
    rng = np.random.default_rng(D)
    for N in (1, 17, 64, 130):
        x = rng.integers(-4, 5, (N, D)).astype(np.float64)
        model = P.PldaModel(rng.integers(-3, 4, D).astype(np.float64), rng.integers(-2, 3, (D, D)).astype(np.float64), np.ones(D))
        want = x @ model.transform.T + model.offset
        got = host(plda_transform(engine, model, x, normalize_length=False))
        # equal as numbers: a zero's sign is not compared (the device's zero-padded steps of k add +0 to a −0 offset)
        assert np.array_equal(got, want) and np.array_equal(plda_transform_host(model, x, normalize_length=False), want), (D, N)


@pytest.mark.parametrize("D", DIMS)
def test_transform_factors_within_the_derived_bound(engine, D):
    """All bounds from the inputs, in longdouble, with γ_m of tests/plda_ref.py.
    u_j = offset_j + Σ_k x_k T_jk, D products and D additions: |Δu_j| ≤ γ_(D+2)·(|offset_j| + Σ_k |x_k T_jk|) =: e_j, plus what
    the model's float64 offset differs from −T·mean formed in longdouble (an input's rounding, not the code's).
    S = Σ_k u_k²/d_k, d_k = ψ_k + 1/n (or 1): from Δu, |Δ(u_k²)| ≤ 2|u_k| e_k + e_k²; a term's own roundings are 4 (1/n, the sum
    d_k, the square, the quotient) and the sum's at most D − 1 in a lane plus 6 butterfly levels: ΔS ≤ Σ_k (2|u_k| e_k + e_k²)/d_k +
    γ_(D+11)·S.  f = sqrt(D/S): with ρ = ΔS/S, |Δf|/f ≤ ρ/2·(1 + ρ) + γ_2 (the quotient and the root).  The output u_k·f takes one
    more rounding: |Δ(u_k f)| ≤ |u_k| f (|Δf|/f + γ_1)(1 + |Δf|/f) + e_k f (1 + |Δf|/f)."""
    rng = np.random.default_rng(100 + D)
    N = 130
    x = rng.standard_normal((N, D))
    psi = np.sort(rng.uniform(0.05, 8.0, D))[::-1].copy()
    model = P.PldaModel(rng.standard_normal(D), rng.standard_normal((D, D)) / np.sqrt(D), psi)
    n = np.where(np.arange(N) % 2 == 0, 1, 9).astype(np.int32)
    LD, g = R.LD, R.gamma
    T, off = LD(model.transform), LD(model.offset)
    for norm, kw in ((0, dict(normalize_length=False)), (1, dict(simple_length_norm=True)), (2, dict())):
        ref = R.transform(model.mean, model.transform, psi, x, n, norm)
        u = R.transform(model.mean, model.transform, psi, x, n, 0)
        e = g(D + 2) * (np.abs(off)[None, :] + np.abs(LD(x)) @ np.abs(T).T) + np.abs(off - LD(model.offset))
        if norm == 0:
            bound = e
        else:
            d = (LD(psi)[None, :] + 1 / LD(n)[:, None]) if norm == 2 else LD(np.ones((N, D)))
            S = (u * u / d).sum(axis=1, keepdims=True)
            dS = ((2 * np.abs(u) * e + e * e) / d).sum(axis=1, keepdims=True) + g(D + 11) * S
            f = np.sqrt(D / S)
            rel_f = dS / S / 2 * (1 + dS / S) + g(2)
            bound = np.abs(u) * f * (rel_f + g(1)) * (1 + rel_f) + e * f * (1 + rel_f)
        bound = np.asarray(bound, dtype=np.float64)
        for name, got in (("device", host(plda_transform(engine, model, x, n, **kw))), ("twin", plda_transform_host(model, x, n, **kw))):
            err = np.abs(np.asarray(LD(got) - ref, dtype=np.float64))
            print(f"D={D} norm={norm} {name}: max err/bound {np.max(err / bound):.3g}")
            assert (err <= bound).all(), (D, norm, name)
            if norm == 1:
                assert np.allclose((got ** 2).sum(axis=1), D, rtol=1e-12, atol=0)
