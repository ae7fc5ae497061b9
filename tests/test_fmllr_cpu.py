"""fMLLR estimation: the oracle's accumulation against the float64 restatement (oracle/np_oracle.py) over the
case grid the device is tested on — the figures the device's bound is derived from —; the host solver, the oracle's solver
and the restatement's on identical statistics; degenerate statistics; transform composition; and the defining property —
features distorted by a known affine map are pulled back towards the model."""
import warnings

import numpy as np
import pytest

from montreal_forced_aligner_amd import fmllr as F
from oracle import np_oracle as N
from oracle import oracle as O
from tests import helpers


def _np_acc(feats, ali_pdf, weight, am):
    r = N.fmllr_acc(feats, ali_pdf, weight, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
    return r["beta"], r["K"], r["G"]


def _data(rng, am, n_frames, W_true=None):
    D = am.dim
    pdfs = rng.integers(0, am.num_pdfs, size=n_frames).astype(np.int32)
    feats = np.zeros((n_frames, D), np.float32)
    for t, p in enumerate(pdfs):
        g = rng.integers(am.pdf_offsets[p], am.pdf_offsets[p + 1])
        var = 1.0 / am.inv_vars[g]
        feats[t] = am.means_invvars[g] * var + np.sqrt(var) * rng.normal(size=D)
    if W_true is not None:  # speaker distortion: x_spk = A^-1 (x - b)  ⇒  the estimate should recover (A, b)
        A, b = W_true[:, :D], W_true[:, D]
        feats = ((feats - b) @ np.linalg.inv(A).T).astype(np.float32)
    return feats, pdfs


def test_accumulation_oracle_vs_numpy():
    rng = np.random.default_rng(0)
    am = helpers.random_gmm(rng, 12, [1, 3, 8, 5, 32, 2])
    feats, pdfs = _data(rng, am, 300)
    w = (rng.random(300) > 0.2).astype(np.float32)
    beta, K, G = O.fmllr_acc(feats, pdfs, w, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
    b2, K2, G2 = _np_acc(feats, pdfs, w, am)
    assert abs(beta[0] - b2) < 1e-3 and abs(beta[0] - w.sum()) < 1e-3
    assert np.allclose(K, K2, rtol=1e-4, atol=1e-3) and np.allclose(G, G2, rtol=1e-4, atol=1e-3)
    assert np.allclose(G, np.transpose(G, (0, 2, 1)))


def test_solver_host_vs_oracle_and_recovers_known_transform():
    rng = np.random.default_rng(1)
    D = 10
    am = helpers.random_gmm(rng, D, [4] * 30)
    W_true = np.concatenate([np.eye(D) + 0.08 * rng.normal(size=(D, D)), 0.5 * rng.normal(size=(D, 1))], axis=1)
    feats, pdfs = _data(rng, am, 4000, W_true)
    stats = O.fmllr_acc(feats, pdfs, np.ones(4000, np.float32), am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
    beta, K, G = stats[0][0], stats[1], stats[2]
    W_o, impr_o = O.fmllr_solve(beta, K, G)
    W_h, impr_h = F.compute_fmllr(beta, K, G)
    assert impr_o > 0 and abs(impr_o - impr_h) < 1e-6 * abs(impr_o) + 1e-6
    assert np.abs(W_o - W_h).max() < 1e-4
    assert np.abs(W_h - W_true).max() < 0.15  # sampling noise of 4000 frames
    # below min_count: identity, no improvement
    W_i, impr_i = F.compute_fmllr(100.0, K, G)
    assert impr_i == 0.0 and np.array_equal(W_i[:, :D], np.eye(D, dtype=np.float32))
    assert O.fmllr_solve(100.0, K, G)[1] == 0.0


def test_two_model_accumulation_and_transform_composition():
    """Two-model form (posteriors from the alignment model, statistics from the final model — MFA/corpus/features.py:503-511)
    against a float64 numpy restatement, and compose_transforms (previous_transform_archive, :482-512) as plain algebra."""
    rng = np.random.default_rng(12)
    D, T = 5, 60
    sizes = [3, 1, 4]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)

    def model(seed):
        r = np.random.default_rng(seed)
        n = int(offs[-1])
        mean = r.normal(0, 2, size=(n, D)); var = r.uniform(0.5, 2, size=(n, D))
        w = np.concatenate([r.dirichlet(np.ones(s)) for s in sizes])
        gc = np.log(w) - 0.5 * (D * np.log(2 * np.pi) + np.log(var).sum(1) + (mean * mean / var).sum(1))
        return gc.astype(np.float32), (mean / var).astype(np.float32), (1 / var).astype(np.float32)

    gc_a, mi_a, iv_a = model(1)
    gc_f, mi_f, iv_f = model(2)
    x = rng.normal(0, 2, size=(T, D)).astype(np.float32)
    pdf = rng.integers(0, len(sizes), size=T).astype(np.int32)
    w = (rng.random(T) > 0.2).astype(np.float32)
    beta, K, G = O.fmllr_acc(x, pdf, w, gc_a, mi_a, iv_a, offs, stat_means_invvars=mi_f, stat_inv_vars=iv_f)
    r = N.fmllr_acc(x, pdf, w, gc_a, mi_a, iv_a, offs, stat_means_invvars=mi_f, stat_inv_vars=iv_f)
    rb, rK, rG = r["beta"], r["K"], r["G"]
    assert abs(beta[0] - rb) < 1e-4 and np.allclose(K, rK, rtol=1e-4, atol=1e-3) and np.allclose(G, rG, rtol=1e-4, atol=1e-3)
    W1 = np.concatenate([np.eye(D) + 0.1 * rng.normal(size=(D, D)), rng.normal(size=(D, 1))], axis=1).astype(np.float32)
    W2 = np.concatenate([np.eye(D) + 0.1 * rng.normal(size=(D, D)), rng.normal(size=(D, 1))], axis=1).astype(np.float32)
    Wc = F.compose_transforms(W2, W1)
    v = rng.normal(size=D)
    once = W1[:, :D] @ v + W1[:, D]
    assert np.allclose(Wc[:, :D] @ v + Wc[:, D], W2[:, :D] @ once + W2[:, D], atol=1e-5)


# ---- the oracle against the float64 restatement, on the grid of tests/test_gpu_fmllr_stats.py ----------------------------
def test_oracle_accumulation_against_float64_over_the_device_grid():
    """The oracle forms log-likelihoods, posteriors, a and b in float32 (as Kaldi and as the device), the restatement in
    float64.  Its worst distance in units of ε32·S (S: the absolute sums N.fmllr_acc returns) over every case the device is
    tested on is the figure the device's bound is four times of: printed here, and it must be what
    tests/helpers.py states (FMLLR_ORACLE_*, to half a percent)."""
    fx = helpers.Fixtures()
    worst = np.zeros(3)
    cases = [(n, None) for n in helpers.fmllr_case_names()] + [("fixture-one", False), ("fixture-two", True)]
    for name, two in cases:
        case = helpers.fmllr_case(name) if two is None else helpers.fmllr_fixture_case(fx, two)
        ids, orc, ref = helpers.fmllr_expected(case)
        d = np.max([helpers.fmllr_distance(o, r) for o, r in zip(orc, ref)], axis=0)
        print(f"{name:14s} {len(case['ali']):6d} frames {len(ids):3d} speakers: oracle - float64 in eps32*S: "
              f"beta {d[0]:.2f} K {d[1]:.2f} G {d[2]:.2f}")
        assert np.isfinite(d).all(), name           # (inf: something non-zero where nothing was summed)
        for (b, K, G), r in zip(orc, ref):
            assert np.array_equal(G, np.transpose(G, (0, 2, 1))), name
            if r["S_beta"] == 0:
                assert b == 0 and not K.any() and not G.any(), name
        worst = np.maximum(worst, d)
    print(f"worst over the grid: beta {worst[0]:.3f} K {worst[1]:.2f} G {worst[2]:.2f}; "
          f"stated: {helpers.FMLLR_ORACLE_BETA} {helpers.FMLLR_ORACLE_K} {helpers.FMLLR_ORACLE_G}")
    for got, stated in zip(worst, (helpers.FMLLR_ORACLE_BETA, helpers.FMLLR_ORACLE_K, helpers.FMLLR_ORACLE_G)):
        assert abs(got - stated) <= 0.005 * stated


def test_oracle_chain_through_the_solver():
    """Oracle statistics → oracle solver against restatement statistics → restatement solver, in ulp of max|W|: the figure
    the device chain's bound in tests/test_gpu_fmllr_stats.py is four times of (plus one ulp for its stored result)."""
    worst = 0.0
    for name in [f"shape-D{d}-{form}" for d in (39, 40, 41) for form in ("one", "two")]:
        case = helpers.fmllr_case(name)
        ids, orc, ref = helpers.fmllr_expected(case)
        for k in range(len(ids)):
            W64, impr = N.fmllr_solve(ref[k]["beta"], ref[k]["K"], ref[k]["G"], min_count=100.0)
            Wo, impr_o = O.fmllr_solve(*orc[k], min_count=100.0)
            d = float(np.abs(Wo - W64).max()) / (helpers.EPS32 * float(np.abs(W64).max()))
            print(f"{name} speaker {ids[k]}: beta {ref[k]['beta']:.0f}, |W oracle chain - W float64 chain| {d:.2f} ulp of max|W|")
            assert impr > 0 and impr_o > 0
            worst = max(worst, d)
    print(f"worst {worst:.2f}; stated {helpers.FMLLR_ORACLE_W}")
    assert abs(worst - helpers.FMLLR_ORACLE_W) <= 0.005 * helpers.FMLLR_ORACLE_W


def test_grid_reaches_what_it_is_for():
    """Every pdf is aligned somewhere; the pdfs of 65 – 128 Gaussians (the frame kernel's second round) carry at least 50
    weighted frames each; the hard posteriors really are one-hot."""
    for name in helpers.fmllr_case_names():
        case = helpers.fmllr_case(name)
        pdf, w = helpers.fmllr_frame_weights(case)
        if name.startswith("shape") or name == "long":
            assert set(pdf[pdf >= 0].tolist()) == set(range(len(case["sizes"]))), name
        for p, n in enumerate(case["sizes"]):
            if n > 64 and not name.startswith("spk"):
                assert w[pdf == p].sum() >= 50, (name, n, w[pdf == p].sum())
    assert (helpers.fmllr_frame_weights(helpers.fmllr_case("hard-far"))[1] > 0).sum() > 1000


# ---- the three solvers on identical statistics --------------------------------------------------------------------------
def _good_stats(D, seed=5, n_frames=4000):
    rng = np.random.default_rng(seed + D)
    am = helpers.random_gmm(rng, D, [4] * 30)
    W_true = np.concatenate([np.eye(D) + 0.3 / np.sqrt(D) * rng.normal(size=(D, D)), 0.5 * rng.normal(size=(D, 1))], axis=1)
    feats, pdfs = _data(rng, am, n_frames, W_true)
    r = N.fmllr_acc(feats, pdfs, np.ones(n_frames), am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
    return r["beta"], r["K"], r["G"], W_true


@pytest.mark.parametrize("D", [13, 39, 40, 41])
def test_solvers_agree_on_well_conditioned_statistics(D):
    beta, K, G, W_true = _good_stats(D)
    W_h, i_h = F.compute_fmllr(beta, K, G)
    W_o, i_o = O.fmllr_solve(beta, K, G)
    trace = []
    W_n, i_n = N.fmllr_solve(beta, K, G, trace=trace)
    ulp = helpers.EPS32 * float(np.abs(W_n).max())
    d_h, d_o = np.abs(W_h - W_n.astype(np.float32)).max(), np.abs(W_o - W_n.astype(np.float32)).max()
    print(f"D {D}: max|W| {np.abs(W_n).max():.3f}; host - restatement {d_h / ulp:.2f} ulp, oracle - restatement {d_o / ulp:.2f} ulp; "
          f"improvement {i_n:.6f}, host {abs(i_h - i_n) / i_n:.1e}, oracle {abs(i_o - i_n) / i_n:.1e} relative")
    assert W_h.dtype == np.float32 and d_h <= 2 * ulp and d_o <= 2 * ulp
    assert i_n > 0 and abs(i_h - i_n) <= 1e-9 * i_n and abs(i_o - i_n) <= 1e-9 * i_n
    assert np.abs(W_h - W_true).max() < 0.2                                   # an estimate of the distortion
    # the auxiliary function never decreases from sweep to sweep: the restatement's trace, and the other two by their
    # improvement after 1, 2, … sweeps
    assert len(trace) == 41 and all(b >= a - 1e-9 * abs(a) for a, b in zip(trace, trace[1:]))
    for solve in (F.compute_fmllr, O.fmllr_solve):
        imp = [solve(beta, K, G, num_iters=n)[1] for n in (0, 1, 2, 3, 5, 10, 20, 40)]
        assert imp[0] == 0.0 and all(b >= a - 1e-9 * abs(a) for a, b in zip(imp, imp[1:])), imp
    # init= is honoured: it is what no sweep returns, what a rejected estimate returns, and where the sweeps start
    rng = np.random.default_rng(D)
    W1 = np.concatenate([np.eye(D) + 0.05 * rng.normal(size=(D, D)), 0.1 * rng.normal(size=(D, 1))], axis=1).astype(np.float32)
    assert np.array_equal(F.compute_fmllr(beta, K, G, num_iters=0, init=W1)[0], W1)
    assert np.array_equal(F.compute_fmllr(beta, K, G, min_count=beta + 1, init=W1)[0], W1)
    W_hi, i_hi = F.compute_fmllr(beta, K, G, num_iters=2, init=W1)
    W_ni, i_ni = N.fmllr_solve(beta, K, G, num_iters=2, init=W1)
    assert np.abs(W_hi - W_ni.astype(np.float32)).max() <= 2 * ulp and abs(i_hi - i_ni) <= 1e-9 * abs(i_ni)
    assert not np.array_equal(W_hi, F.compute_fmllr(beta, K, G, num_iters=2)[0])
    # min_count: an estimate at β = min_count, none just below
    below = np.nextafter(beta, np.inf)
    for solve in (F.compute_fmllr, O.fmllr_solve):
        W_at, i_at = solve(beta, K, G, min_count=beta)
        W_b, i_b = solve(beta, K, G, min_count=below)
        assert i_at > 0 and np.array_equal(W_at, solve(beta, K, G)[0])
        assert i_b == 0.0 and np.array_equal(W_b, np.eye(D, D + 1, dtype=np.float32))
    assert N.fmllr_solve(beta, K, G, min_count=below)[1] == 0.0
    assert F.estimate_fmllr(beta, K, G)[2] is None and F.estimate_fmllr(beta, K, G, min_count=below)[2] == F.COUNT


# ---- degenerate statistics ----------------------------------------------------------------------------------------------
DEGENERATE = ("all_zero", "constant", "rank5", "zero_b_row", "nan_in_K", "thirty_heavy_frames")


def _degenerate_stats(kind, D=40, T=600):
    """β ≥ 500 (min_count) in every case: the count does not stop the solver, the statistics must."""
    if kind in ("zero_b_row", "nan_in_K"):
        beta, K, G, _ = _good_stats(D)
        K, G = K.copy(), G.copy()
        if kind == "zero_b_row":
            G[7] = 0.0
        else:
            K[3, 5] = np.nan
        return beta, K, G
    rng = np.random.default_rng(77)
    am = helpers.random_gmm(rng, D, [4] * 10)
    w = np.ones(T)
    if kind == "thirty_heavy_frames":
        T, w = 30, np.full(30, 20.0)
    pdfs = rng.integers(0, am.num_pdfs, size=T).astype(np.int32)
    x = {"all_zero": np.zeros((T, D)), "constant": np.tile(rng.normal(size=(1, D)), (T, 1)),
         "rank5": rng.normal(size=(T, 5)) @ rng.normal(size=(5, D)),
         "thirty_heavy_frames": helpers.fmllr_draw(rng, am, pdfs)}[kind].astype(np.float32)
    r = N.fmllr_acc(x, pdfs, w, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets)
    assert r["beta"] >= 500.0
    return r["beta"], r["K"], r["G"]


@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_statistics_are_rejected_quietly(kind):
    """Digital silence gives constant features (G_d of rank 1); a muted channel must cost its speaker the transform, not the
    corpus its run: both solvers return the starting transform and 0.0, raise nothing and warn of nothing."""
    beta, K, G = _degenerate_stats(kind)
    D = K.shape[0]
    rng = np.random.default_rng(1)
    W1 = np.concatenate([np.eye(D) + 0.05 * rng.normal(size=(D, D)), 0.1 * rng.normal(size=(D, 1))], axis=1).astype(np.float32)
    eye = np.eye(D, D + 1, dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        W, impr, why = F.estimate_fmllr(beta, K, G)
        Wi, impr_i = F.compute_fmllr(beta, K, G, init=W1)
        Wo, impr_o = O.fmllr_solve(beta, K, G)
    assert impr == 0.0 and np.array_equal(W, eye) and W.dtype == np.float32
    assert why == F.DEGENERATE                 # the reason CorpusAligner.fmllr_rejected goes by: not the count, not the objective
    assert impr_i == 0.0 and np.array_equal(Wi, W1)
    assert impr_o == 0.0 and np.array_equal(Wo, eye)


# ---- composition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [39, 40, 41])
def test_compose_transforms_is_one_after_the_other(D):
    rng = np.random.default_rng(100 + D)

    def affine():
        return np.concatenate([np.eye(D) + 0.1 * rng.normal(size=(D, D)), rng.normal(size=(D, 1))], axis=1).astype(np.float32)

    W1, W2 = affine(), affine()
    Wc = F.compose_transforms(W2, W1)
    assert Wc.dtype == np.float32 and Wc.shape == (D, D + 1)
    v = rng.normal(0, 5, size=(50, D))
    xi = np.concatenate([v, np.ones((50, 1))], axis=1)
    once = xi @ W1.astype(np.float64).T
    twice = np.concatenate([once, np.ones((50, 1))], axis=1) @ W2.astype(np.float64).T
    # the stored product is rounded to float32 once per entry: at most ε32/2 of |Wc|·|ξ| a row
    bound = 0.5 * helpers.EPS32 * (np.abs(xi) @ np.abs(Wc.astype(np.float64)).T) * 1.01
    assert (np.abs(xi @ Wc.astype(np.float64).T - twice) <= bound).all()
    # a rejected estimate is the identity: the composition is the previous transform, bit for bit
    eye = np.eye(D, D + 1, dtype=np.float32)
    assert F.compose_transforms(eye, W1).tobytes() == W1.tobytes()
    assert F.compose_transforms(W1, eye).tobytes() == W1.tobytes()
