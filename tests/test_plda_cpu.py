"""The PLDA stage without a GPU: the model's formulas by hand, the expanded form against the direct one, the EM estimate and
the adaptation on data drawn from known models, the file, the host twins against the longdouble restatement
(tests/plda_ref.py), the premises of the GPU tests' cases, and the twins' translation unit under the host sanitizers as a
stand-alone program (nothing is preloaded anywhere)."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.stats import (plda_classify_host, plda_knn_host, plda_prepare_host, plda_scores_host, plda_sweep_host,
                                               plda_transform_host)
from tests import plda_ref as R

ROOT = Path(__file__).resolve().parent.parent


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32).tolist()


# ---- by hand -----------------------------------------------------------------------------------------------------------------
def test_llr_and_transform_by_hand():
    m = P.PldaModel([1.0, -1.0], [[2.0, 0.0], [1.0, 1.0]], [3.0, 1.0])
    assert m.offset.tolist() == [-2.0, 0.0]
    # x = (2, 1): u = T x + offset = (4 − 2, 3 + 0) = (2, 3)
    assert m.transform_ivector([2.0, 1.0], normalize_length=False).tolist() == [2.0, 3.0]
    # simple: √2 / √13;   the model's, n = 1: √(2 / (4 / (3 + 1) + 9 / (1 + 1))) = √(2 / 5.5);   n = 2: √(2 / (4 / 3.5 + 9 / 1.5))
    np.testing.assert_allclose(m.transform_ivector([2.0, 1.0], simple_length_norm=True), np.array([2.0, 3.0]) * math.sqrt(2 / 13), rtol=1e-15)
    np.testing.assert_allclose(m.transform_ivector([2.0, 1.0]), np.array([2.0, 3.0]) * math.sqrt(2 / 5.5), rtol=1e-15)
    np.testing.assert_allclose(m.transform_ivector([2.0, 1.0], 2), np.array([2.0, 3.0]) * math.sqrt(2 / (4 / 3.5 + 6.0)), rtol=1e-15)
    # LLR, train (1, 2) with n = 2, test (2, −1):
    #   k = 0: ψ = 3: mean = 6/7·1, var = 1 + 3/7 = 10/7;   k = 1: ψ = 1: mean = 2/3·2 = 4/3, var = 1 + 1/3 = 4/3
    given = -0.5 * (math.log(10 / 7) + math.log(4 / 3) + (2 - 6 / 7) ** 2 / (10 / 7) + (-1 - 4 / 3) ** 2 / (4 / 3))
    without = -0.5 * (math.log(4.0) + math.log(2.0) + 4 / 4 + 1 / 2)
    assert m.log_likelihood_ratio([1.0, 2.0], 2, [2.0, -1.0]) == pytest.approx(given - without, rel=1e-14)
    assert float(R.llr(m.psi, [[1.0, 2.0]], [2], [[2.0, -1.0]])[0, 0]) == pytest.approx(given - without, rel=1e-14)
    np.testing.assert_allclose(P.normalize_length(np.array([[3.0, 4.0], [0.0, 0.0]])),
                               [[3 * math.sqrt(2) / 5, 4 * math.sqrt(2) / 5], [0.0, 0.0]], rtol=1e-15)
    assert P.subtract_mean(np.array([[1.0, 2.0], [3.0, 6.0]])).tolist() == [[-1.0, -2.0], [1.0, 2.0]]


# ---- expanded against direct -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 3, 4, 5, 16, 17, 192))
def test_expanded_form_against_the_direct_form(D):
    """The twin (expanded form, float64) and numpy's restatement of the operands against the longdouble direct form under
    the bound of tests/plda_ref.py; and the premises of the GPU tests' cases, from the restatement alone: the bound's premise
    on c_j, and at most 5 % of rows without a clear gap."""
    from tests.test_gpu_plda import KS, pairs
    left_out = total = 0
    for nt, ns in pairs(D):
        psi, train, n, test = R.random_case(D, nt, ns, seed=D * 100 + nt + 3 * ns)
        R.check_case(psi, train, n, test)
        ref, bound = R.llr(psi, train, n, test), R.error_bound(psi, train, n, test)
        model = P.PldaModel(np.zeros(D), np.eye(D), psi)
        got = plda_scores_host(model, test, train, n)
        assert (np.abs(np.asarray(R.LD(got) - ref, dtype=np.float64)) <= bound).all(), (D, nt, ns)
        A, B, c = P.expanded_operands(psi, train, n)
        np_form = c[None, :] + (test ** 2) @ A.T + test @ B.T
        assert (np.abs(np.asarray(R.LD(np_form) - ref, dtype=np.float64)) <= bound).all(), (D, nt, ns)
        hA, hB, hc = plda_prepare_host(model, train, n)
        assert bits(hA) == bits(A) and bits(hB) == bits(B)                  # basic operations in the same order
        np.testing.assert_allclose(hc, c, rtol=0, atol=R.gamma(D + 18) * float(R.bracket(psi, train, n, test)[1].max()))
        own = np.abs(np.asarray(R.LD(model.log_likelihood_ratios(train, n, test)) - ref, dtype=np.float64))
        assert (own <= R.direct_form_error(psi, train, n, test)).all(), (D, nt, ns)   # the float64 direct form's own rounding
        for k in KS:
            clear, _, _ = R.clear_rows(np.asarray(ref, dtype=np.float64), bound, k, nt == ns and k == 5)
            left_out, total = left_out + int((~clear).sum()), total + nt
    assert left_out <= 0.05 * total, (left_out, total)


def test_twin_selections_and_edge_rules():
    test, A, B, c = R.exact_case(5, 17, 40, seed=4)
    want = np.asarray(R.exact_scores(test, A, B, c), dtype=np.float64)
    for k in (1, 5, 64):
        for excl in (False, True):
            s, b, q = plda_sweep_host(test, A, B, c, excl, k)
            ri, rs = R.stable_topk(want, k, excl)
            assert bits(s) == bits(want) and bits(q[0]) == bits(ri) and bits(q[1]) == bits(rs)
            assert bits(b[0]) == bits(ri[:, 0]) and bits(b[1]) == bits(rs[:, 0])
    assert (want[:, 0] == want[:, 39]).all()                 # identical columns: a tie in every row, the lower index first
    s, b, q = plda_sweep_host(test, A, B, c, False, 64)
    for row in q[0]:
        assert list(row).index(0) < list(row).index(39)
    t2 = test.copy()
    t2[3, 1] = np.nan
    c2 = c.copy()
    c2[7] = np.nan
    s, b, q = plda_sweep_host(t2, A, B, c2, False, 5)
    assert np.isnan(s[3]).all() and np.isnan(s[:, 7]).all() and b[0][3] == -1 and np.isneginf(b[1][3]) and (q[0] != 7).all()
    keep = np.ones_like(want, bool)
    keep[3, :] = keep[:, 7] = False
    assert bits(s[keep]) == bits(want[keep])


def test_twins_against_the_restatement_transform():
    rng = np.random.default_rng(3)
    D, N = 17, 40
    x = rng.standard_normal((N, D))
    model = P.PldaModel(rng.standard_normal(D), rng.standard_normal((D, D)) / 4, np.sort(rng.uniform(0.05, 8, D))[::-1])
    n = np.where(np.arange(N) % 2 == 0, 1, 9).astype(np.int32)
    for norm, kw in ((0, dict(normalize_length=False)), (1, dict(simple_length_norm=True)), (2, dict())):
        ref = np.asarray(R.transform(model.mean, model.transform, model.psi, x, n, norm), dtype=np.float64)
        np.testing.assert_allclose(plda_transform_host(model, x, n, **kw), ref, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(model.transform_ivector(x, n, **kw), ref, rtol=1e-12, atol=1e-13)
    xi = rng.integers(-4, 5, (N, D)).astype(np.float64)
    mi = P.PldaModel(rng.integers(-3, 4, D).astype(np.float64), rng.integers(-2, 3, (D, D)).astype(np.float64), np.ones(D))
    assert bits(plda_transform_host(mi, xi, normalize_length=False)) == bits(xi @ mi.transform.T + mi.offset)


def test_twins_refuse_what_the_contract_excludes():
    lib = _lib.lib()
    d, i = np.ones(64), np.ones(64, np.int32)
    p = lambda a: a.ctypes.data
    score = lambda D, k, psi=d, n=i, outs=(None, p(i), p(d), None, None): lib.mfa_debug_plda_score_host(p(d), 2, p(d), 3, D, p(n), p(psi), 0, k, *outs)
    assert score(4, 1) == 0
    assert score(0, 1) == -2 and score(1025, 1) == -2
    assert score(4, 0, outs=(None, None, None, p(i), p(d))) == -3 and score(4, 65, outs=(None, None, None, p(i), p(d))) == -3
    assert score(4, 1, outs=(None,) * 5) == -7
    assert score(4, 1, outs=(None, p(i), None, None, None)) == -1
    for bad in (0.0, -1.0, np.inf, np.nan):
        psi = d.copy()
        psi[3] = bad
        assert score(4, 1, psi=psi) == -4
    n = i.copy()
    n[2] = 0
    assert score(4, 1, n=n) == -6
    assert lib.mfa_debug_plda_score_host(p(d), 1 << 31, p(d), 3, 4, None, p(d), 0, 1, None, p(i), p(d), None, None) == -5
    assert lib.mfa_debug_plda_transform_host(p(d), 2, 4, p(d), p(d), p(d), None, 3, p(d.copy())) == -1
    assert lib.mfa_debug_plda_transform_host(p(d), 2, 0, p(d), p(d), p(d), None, 1, p(d.copy())) == -2


# ---- estimation ----------------------------------------------------------------------------------------------------------------
def draw_classes(D, n_classes, sizes, seed):
    """Classes from a known model: (groups, class means, within, between, mean)."""
    rng = np.random.default_rng(seed)
    Lw, Lb = rng.standard_normal((D, D)) / math.sqrt(D) + np.eye(D), rng.standard_normal((D, D)) / math.sqrt(D) + 0.7 * np.eye(D)
    within, between, mean = Lw @ Lw.T, Lb @ Lb.T, rng.standard_normal(D)
    ys = mean + rng.standard_normal((n_classes, D)) @ Lb.T
    groups = [ys[c] + rng.standard_normal((sizes[c % len(sizes)], D)) @ Lw.T for c in range(n_classes)]
    return groups, ys, within, between, mean


@pytest.fixture(scope="module")
def known():
    groups, ys, within, between, mean = draw_classes(4, 1500, (4, 6, 8, 6), seed=0)
    st = P.PldaStats()
    for g in groups:
        st.add_samples(1.0, g)
    st.sort()
    return dict(groups=groups, ys=ys, within=within, between=between, mean=mean, stats=st)


def test_stats_accumulate_what_they_say(known):
    st, groups = known["stats"], known["groups"]
    assert st.num_classes == 1500 and st.num_examples == sum(g.shape[0] for g in groups) and st.class_weight == 1500.0
    assert st.is_sorted() and [r[2] for r in st.records][:2] == [4, 4]
    np.testing.assert_allclose(st.sum, sum(g.mean(axis=0) for g in groups), rtol=1e-12)
    scatter = sum((g - g.mean(axis=0)).T @ (g - g.mean(axis=0)) for g in groups)
    np.testing.assert_allclose(st.offset_scatter, scatter, rtol=1e-9, atol=1e-9)


def test_estimate_recovers_the_covariances_within_sampling_error(known):
    """The EM estimate is the maximum-likelihood one given the data, so it is compared with the data's own sample covariances,
    which the test can form because it knows the class means: W_s over all deviations from the true class means, B_s over the
    true class means.  Both are averages of N resp. C outer products of Gaussian vectors, so an entry's standard error is at
    most sqrt((σ_ii σ_jj + σ_ij²)/N) ≤ sqrt(2) σ_max/sqrt(N); the estimate sees class means only through n ≈ 6 noisy examples,
    which adds within/n of noise to each: its entries differ from B_s's by that noise's own sampling error, of the same
    order with σ → (between + within/4).  Five standard errors each."""
    st, groups, ys = known["stats"], known["groups"], known["ys"]
    within, between, _ = P.em_plda(st, 20)
    dev = np.concatenate([g - y for g, y in zip(groups, ys)])
    W_s = dev.T @ dev / dev.shape[0]
    yc = ys - ys.mean(axis=0)
    B_s = yc.T @ yc / ys.shape[0]
    se_w = 5 * math.sqrt(2) * W_s.diagonal().max() / math.sqrt(dev.shape[0])
    se_b = 5 * math.sqrt(2) * (B_s + W_s / 4).diagonal().max() / math.sqrt(ys.shape[0])
    print("within err", np.abs(within - W_s).max(), "allowed", se_w, "between err", np.abs(between - B_s).max(), "allowed", se_b)
    assert np.abs(within - W_s).max() <= se_w
    assert np.abs(between - B_s).max() <= se_b


def test_transform_whitens_and_psi_descends(known):
    st = known["stats"]
    model = P.estimate_plda(st, 10)
    within, between, _ = P.em_plda(st, 10)
    T = model.transform
    np.testing.assert_allclose(T @ within @ T.T, np.eye(4), atol=1e-10)
    np.testing.assert_allclose(T @ between @ T.T, np.diag(model.psi), atol=1e-10)
    assert (np.diff(model.psi) <= 0).all() and (model.psi >= 0).all()
    np.testing.assert_allclose(model.mean, st.sum / st.class_weight)
    # the within-class scatter of the data, transformed: the identity up to what EM moved between the two covariances
    scatter = T @ (st.offset_scatter / (st.example_weight - st.class_weight)) @ T.T
    np.testing.assert_allclose(scatter, np.eye(4), atol=0.05)
    w2, b2 = model.covariances()
    np.testing.assert_allclose(w2, within, atol=1e-9)
    np.testing.assert_allclose(b2, between, atol=1e-9)


def test_marginal_likelihood_does_not_fall(known):
    _, _, objs = P.em_plda(known["stats"], 12)
    print("objective per example:", np.round(objs, 6))
    assert len(objs) == 13 and (np.diff(objs) >= -1e-12).all() and objs[-1] > objs[0]


def test_objective_is_the_joint_density_of_a_class():
    """One class of three examples in one dimension against the joint Gaussian written out: covariance w I + b 11ᵀ."""
    x = np.array([[0.3], [1.1], [-0.4]])
    st = P.PldaStats()
    st.add_samples(1.0, x)
    w, b = 0.7, 1.9
    cov = w * np.eye(3) + b * np.ones((3, 3))
    d = x[:, 0] - st.sum[0]                                   # the objective centres on the mean of the class means
    joint = -0.5 * (3 * math.log(2 * math.pi) + np.linalg.slogdet(cov)[1] + d @ np.linalg.solve(cov, d))
    assert P.plda_objective(st, np.array([[w]]), np.array([[b]])) * 3 == pytest.approx(joint, rel=1e-12)


def test_the_three_refusals():
    rng = np.random.default_rng(0)
    vec = lambda: rng.standard_normal(3)
    with pytest.raises(P.PldaTrainingError, match="No stats accumulated"):
        P.train_plda({}, {})
    with pytest.raises(P.PldaTrainingError, match="No stats accumulated"):
        P.train_plda({"a": vec(), "b": vec()}, {"a": "s", "b": "t"}, minimum_utterance_count=2)
    with pytest.raises(P.PldaTrainingError, match="not greater than their dimension"):
        P.train_plda({"a": vec(), "b": vec(), "c": vec()}, {"a": "s", "b": "s", "c": "t"})
    with pytest.raises(P.PldaTrainingError, match="No speakers with multiple utterances"):
        P.train_plda({k: vec() for k in "abcde"}, {k: k for k in "abcde"})
    m = P.train_plda({k: vec() for k in "abcdefgh"}, {k: "s" + str(i // 2) for i, k in enumerate("abcdefgh")})
    assert m.dim == 3 and (np.diff(m.psi) <= 0).all()


# ---- adaptation -----------------------------------------------------------------------------------------------------------------
def model_data(model, n_classes, per_class, seed, scale=None):
    """Examples of ``model``'s own distribution in the original space (``scale``: per-direction factors in the model's space)."""
    rng = np.random.default_rng(seed)
    D = model.dim
    y = rng.standard_normal((n_classes, D)) * np.sqrt(model.psi)
    u = np.repeat(y, per_class, axis=0) + rng.standard_normal((n_classes * per_class, D))
    if scale is not None:
        u = u * scale
    return u @ np.linalg.inv(model.transform).T + model.mean


def test_adapting_to_the_models_own_data_moves_little():
    """Data drawn from the model has, in the model's space scaled by 1/√(1 + ψ), the identity as its covariance: the sample
    eigenvalues are s_i = 1 + δ_i, and only the δ_i > 0 change anything.  A change of δ in one direction takes
    (within, between) = (1/(1+ψ), ψ/(1+ψ)) to (1/(1+ψ) + 0.3δ, ψ/(1+ψ) + 0.7δ), i.e. ψ to (ψ + 0.7δ(1+ψ)) / (1 + 0.3δ(1+ψ)):
    |Δψ| ≤ δ(1+ψ)(0.7 + 0.3ψ).  The eigenbasis need not be the model's, so the largest ψ stands for all:
    |ψ' − ψ| ≤ max|δ|·(1 + ψ_max)(0.7 + 0.3ψ_max)·(1 + that much again for the second order).  The δ are the test's own, from
    the data.  They are sampling noise: an entry of a sample covariance of C = 20 000 independent classes has standard error
    at most sqrt(2/C), five of which bound max|δ| here."""
    model = P.PldaModel(np.array([0.5, -1.0, 2.0]), np.array([[1.0, 0.2, 0.0], [0.0, 0.8, 0.1], [0.3, 0.0, 1.2]]), np.array([4.0, 1.5, 0.4]))
    x = model_data(model, 20000, 4, seed=1)
    ad = P.PldaUnsupervisedAdaptor()
    ad.add_stats(1.0, x[:100])
    for v in x[100:110]:
        ad.add_stats(1.0, v)
    ad.add_stats(1.0, x[110:])
    new = ad.update_plda(model)
    np.testing.assert_allclose(new.mean, x.mean(axis=0), rtol=1e-12)
    Tm = model.transform / np.sqrt(1 + model.psi)[:, None]
    xc = x - x.mean(axis=0)
    shift = Tm @ (x.mean(axis=0) - model.mean)
    delta = np.abs(np.linalg.eigvalsh(Tm @ (xc.T @ xc / x.shape[0]) @ Tm.T + np.outer(shift, shift)) - 1).max()
    assert delta <= 5 * math.sqrt(2 / 20000)
    pm = model.psi.max()
    allowed = delta * (1 + pm) * (0.7 + 0.3 * pm)
    allowed *= 1 + allowed
    print("psi'", new.psi, "psi", model.psi, "max |delta|", delta, "allowed", allowed)
    assert (np.abs(new.psi - model.psi) <= allowed).all()


def test_adaptation_splits_the_excess_variance():
    """Exact moments instead of samples: second-moment statistics built so that the data covariance in the scaled model space
    is diag(1 + e, 0.5, 1): direction 0 inflated by e, direction 1 below 1 (no excess: untouched), direction 2 as the model.
    There within' = diag(1/(1+ψ)) + 0.3·diag(e, 0, 0) and between' = diag(ψ/(1+ψ)) + 0.7·diag(e, 0, 0); in the model's own
    (unscaled) space that is I + 0.3 e (1 + ψ_0) e₀e₀ᵀ and diag(ψ) + 0.7 e (1 + ψ_0) e₀e₀ᵀ."""
    psi = np.array([3.0, 1.0, 0.5])
    T = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 2.0]])
    model = P.PldaModel(np.array([1.0, 2.0, 3.0]), T, psi)
    e = 2.5
    S = np.diag([1 + e, 0.5, 1.0])
    Tmi = np.linalg.inv(T / np.sqrt(1 + psi)[:, None])
    cov = Tmi @ S @ Tmi.T
    ad = P.PldaUnsupervisedAdaptor(mean_diff_scale=1.0)
    mean = model.mean.copy()                                  # no mean shift
    ad.tot_weight, ad.mean_stats, ad.variance_stats = 10.0, 10.0 * mean, 10.0 * (cov + np.outer(mean, mean))
    new = ad.update_plda(model)
    w, b = new.covariances()
    excess = np.diag([e * (1 + psi[0]), 0.0, 0.0])
    np.testing.assert_allclose(T @ w @ T.T, np.eye(3) + 0.3 * excess, atol=1e-10)
    np.testing.assert_allclose(T @ b @ T.T, np.diag(psi) + 0.7 * excess, atol=1e-10)
    np.testing.assert_allclose(new.mean, mean)
    # exactly the model's own moments: nothing moves
    own = Tmi @ Tmi.T
    ad0 = P.PldaUnsupervisedAdaptor()
    ad0.tot_weight, ad0.mean_stats, ad0.variance_stats = 10.0, 10.0 * mean, 10.0 * (own + np.outer(mean, mean))
    np.testing.assert_allclose(ad0.update_plda(model).psi, psi, atol=1e-10)
    # a mean shift counts as variance: mean_diff_scale·Δ Δᵀ, here 0.5·4 more in direction 0
    shift = Tmi @ np.array([2.0, 0.0, 0.0])
    ad2 = P.PldaUnsupervisedAdaptor(mean_diff_scale=0.5)
    m2 = mean + shift
    ad2.tot_weight, ad2.mean_stats, ad2.variance_stats = 10.0, 10.0 * m2, 10.0 * (cov + np.outer(m2, m2))
    w2, _ = ad2.update_plda(model).covariances()
    np.testing.assert_allclose(T @ w2 @ T.T, np.eye(3) + 0.3 * np.diag([(e + 2.0) * (1 + psi[0]), 0, 0]), atol=1e-10)


# ---- the file -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", (True, False))
def test_file_round_trip(tmp_path, binary):
    rng = np.random.default_rng(5)
    m = P.PldaModel(rng.standard_normal(5), rng.standard_normal((5, 5)), np.sort(rng.random(5))[::-1])
    m.write(tmp_path / "plda", binary=binary)
    back = P.PldaModel.read(tmp_path / "plda")
    assert bits(back.mean) == bits(m.mean) and bits(back.transform) == bits(m.transform) and bits(back.psi) == bits(m.psi)
    data = (tmp_path / "plda").read_bytes()
    assert data.startswith(b"\0B<Plda> DV " if binary else b"<Plda>  [ ")
    assert bits(P.PldaModel.read(data).psi) == bits(m.psi)
    with pytest.raises(Exception):
        P.PldaModel.read(data[: len(data) // 2])


def test_kalpy_surface_on_the_host():
    from montreal_forced_aligner_amd import kalpy_api as K
    groups, *_ = draw_classes(3, 60, (3, 5), seed=2)
    stats = K.PldaStats()
    for g in groups:
        stats.AddSamples(1.0, g)
    stats.Sort()
    assert stats.Dim() == 3
    plda = K.Plda()
    K.PldaEstimator(stats).Estimate(K.PldaEstimationConfig(), plda)
    assert plda.Dim() == 3
    a, b = plda.transform_ivector(groups[0][0], 1), plda.transform_ivector(groups[0][1], 1)
    assert plda.distance(a, b) == -plda.log_likelihood(a, 1, b)
    ad = K.PldaUnsupervisedAdaptor()
    for g in groups[:20]:
        for v in g:
            ad.AddStats(1.0, v)
    before = plda.model
    ad.UpdatePlda(K.PldaUnsupervisedAdaptorConfig(), plda)
    assert plda.model is not before
    np.testing.assert_allclose(plda.model.mean, np.concatenate(groups[:20]).mean(axis=0))
    v = np.array([3.0, 4.0, 0.0])
    assert K.ivector_normalize_length(v) is v and np.allclose(v, np.array([3.0, 4.0, 0.0]) * math.sqrt(3) / 5)
    rows = [np.array([1.0, 2.0, 3.0]), np.array([3.0, 2.0, 1.0])]
    assert K.ivector_subtract_mean(rows).tolist() == [[-1.0, 0.0, 1.0], [1.0, 0.0, -1.0]] and rows[0].tolist() == [-1.0, 0.0, 1.0]
    scorer = K.PldaScorer(plda, backend="host")
    means = [(f"s{i}", g.mean(axis=0)) for i, g in enumerate(groups)]
    scorer.load_speaker_ivectors(means, {f"s{i}": g.shape[0] for i, g in enumerate(groups)})
    idx, llr = scorer.classify_speakers(np.stack([g[0] for g in groups]))
    one = scorer.classify_speaker(groups[7][0])
    assert one == (int(idx[7]), float(llr[7])) and scorer.num_speaker_examples.tolist()[:2] == [3, 5]


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "plda_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "plda_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "plda_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
