"""GMM statistics from two feature matrices on the device (mfa_gmm_acc_twofeats_batch: gmm_acc_kernel<true> of
csrc/gmm_acc.hip between the lookup, ordering and reductions it shares with mfa_gmm_acc_batch): posteriors from
``feats_post``, sums from ``feats_sum``.  The three tiers and the bounds of tests/test_gpu_gmm_acc.py (its docstring
derives them), with S = Σ γ|term| taken over ``feats_sum``, whose rows are the sums' terms; C =
mfa_gmm_acc_chunk_frames().

0. Equal matrices: the contract's stated consequence, the bits of mfa_gmm_acc_batch on that input.
1. Single-Gaussian pdfs: γ = w exactly whatever ``feats_post`` holds, so the sums are exact sums of ``feats_sum``'s rows and
   tot_like is the one-feature call's on ``feats_post``, bit for bit.
2. One-hot mixtures: ``feats_post`` within 3 deviations of one component of means 40 deviations apart, ``feats_sum``
   independent of it.  Sizes 2 … 128 and a pdf of 64 beside one of 65 Gaussians: the second round of the posterior phase
   (its weight reload) with a single Gaussian in it.
3. Soft: tests/gmm_acc2_ref.py's cases against the two-feature host twin (13.5 ε32·S + 2T·2⁻⁵³·S) and against the float64
   restatement under its derived bound."""
import functools

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd._lib import MfaHipError, check
from montreal_forced_aligner_amd.engine import (GmmStats, _ptr, gmm_statistics, gmm_statistics_twofeats, gmm_statistics_twofeats_host,
                                                tid_tables)
from tests import gmm_acc2_ref as R2
from tests import gmm_ref, helpers
from tests.test_gmm_acc_twofeats_cpu import check_against_float64
from tests.test_gpu_gmm_acc import DEVICE_VS_TWIN, DEVICE_VS_TWIN_LL, check_exact_tier, one_hot_case

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def device_stats2(engine, am, feats_post, feats_sum, ali, tm, weights=None, into=None, load=True):
    if load:
        engine.load_gmm(am)
    return gmm_statistics_twofeats(engine, _dev(engine, feats_post), _dev(engine, feats_sum), _dev(engine, ali), tm, weights, into=into)


def device_stats1(engine, feats, ali, tm, weights=None):
    return gmm_statistics(engine, _dev(engine, feats), _dev(engine, ali), tm, weights)


def _bits(st):
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count], st.tid_count))


def _chunk(engine):
    return int(engine.lib.mfa_gmm_acc_chunk_frames())


# ---- equal matrices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (13, 40, 48))
def test_equal_matrices_give_the_one_feature_bits(engine, dim):
    case = R2.skewed_case2(dim)
    engine.load_gmm(case.am)
    one = device_stats1(engine, case.feats, case.ali, case.tm, case.weights)
    two = device_stats2(engine, case.am, case.feats, case.feats.copy(), case.ali, case.tm, case.weights, load=False)
    assert _bits(two) == _bits(one)
    x, a = _dev(engine, case.feats), _dev(engine, case.ali)
    same = gmm_statistics_twofeats(engine, x, x, a, case.tm, case.weights)
    assert _bits(same) == _bits(one)


# ---- tier 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (13, 39, 40, 45, 48))
def test_single_gaussian_pdfs_are_exact(engine, dim):
    C = _chunk(engine)
    rng = np.random.default_rng(9400 + dim)
    P = 37
    counts = np.concatenate([[0, 1, C - 1, C, C + 1, 2 * C + 1], rng.integers(0, 300, size=P - 6)])
    counts = counts[rng.permutation(P)]
    am = helpers.random_gmm(rng, dim, [1] * P)
    tm = helpers.fmllr_tm(P)
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    weights = rng.choice(np.array([1.0, 0.5], np.float32), size=2 * P + 1)
    feats_post = helpers.fmllr_draw(rng, am, pdfs)
    feats_sum = rng.normal(size=feats_post.shape).astype(np.float32) * 3.0          # independent of feats_post
    st = device_stats2(engine, am, feats_post, feats_sum, ali, tm, weights)
    pdf, fw = R2.frame_tables(tm, ali, weights)
    check_exact_tier(st, am, feats_sum, pdf, fw, ali, 2 * P + 1, f"two features, single Gaussians dim {dim}")
    assert (st.occ[counts == 0] == 0).all() and not st.mean_acc[counts == 0].any()
    one = device_stats1(engine, feats_post, ali, tm, weights)
    assert st.tot_like == one.tot_like and st.tot_count == one.tot_count and st.occ.tobytes() == one.occ.tobytes()


# ---- tier 2 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_hot_case2(dim, C):
    """tests/test_gpu_gmm_acc.py's one-hot case with two more pdfs, of 64 and of 65 Gaussians built the same way, and a
    ``feats_sum`` drawn independently of the frames."""
    am, tm, feats, ali, weights, gauss = one_hot_case(dim, C)
    rng = np.random.default_rng(9500 + dim)
    P0, G0 = am.num_pdfs, am.num_gauss
    dev = np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=dim))
    gconsts, mi, iv, means, offs = [am.gconsts], [am.means_invvars], [am.inv_vars], [], [int(o) for o in am.pdf_offsets]
    for n in (64, 65):
        w = rng.dirichlet(np.full(n, 2.0))
        step = rng.permutation(n)[:, None] * np.ones((1, dim))
        mean = 40.0 * (step - (n - 1) / 2.0) * dev[None, :]
        var = np.tile(dev * dev, (n, 1))
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean / var).astype(np.float32)); iv.append((1.0 / var).astype(np.float32))
        means.append(mean); offs.append(offs[-1] + n)
    am2 = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    means = np.concatenate(means)
    counts = np.array([C + 30, C + 31])
    pdfs = np.repeat(np.arange(P0, P0 + 2), counts)
    g_new = np.array([rng.integers(offs[p], offs[p + 1]) for p in pdfs])
    g_new[:C + 30:7] = offs[P0] + 63                     # the last Gaussian of the first round …
    g_new[C + 30::7] = offs[P0 + 1] + 64                 # … and the only one of the second, often
    x_new = (means[g_new - G0] + rng.uniform(-3.0, 3.0, size=(len(pdfs), dim)) * dev[None, :]).astype(np.float32)
    a_new = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    order = rng.permutation(len(ali) + len(pdfs))
    feats2 = np.concatenate([feats, x_new])[order]
    ali2 = np.concatenate([ali, a_new])[order]
    gauss2 = np.concatenate([gauss, g_new])[order]
    weights2 = np.concatenate([weights, rng.choice(np.array([1.0, 0.5], np.float32), size=4)])
    feats_sum = (rng.normal(size=feats2.shape) * 2.0 + 0.5).astype(np.float32)
    return am2, helpers.fmllr_tm(P0 + 2), feats2, feats_sum, ali2, weights2, gauss2


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_one_hot_mixtures_are_exact(engine, dim):
    am, tm, feats_post, feats_sum, ali, weights, gauss = one_hot_case2(dim, _chunk(engine))
    assert {64, 65} <= set(np.diff(am.pdf_offsets).tolist())
    pdf, fw = R2.frame_tables(tm, ali, weights)
    _, post = gmm_statistics_twofeats_host(am, feats_post, feats_sum, ali, tm, weights, want_post=True)
    local = gauss - am.pdf_offsets[pdf]
    expect = np.zeros_like(post)
    expect[np.arange(len(ali)), local] = fw
    assert np.array_equal(post, expect), "host twin: posteriors are not exactly one-hot"
    st = device_stats2(engine, am, feats_post, feats_sum, ali, tm, weights)
    check_exact_tier(st, am, feats_sum, gauss, fw, ali, len(weights), f"two features, one-hot mixtures dim {dim}")


# ---- tier 3 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin(dim):
    case = R2.skewed_case2(dim)
    return case, gmm_statistics_twofeats_host(case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights)


def check_against_twin(st, twin, ref, case, what):
    """Device against the two-feature host twin: tier 3's bound of tests/test_gpu_gmm_acc.py, S over ``feats_sum``."""
    T2 = 2.0 * ref["n_frames"] * U64
    worst = {}
    for name, got, want, S, t2 in (("occ", st.occ, twin.occ, ref["occ"], T2), ("mean", st.mean_acc, twin.mean_acc, ref["S_mean"], T2[:, None]),
                                   ("var", st.var_acc, twin.var_acc, ref["var"], T2[:, None])):
        err, lim = np.abs(got - want), (DEVICE_VS_TWIN * R2.EPS32 + t2) * S
        worst[name] = float((err / np.where(S > 0, R2.EPS32 * S, 1.0)).max())
        assert (err <= lim).all(), (what, name, worst[name])
    pdf, fw = R2.frame_tables(case.tm, case.ali, case.weights)
    took = pdf >= 0
    s_ll = ref["S_tot"]
    lim_ll = R2.EPS32 * (s_ll + DEVICE_VS_TWIN_LL * float(fw[took].sum())) + 2 * took.sum() * U64 * s_ll
    worst["tot"] = abs(st.tot_like - twin.tot_like) / (R2.EPS32 * s_ll)
    print(f"{what}: device - host twin in eps32*S: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert abs(st.tot_like - twin.tot_like) <= lim_ll, (what, worst)
    assert st.tot_count == twin.tot_count and np.array_equal(st.tid_count, twin.tid_count)


@pytest.mark.parametrize("dim", gmm_ref.DIMS_SKEWED)
def test_soft_posteriors_against_the_host_twin(engine, dim):
    case, twin = _twin(dim)
    st = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights)
    ref = check_against_float64(case, st, f"device, {case.name}")
    check_against_twin(st, twin, ref, case, case.name)


# ---- reproducibility and additivity -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_split_batch_adds_up(engine):
    case, _ = _twin(40)
    args = (case.tm, case.weights)
    one = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, *args)
    again = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, *args, load=False)
    assert _bits(one) == _bits(again)
    cut = 1237
    half = device_stats2(engine, case.am, case.feats[:cut], case.feats_sum[:cut], case.ali[:cut], *args, load=False)
    both = device_stats2(engine, case.am, case.feats[cut:], case.feats_sum[cut:], case.ali[cut:], *args, into=half, load=False)
    assert both is half
    pdf, fw = R2.frame_tables(case.tm, case.ali, case.weights)
    ref = R2.gmm_acc2(case.feats, case.feats_sum, pdf, fw, case.am)
    T2 = 2.0 * ref["n_frames"] * U64
    assert (np.abs(both.occ - one.occ) <= T2 * ref["occ"]).all()
    assert (np.abs(both.mean_acc - one.mean_acc) <= T2[:, None] * ref["S_mean"]).all()
    assert (np.abs(both.var_acc - one.var_acc) <= T2[:, None] * ref["var"]).all()
    assert abs(both.tot_like - one.tot_like) <= 2 * len(pdf) * U64 * ref["S_tot"]
    assert both.tot_count == one.tot_count and np.array_equal(both.tid_count, one.tid_count)


def test_accumulators_are_added_to_and_odd_frames_leave_no_trace(engine):
    case, _ = _twin(39)
    rng = np.random.default_rng(78)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(rng.normal(size=G) * 100, rng.normal(size=(G, D)) * 100, rng.normal(size=(G, D)) * 100, -12.5, 40.0,
                     rng.integers(0, 1000, size=n_tids).astype(np.int64))
    args = (case.tm, case.weights)
    plain = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, *args)
    added = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, *args, into=start.copy(), load=False)
    pdf, fw = R2.frame_tables(case.tm, case.ali, case.weights)
    ref = R2.gmm_acc2(case.feats, case.feats_sum, pdf, fw, case.am)
    for got, zero, first, S in ((added.occ, plain.occ, start.occ, ref["occ"]), (added.mean_acc, plain.mean_acc, start.mean_acc, ref["S_mean"]),
                                (added.var_acc, plain.var_acc, start.var_acc, ref["var"])):
        nf = ref["n_frames"].reshape((-1,) + (1,) * (S.ndim - 1))
        assert (np.abs(got - (zero + first)) <= 2.0 * (nf + 1) * U64 * (S + np.abs(first))).all()
    assert np.array_equal(added.tid_count, plain.tid_count + start.tid_count)
    assert added.tot_count == plain.tot_count + 40.0
    idle = ref["n_frames"] == 0
    assert added.occ[idle].tobytes() == start.occ[idle].tobytes() and added.mean_acc[idle].tobytes() == start.mean_acc[idle].tobytes()
    odd = np.concatenate([np.zeros(300), np.full(300, n_tids), np.full(300, -7), np.full(300, 4)]).astype(np.int32)
    assert case.weights[4] == 0
    nan = np.full((len(odd), D), np.nan, np.float32)
    same = device_stats2(engine, case.am, nan, nan.copy(), odd, *args, into=start.copy(), load=False)
    assert _bits(same) == _bits(start)
    keep = pdf >= 0
    only = device_stats2(engine, case.am, case.feats[keep], case.feats_sum[keep], case.ali[keep], *args, load=False)
    assert _bits(only) == _bits(plain)


def _raw_call(engine, case, f, f2, total, cnt=None):
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    id2pdf, w = tid_tables(case.tm, case.weights)
    dev = engine.device
    occ = torch.zeros(G, dtype=torch.float64, device=dev)
    mean, var = torch.zeros((G, D), dtype=torch.float64, device=dev), torch.zeros((G, D), dtype=torch.float64, device=dev)
    tot = torch.zeros(2, dtype=torch.float64, device=dev)
    a, p, ww = _dev(engine, case.ali), _dev(engine, id2pdf), _dev(engine, w)
    rc = engine.lib.mfa_gmm_acc_twofeats_batch(engine.ctx, _ptr(f), _ptr(f2), total, _ptr(a), _ptr(p), _ptr(ww), n_tids, _ptr(occ), _ptr(mean),
                                               _ptr(var), _ptr(tot), cnt)
    torch.cuda.synchronize()
    return rc, occ, mean, var, tot


def test_empty_batch_and_no_counts(engine):
    case, _ = _twin(45)
    engine.load_gmm(case.am)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(np.ones(G), np.ones((G, D)), np.ones((G, D)), 1.0, 2.0, np.ones(n_tids, np.int64))
    empty = torch.zeros((0, D), device=engine.device)
    st = gmm_statistics_twofeats(engine, empty, empty.clone(), torch.zeros(0, dtype=torch.int32, device=engine.device), case.tm, case.weights,
                                 into=start.copy())
    assert _bits(st) == _bits(start)
    # d_tid_count NULL: the same sums
    full = device_stats2(engine, case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights, load=False)
    rc, occ, mean, var, tot = _raw_call(engine, case, _dev(engine, case.feats), _dev(engine, case.feats_sum), len(case.ali))
    check(engine.ctx, rc, "mfa_gmm_acc_twofeats_batch")
    assert occ.cpu().numpy().tobytes() == full.occ.tobytes() and mean.cpu().numpy().tobytes() == full.mean_acc.tobytes()
    assert var.cpu().numpy().tobytes() == full.var_acc.tobytes() and tot.cpu().numpy().tolist() == [full.tot_like, full.tot_count]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _small_call_is_right(engine):
    rng = np.random.default_rng(3)
    am = helpers.random_gmm(rng, 13, [1, 1, 1])
    pdfs = rng.integers(0, 3, size=50)
    feats, ali = helpers.fmllr_draw(rng, am, pdfs), (2 * pdfs + 1).astype(np.int32)
    feats_sum = rng.normal(size=feats.shape).astype(np.float32)
    st = device_stats2(engine, am, feats, feats_sum, ali, helpers.fmllr_tm(3))
    check_exact_tier(st, am, feats_sum, pdfs, np.ones(50, np.float32), ali, 7, "small call after a refusal")


def test_refusals_leave_a_message_and_a_usable_context(engine):
    from montreal_forced_aligner_amd.engine import AlignmentEngine
    rng = np.random.default_rng(4)
    fresh = AlignmentEngine(0)
    try:
        fresh.gmm = helpers.random_gmm(rng, 13, [1])          # the Python layer's own check is not what is tested here
        x = torch.zeros((4, 13), device=fresh.device)
        with pytest.raises(MfaHipError, match="mfa_load_gmm has not been called"):
            gmm_statistics_twofeats(fresh, x, x.clone(), torch.ones(4, dtype=torch.int32, device=fresh.device), helpers.fmllr_tm(1))
        _small_call_is_right(fresh)
    finally:
        fresh.close()
    z = np.zeros((4, 13), np.float32)
    big = helpers.random_gmm(rng, 13, [2, 129])
    with pytest.raises(MfaHipError, match="more than 128 Gaussians"):
        device_stats2(engine, big, z, z.copy(), np.ones(4, np.int32), helpers.fmllr_tm(2))
    _small_call_is_right(engine)
    limit = int(engine.lib.mfa_gmm_acc_max_dim())
    assert limit == 48
    wide = helpers.random_gmm(rng, limit + 1, [2, 3])
    zw = np.zeros((4, limit + 1), np.float32)
    with pytest.raises(MfaHipError, match="feature dim"):
        device_stats2(engine, wide, zw, zw.copy(), np.ones(4, np.int32), helpers.fmllr_tm(2))
    _small_call_is_right(engine)
    # the two matrices must agree in shape, dtype and device, and have the model's dim
    ok = helpers.random_gmm(rng, 13, [2, 3])
    engine.load_gmm(ok)
    tm, ali = helpers.fmllr_tm(2), torch.ones(4, dtype=torch.int32, device=engine.device)
    x = torch.zeros((4, 13), device=engine.device)
    for bad in (torch.zeros((5, 13), device=engine.device), torch.zeros((4, 12), device=engine.device),
                torch.zeros((4, 13), dtype=torch.float64, device=engine.device), torch.zeros((4, 13))):
        with pytest.raises(MfaHipError, match="differ|different devices"):
            gmm_statistics_twofeats(engine, x, bad, ali, tm)
    x14 = torch.zeros((4, 14), device=engine.device)
    with pytest.raises(MfaHipError, match="model of dim 13"):
        gmm_statistics_twofeats(engine, x14, x14.clone(), ali, tm)
    _small_call_is_right(engine)
    # the library's own refusal of a NULL sum matrix
    case, _ = _twin(13)
    engine.load_gmm(case.am)
    rc, occ, _mean, _var, tot = _raw_call(engine, case, _dev(engine, case.feats), None, len(case.ali))
    assert rc != 0 and b"d_feats_sum is NULL" in engine.lib.mfa_last_error(engine.ctx)
    assert not occ.cpu().numpy().any() and not tot.cpu().numpy().any()
    _small_call_is_right(engine)
