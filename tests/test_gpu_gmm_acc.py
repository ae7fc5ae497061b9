"""GMM statistics on the device (csrc/gmm_acc.hip: the lookup with its histograms, the ordering by pdf, gmm_acc_kernel and
the two reductions) at the shapes where the kernels can go wrong: pdfs of 0, 1, C − 1, C, C + 1, 2C + 1 frames (C =
mfa_gmm_acc_chunk_frames()), dims 13 – 48, pdfs of 1 – 128 Gaussians, frames shuffled across the batch.  Key counts (hundreds and
thousands of pdfs), pdfs of eight chunks and more and alignment-shaped frame orders are in tests/test_gpu_stats_scale.py.

Three tiers.
1. Single-Gaussian pdfs: e = expf(0) = 1, s = 1, 1/s = 1, so γ = w exactly; with weights 1 and ½ every product γ·x and γ·x² is
   exact in double.  Device and float64 numpy then form two sums of the same n exact addends in different association:
   each within (n − 1)·2⁻⁵³·S of the true sum, so within 2(n − 1)·2⁻⁵³·S of each other, S = Σ|terms|.  occ = Σ w and the
   transition-id counts are exact.
2. One-hot mixtures: means 40 deviations apart in every coordinate, frames within 3 deviations of one component.  Every
   other component is at least 37 deviations off in every coordinate: ll − m ≤ −½·dim·(37² − 3²) < −8 800 even at dim 13,
   against a float32 chain error of at most (2·dim + 1)·2⁻²⁴·M ≈ 2 400 at dim 40 (M ≈ 5·10⁸: means centred, up to ±2 540
   deviations), and expf is exactly 0 below −104.  The host twin is asserted to give exactly one-hot posteriors on every
   frame; the device then meets the bound of tier 1 per Gaussian, n its own frames (a term with γ = 0 adds exactly nothing).
3. Soft: tests/gmm_acc_ref.py's skewed cases, device against the host twin.  Both run csrc/gmm_acc_math.hpp on the same
   float32 inputs: identical log-likelihood bits.  Per frame of n ≤ 128 Gaussians they differ, in units of ε32 on a
   posterior (the derivation of tests/test_gpu_fmllr_stats.py, the terms that apply):
     exp: libm ≤ 1 ulp, device ≤ 2.5 ulp                                                           3.5
     Σ exp: n − 1 sequential additions against a 7-level tree, ½-ulp roundings as a random walk,
            (√127 + √7) / 2                                                                         7.0
     1/Σ, · inv, · weight: three roundings of ½ ulp on either side                                  3.0
   and nothing after the posteriors: the sums are double (their 2·T·2⁻⁵³·S is added).  13.5·ε32·S, S = Σ γ|term|.
   The frame's log-likelihood m + logf(s): its own rounding on either side, ε32·|LL|; s moved by 10.5 ε32 relative; logf
   3.5 ulp of at most ln 128 < 5 apart: ε32·(|LL| + 10.5 + 17.5) per unit of weight.
   The device is also held to the float64 restatement under the bound derived in tests/gmm_acc_ref.py."""
import functools

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.engine import GmmStats, gmm_statistics, gmm_statistics_host
from tests import gmm_acc_ref as R
from tests import gmm_ref, helpers
from tests.test_gmm_acc_cpu import check_against_float64

pytestmark = pytest.mark.gpu

DEVICE_VS_TWIN = 13.5          # ε32·S: see the module docstring
DEVICE_VS_TWIN_LL = 28.0       # ε32 per unit of weight, beside ε32·|LL|
U64 = 2.0 ** -53


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def device_stats(engine, am, feats, ali, tm, weights=None, into=None, load=True):
    if load:
        engine.load_gmm(am)
    return gmm_statistics(engine, _dev(engine, feats), _dev(engine, ali), tm, weights, into=into)


def _bits(st):
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count], st.tid_count))


def _chunk(engine):
    return int(engine.lib.mfa_gmm_acc_chunk_frames())


def check_exact_tier(st, am, feats, gauss, fw, ali, n_tids, what):
    """``gauss`` [T]: the one Gaussian (model index) that holds all of frame t's posterior, −1 for a frame that takes no
    part.  occ and the counts exactly; mean / var per Gaussian within 2(n − 1)·2⁻⁵³·S of float64 numpy."""
    x = feats.astype(np.float64)
    w = fw.astype(np.float64)
    worst = 0.0
    for g in range(am.num_gauss):
        rows = np.flatnonzero(gauss == g)
        n = len(rows)
        assert st.occ[g] == w[rows].sum(), (what, g)
        lim = 2 * max(n - 1, 0) * U64
        for got, terms in ((st.mean_acc[g], w[rows, None] * x[rows]), (st.var_acc[g], w[rows, None] * x[rows] * x[rows])):
            err, S = np.abs(got - terms.sum(axis=0)), np.abs(terms).sum(axis=0)
            assert (err <= lim * S).all(), (what, g, n)
            if n > 1:
                worst = max(worst, float((err / np.where(S > 0, lim * S, 1.0)).max()))
    took = gauss >= 0
    assert np.array_equal(st.tid_count, np.bincount(ali[took], minlength=n_tids)), what
    assert st.tot_count == w[took].sum(), what
    print(f"{what}: worst |device - float64| / (2(n-1) 2^-53 S) = {worst:.3f}")


# ---- tier 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (13, 39, 40, 45, 48))
def test_single_gaussian_pdfs_are_exact(engine, dim):
    C = _chunk(engine)
    rng = np.random.default_rng(9000 + dim)
    P = 37
    counts = np.concatenate([[0, 1, C - 1, C, C + 1, 2 * C + 1], rng.integers(0, 300, size=P - 6)])
    counts = counts[rng.permutation(P)]
    am = helpers.random_gmm(rng, dim, [1] * P)
    tm = helpers.fmllr_tm(P)
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    weights = rng.choice(np.array([1.0, 0.5], np.float32), size=2 * P + 1)
    feats = helpers.fmllr_draw(rng, am, pdfs)
    st = device_stats(engine, am, feats, ali, tm, weights)
    pdf, fw = R.frame_tables(tm, ali, weights)
    check_exact_tier(st, am, feats, pdf, fw, ali, 2 * P + 1, f"single Gaussians dim {dim}")
    assert (st.occ[counts == 0] == 0).all() and not st.mean_acc[counts == 0].any()


# ---- tier 2 ----------------------------------------------------------------------------------------------------------------
ONE_HOT_SIZES = [2, 5, 16, 17, 32, 33, 70, 128]


@functools.lru_cache(maxsize=None)
def one_hot_case(dim, C):
    rng = np.random.default_rng(9100 + dim)
    sizes = ONE_HOT_SIZES
    P = len(sizes)
    dev = np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=dim))
    gconsts, mi, iv, means, offs = [], [], [], [], [0]
    for n in sizes:
        w = rng.dirichlet(np.full(n, 2.0))
        step = rng.permutation(n)[:, None] * np.ones((1, dim))        # every Gaussian its own slot, the same in every coordinate
        mean = 40.0 * (step - (n - 1) / 2.0) * dev[None, :]
        var = np.tile(dev * dev, (n, 1))
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean / var).astype(np.float32)); iv.append((1.0 / var).astype(np.float32))
        means.append(mean); offs.append(offs[-1] + n)
    am = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    means = np.concatenate(means)
    counts = np.array([2 * C + 40, 300, 77, C + 1, 3 * C + 5, 150, 200, 2 * C + 1])     # multi-chunk pdfs of 2 … 128 Gaussians
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    gauss = np.array([rng.integers(offs[p], offs[p + 1]) for p in pdfs])
    feats = (means[gauss] + rng.uniform(-3.0, 3.0, size=(len(pdfs), dim)) * dev[None, :]).astype(np.float32)
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    weights = rng.choice(np.array([1.0, 0.5], np.float32), size=2 * P + 1)
    return am, helpers.fmllr_tm(P), feats, ali, weights, gauss


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_one_hot_mixtures_are_exact(engine, dim):
    am, tm, feats, ali, weights, gauss = one_hot_case(dim, _chunk(engine))
    pdf, fw = R.frame_tables(tm, ali, weights)
    _, post = gmm_statistics_host(am, feats, ali, tm, weights, want_post=True)
    # the condition that makes this tier exact, on every frame: all of w on the Gaussian the frame was drawn around
    local = gauss - am.pdf_offsets[pdf]
    expect = np.zeros_like(post)
    expect[np.arange(len(ali)), local] = fw
    assert np.array_equal(post, expect), "host twin: posteriors are not exactly one-hot"
    st = device_stats(engine, am, feats, ali, tm, weights)
    check_exact_tier(st, am, feats, gauss, fw, ali, len(weights), f"one-hot mixtures dim {dim}")


# ---- tier 3 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin(dim):
    case = R.skewed_case(dim)
    return case, gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)


@pytest.mark.parametrize("dim", gmm_ref.DIMS_SKEWED)
def test_soft_posteriors_against_the_host_twin(engine, dim):
    case, twin = _twin(dim)
    st = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights)
    ref = check_against_float64(case, st, f"device, {case.name}")
    T2 = 2.0 * ref["n_frames"] * U64
    worst = {}
    for name, got, want, S, t2 in (("occ", st.occ, twin.occ, ref["occ"], T2), ("mean", st.mean_acc, twin.mean_acc, ref["S_mean"], T2[:, None]),
                                   ("var", st.var_acc, twin.var_acc, ref["var"], T2[:, None])):
        err, lim = np.abs(got - want), (DEVICE_VS_TWIN * R.EPS32 + t2) * S
        worst[name] = float((err / np.where(S > 0, R.EPS32 * S, 1.0)).max())
        assert (err <= lim).all(), (case.name, name, worst[name])
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    took = pdf >= 0
    s_ll = ref["S_tot"]
    lim_ll = R.EPS32 * (s_ll + DEVICE_VS_TWIN_LL * float(fw[took].sum())) + 2 * took.sum() * U64 * s_ll
    worst["tot"] = abs(st.tot_like - twin.tot_like) / (R.EPS32 * s_ll)
    print(f"{case.name}: device - host twin in eps32*S: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert abs(st.tot_like - twin.tot_like) <= lim_ll, (case.name, worst)
    assert st.tot_count == twin.tot_count and np.array_equal(st.tid_count, twin.tid_count)


# ---- reproducibility and additivity -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_split_batch_adds_up(engine):
    case, _ = _twin(40)
    one = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights)
    again = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights, load=False)
    assert _bits(one) == _bits(again)
    cut = 1237
    half = device_stats(engine, case.am, case.feats[:cut], case.ali[:cut], case.tm, case.weights, load=False)
    both = device_stats(engine, case.am, case.feats[cut:], case.ali[cut:], case.tm, case.weights, into=half, load=False)
    assert both is half
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = R.gmm_acc(case.feats, pdf, fw, case.am)
    # the same posteriors (a frame's do not depend on its neighbours), summed in two associations: 2·T·2⁻⁵³·S
    T2 = 2.0 * ref["n_frames"] * U64
    assert (np.abs(both.occ - one.occ) <= T2 * ref["occ"]).all()
    assert (np.abs(both.mean_acc - one.mean_acc) <= T2[:, None] * ref["S_mean"]).all()
    assert (np.abs(both.var_acc - one.var_acc) <= T2[:, None] * ref["var"]).all()
    assert abs(both.tot_like - one.tot_like) <= 2 * len(pdf) * U64 * ref["S_tot"]
    assert both.tot_count == one.tot_count and np.array_equal(both.tid_count, one.tid_count)


def test_accumulators_are_added_to_and_odd_frames_leave_no_trace(engine):
    case, _ = _twin(39)
    rng = np.random.default_rng(77)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(rng.normal(size=G) * 100, rng.normal(size=(G, D)) * 100, rng.normal(size=(G, D)) * 100, -12.5, 40.0,
                     rng.integers(0, 1000, size=n_tids).astype(np.int64))
    plain = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights)
    added = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights, into=start.copy(), load=False)
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = R.gmm_acc(case.feats, pdf, fw, case.am)
    # start + (chunks) against (0 + chunks) + start: one more association over T + 1 addends
    for got, zero, first, S in ((added.occ, plain.occ, start.occ, ref["occ"]), (added.mean_acc, plain.mean_acc, start.mean_acc, ref["S_mean"]),
                                (added.var_acc, plain.var_acc, start.var_acc, ref["var"])):
        nf = ref["n_frames"].reshape((-1,) + (1,) * (S.ndim - 1))
        assert (np.abs(got - (zero + first)) <= 2.0 * (nf + 1) * U64 * (S + np.abs(first))).all()
    assert np.array_equal(added.tid_count, plain.tid_count + start.tid_count)
    assert added.tot_count == plain.tot_count + 40.0
    # Gaussians of pdfs without a frame keep the caller's bits
    idle = ref["n_frames"] == 0
    assert added.occ[idle].tobytes() == start.occ[idle].tobytes() and added.mean_acc[idle].tobytes() == start.mean_acc[idle].tobytes()
    # frames that take no part: id 0, ids outside the table (either side), an id of weight 0 — nothing moves, bit for bit
    odd = np.concatenate([np.zeros(300), np.full(300, n_tids), np.full(300, -7), np.full(300, 4)]).astype(np.int32)
    assert case.weights[4] == 0
    feats = np.full((len(odd), D), np.nan, np.float32)
    same = device_stats(engine, case.am, feats, odd, case.tm, case.weights, into=start.copy(), load=False)
    assert _bits(same) == _bits(start)
    keep = pdf >= 0
    only = device_stats(engine, case.am, case.feats[keep], case.ali[keep], case.tm, case.weights, load=False)
    assert _bits(only) == _bits(plain)


def test_empty_batch_and_no_counts(engine):
    case, _ = _twin(45)
    engine.load_gmm(case.am)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(np.ones(G), np.ones((G, D)), np.ones((G, D)), 1.0, 2.0, np.ones(n_tids, np.int64))
    st = gmm_statistics(engine, torch.zeros((0, D), device=engine.device), torch.zeros(0, dtype=torch.int32, device=engine.device),
                        case.tm, case.weights, into=start.copy())
    assert _bits(st) == _bits(start)
    # d_tid_count NULL: the same sums
    full = device_stats(engine, case.am, case.feats, case.ali, case.tm, case.weights, load=False)
    from montreal_forced_aligner_amd.engine import _ptr, tid_tables
    from montreal_forced_aligner_amd._lib import check
    id2pdf, w = tid_tables(case.tm, case.weights)
    occ = torch.zeros(G, dtype=torch.float64, device=engine.device)
    mean, var = torch.zeros((G, D), dtype=torch.float64, device=engine.device), torch.zeros((G, D), dtype=torch.float64, device=engine.device)
    tot = torch.zeros(2, dtype=torch.float64, device=engine.device)
    f, a, p, ww = _dev(engine, case.feats), _dev(engine, case.ali), _dev(engine, id2pdf), _dev(engine, w)
    check(engine.ctx, engine.lib.mfa_gmm_acc_batch(engine.ctx, _ptr(f), len(case.ali), _ptr(a), _ptr(p), _ptr(ww), n_tids, _ptr(occ),
                                                    _ptr(mean), _ptr(var), _ptr(tot), None), "mfa_gmm_acc_batch")
    assert occ.cpu().numpy().tobytes() == full.occ.tobytes() and mean.cpu().numpy().tobytes() == full.mean_acc.tobytes()
    assert var.cpu().numpy().tobytes() == full.var_acc.tobytes() and tot.cpu().numpy().tolist() == [full.tot_like, full.tot_count]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _small_call_is_right(engine):
    rng = np.random.default_rng(3)
    am = helpers.random_gmm(rng, 13, [1, 1, 1])
    pdfs = rng.integers(0, 3, size=50)
    feats, ali = helpers.fmllr_draw(rng, am, pdfs), (2 * pdfs + 1).astype(np.int32)
    st = device_stats(engine, am, feats, ali, helpers.fmllr_tm(3))
    check_exact_tier(st, am, feats, pdfs, np.ones(50, np.float32), ali, 7, "small call after a refusal")


def test_refusals_leave_a_message_and_a_usable_context(engine):
    from montreal_forced_aligner_amd.engine import AlignmentEngine
    rng = np.random.default_rng(4)
    fresh = AlignmentEngine(0)
    try:
        fresh.gmm = helpers.random_gmm(rng, 13, [1])          # the Python layer's own check is not what is tested here
        with pytest.raises(MfaHipError, match="mfa_load_gmm has not been called"):
            gmm_statistics(fresh, torch.zeros((4, 13), device=fresh.device), torch.ones(4, dtype=torch.int32, device=fresh.device),
                           helpers.fmllr_tm(1))
        _small_call_is_right(fresh)
    finally:
        fresh.close()
    big = helpers.random_gmm(rng, 13, [2, 129])
    with pytest.raises(MfaHipError, match="more than 128 Gaussians"):
        device_stats(engine, big, np.zeros((4, 13), np.float32), np.ones(4, np.int32), helpers.fmllr_tm(2))
    _small_call_is_right(engine)
    limit = int(engine.lib.mfa_gmm_acc_max_dim())
    assert limit >= 48
    wide = helpers.random_gmm(rng, limit + 1, [2, 3])
    with pytest.raises(MfaHipError, match="feature dim"):
        device_stats(engine, wide, np.zeros((4, limit + 1), np.float32), np.ones(4, np.int32), helpers.fmllr_tm(2))
    _small_call_is_right(engine)
