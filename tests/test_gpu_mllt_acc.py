"""MLLT statistics on the device (csrc/mllt_acc.hip: the lookup, the ordering by pdf, mllt_acc_kernel with its posterior and
moment phases, and the reductions) against the host twin and the float64 restatement of tests/mllt_ref.py, in its tiers:

1. Integer single-Gaussian pdfs (γ = 1, every term an integer): device, twin and numpy are bit-equal.  Per-pdf frame counts
   0, 1, C − 1, C, C + 1 and 2C + 1 with C = mfa_mllt_acc_chunk_frames(): none, one, two and three units of a pdf.
2. One-hot mixtures on a dyadic grid (tests/mllt_ref.one_hot_case: every sum exact) of 1, 2, 5, 63, 64, 65 and 128
   Gaussians — one and two posterior rounds, one to eight Gaussian groups of the moment phase, a group of a single Gaussian —
   with pdfs of more than one and more than two units: bit-equal to the twin.
3. Soft posteriors: under the derived bound against the restatement, and against the twin under the two-implementations
   bound (13.5·ε32 per posterior, tests/test_gpu_gmm_acc.py's derivation, propagated through |d_i·d_j|, plus the double sums').
occ and tot are held to mfa_gmm_acc_batch's bits on the same input.  Key counts (hundreds and thousands of pdfs) and pdfs of
eight units and more are in tests/test_gpu_stats_scale.py."""
import functools

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError, _ptr, check
from montreal_forced_aligner_amd.stats import (MlltStats, gaussian_means, gmm_statistics, mllt_statistics, mllt_statistics_host,
                                               tid_tables)
from tests import gmm_acc_ref as R
from tests import gmm_ref, helpers
from tests import mllt_ref as MR

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def device_stats(engine, case, into=None, load=True, rows=slice(None)):
    if load:
        engine.load_gmm(case.am)
    return mllt_statistics(engine, _dev(engine, case.feats[rows]), _dev(engine, case.ali[rows]), case.tm, case.weights, into=into)


def host(case):
    return mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)


def _bits(st):
    return st.occ.tobytes() + st.full.tobytes() + np.array([st.tot_like, st.tot_count]).tobytes()


def _chunk(engine):
    return int(engine.lib.mfa_mllt_acc_chunk_frames())


def same_occ_and_tot_as_the_gmm_statistics(engine, case, st):
    g = gmm_statistics(engine, _dev(engine, case.feats), _dev(engine, case.ali), case.tm, case.weights)
    assert st.occ.tobytes() == g.occ.tobytes(), case.name
    assert (st.tot_like, st.tot_count) == (g.tot_like, g.tot_count), case.name


# ---- tier 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (13, 16, 17, 40, 48))
def test_integer_single_gaussian_pdfs_are_bit_equal(engine, dim):
    C = _chunk(engine)
    case = MR.integer_case(dim, [0, 1, C - 1, C, C + 1, 2 * C + 1, 7, 130, 0, 600])
    st = device_stats(engine, case)
    occ, full = MR.integer_expect(case)
    assert st.occ.tobytes() == occ.tobytes() and st.full.tobytes() == full.tobytes()
    twin = host(case)
    assert st.full.tobytes() == twin.full.tobytes() and st.occ.tobytes() == twin.occ.tobytes() and st.tot_count == twin.tot_count
    assert not st.full[0].any() and not st.full[8].any()
    same_occ_and_tot_as_the_gmm_statistics(engine, case, st)


# ---- tier 2 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_hot(dim, C):
    # by MR.ONE_HOT_SIZES = 1, 2, 5, 63, 64, 65, 128 Gaussians: the 5-Gaussian pdf has three units, the 128-Gaussian pdf two
    case, gauss = MR.one_hot_case(dim, (300, 77, 2 * C + 1, 150, 300, 200, C + 1))
    st, post = mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights, want_post=True)
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    expect = np.zeros_like(post)
    expect[np.arange(len(gauss)), gauss - case.am.pdf_offsets[pdf]] = fw
    assert np.array_equal(post, expect), "host twin: posteriors are not exactly one-hot"
    return case, gauss, st


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_one_hot_mixtures_are_bit_equal(engine, dim):
    case, gauss, twin = _one_hot(dim, _chunk(engine))
    st = device_stats(engine, case)
    occ, full = MR.one_hot_expect(case, gauss)
    assert st.occ.tobytes() == twin.occ.tobytes() == occ.tobytes()
    assert st.full.tobytes() == twin.full.tobytes() == full.tobytes()
    assert st.tot_count == twin.tot_count
    same_occ_and_tot_as_the_gmm_statistics(engine, case, st)          # tot over several chunks of the GMM statistics' length


# ---- tier 3 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soft(kind, dim):
    case = R.skewed_case(dim) if kind == "skewed" else MR.grouped_soft_case(dim)
    return case, host(case)


@pytest.mark.parametrize("kind,dim", [("skewed", d) for d in gmm_ref.DIMS_SKEWED] + [("grouped", 13), ("grouped", 40), ("grouped", 48)])
def test_soft_posteriors_against_the_twin_and_the_restatement(engine, kind, dim):
    case, twin = _soft(kind, dim)
    st = device_stats(engine, case)
    ref = MR.check_against_float64(case, st, f"device, {case.name}")
    MR.check_against_float64(case, twin, f"host twin, {case.name}")
    T2 = (2.0 * ref["n_frames"] * U64)[:, None, None]
    err, lim = np.abs(st.full - twin.full), (MR.DEVICE_VS_TWIN * R.EPS32 + T2) * ref["S_full"]
    worst = float((err / np.where(ref["S_full"] > 0, R.EPS32 * ref["S_full"], 1.0)).max())
    print(f"{case.name}: device - host twin in eps32*S: full {worst:.3f}")
    assert (err <= lim).all(), (case.name, worst)
    assert st.tot_count == twin.tot_count
    same_occ_and_tot_as_the_gmm_statistics(engine, case, st)


# ---- reproducibility and additivity -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_a_split_batch_adds_up(engine):
    case, _ = _soft("grouped", 40)
    one = device_stats(engine, case)
    again = device_stats(engine, case, load=False)
    assert _bits(one) == _bits(again)
    cut = 937
    half = device_stats(engine, case, load=False, rows=slice(0, cut))
    both = device_stats(engine, case, into=half, load=False, rows=slice(cut, None))
    assert both is half
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = MR.mllt_acc(case.feats, pdf, fw, case.am)
    # the same posteriors (a frame's do not depend on its neighbours), summed in two associations: 2·T·2⁻⁵³·S
    T2 = 2.0 * ref["n_frames"] * U64
    assert (np.abs(both.full - one.full) <= T2[:, None, None] * ref["S_full"]).all()
    assert (np.abs(both.occ - one.occ) <= T2 * ref["occ"]).all() and both.tot_count == one.tot_count
    assert np.array_equal(both.full, np.swapaxes(both.full, 1, 2))
    # on exact sums a split batch is bit-equal
    case, _gauss, twin = _one_hot(13, _chunk(engine))
    half = device_stats(engine, case, rows=slice(0, 5000))
    both = device_stats(engine, case, into=half, load=False, rows=slice(5000, None))
    assert both.full.tobytes() == twin.full.tobytes() and both.occ.tobytes() == twin.occ.tobytes()


def test_accumulators_are_added_to_and_odd_frames_leave_no_trace(engine):
    case, _ = _soft("grouped", 13)
    rng = np.random.default_rng(77)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    sym = rng.normal(size=(G, D, D)) * 100
    start = MlltStats(rng.normal(size=G) * 100, sym + np.swapaxes(sym, 1, 2), -12.5, 40.0)
    plain = device_stats(engine, case)
    added = device_stats(engine, case, into=start.copy(), load=False)
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = MR.mllt_acc(case.feats, pdf, fw, case.am)
    nf = ref["n_frames"]
    # start + (chunks) against (0 + chunks) + start: one more association over T + 1 addends
    assert (np.abs(added.full - (plain.full + start.full)) <= (2.0 * (nf + 1) * U64)[:, None, None] * (ref["S_full"] + np.abs(start.full))).all()
    assert (np.abs(added.occ - (plain.occ + start.occ)) <= 2.0 * (nf + 1) * U64 * (ref["occ"] + np.abs(start.occ))).all()
    assert added.tot_count == plain.tot_count + 40.0
    assert np.array_equal(added.full, np.swapaxes(added.full, 1, 2))
    # frames that take no part: id 0, ids outside the table (either side), an id of weight 0 — nothing moves, bit for bit
    zero_w = case.weights.copy()
    zero_w[4] = 0.0
    odd = np.concatenate([np.zeros(300), np.full(300, n_tids), np.full(300, -7), np.full(300, 4)]).astype(np.int32)
    feats = np.full((len(odd), D), np.nan, np.float32)
    same = mllt_statistics(engine, _dev(engine, feats), _dev(engine, odd), case.tm, zero_w, into=start.copy())
    assert _bits(same) == _bits(start)
    keep = pdf >= 0
    only = mllt_statistics(engine, _dev(engine, case.feats[keep]), _dev(engine, case.ali[keep]), case.tm, case.weights)
    assert _bits(only) == _bits(plain)
    # a pdf without a frame keeps the caller's bits, both triangles
    first = pdf != 1
    part = mllt_statistics(engine, _dev(engine, case.feats[first]), _dev(engine, case.ali[first]), case.tm, case.weights, into=start.copy())
    a, b = int(case.am.pdf_offsets[1]), int(case.am.pdf_offsets[2])
    assert part.full[a:b].tobytes() == start.full[a:b].tobytes() and part.occ[a:b].tobytes() == start.occ[a:b].tobytes()
    # an empty batch writes nothing
    none = mllt_statistics(engine, torch.zeros((0, D), device=engine.device), torch.zeros(0, dtype=torch.int32, device=engine.device),
                           case.tm, case.weights, into=start.copy())
    assert _bits(none) == _bits(start)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _small_call_is_right(engine):
    case = MR.integer_case(13, [20, 0, 30], seed=5)
    st = device_stats(engine, case)
    occ, full = MR.integer_expect(case)
    assert st.occ.tobytes() == occ.tobytes() and st.full.tobytes() == full.tobytes()


def test_refusals_leave_a_message_and_a_usable_context(engine):
    from montreal_forced_aligner_amd.engine import AlignmentEngine
    rng = np.random.default_rng(4)
    ones = lambda am, n=4: R.AccCase("refused", am, helpers.fmllr_tm(am.num_pdfs), np.zeros((n, am.dim), np.float32),
                                     np.ones(n, np.int32), np.ones(2 * am.num_pdfs + 1, np.float32))
    fresh = AlignmentEngine(0)
    try:
        fresh.gmm = helpers.random_gmm(rng, 13, [1])          # the Python layer's own check is not what is tested here
        with pytest.raises(MfaHipError, match="mfa_load_gmm has not been called"):
            device_stats(fresh, ones(fresh.gmm), load=False)
        _small_call_is_right(fresh)
    finally:
        fresh.close()
    with pytest.raises(MfaHipError, match="more than 128 Gaussians"):
        device_stats(engine, ones(helpers.random_gmm(rng, 13, [2, 129])))
    _small_call_is_right(engine)
    limit = int(engine.lib.mfa_mllt_acc_max_dim())
    assert limit == 48
    with pytest.raises(MfaHipError, match="feature dim"):
        device_stats(engine, ones(helpers.random_gmm(rng, limit + 1, [2, 3])))
    _small_call_is_right(engine)
    # NULL arrays and 2^31 frames: refused before anything is read
    case = ones(helpers.random_gmm(rng, 13, [2, 3]))
    engine.load_gmm(case.am)
    id2pdf, w = tid_tables(case.tm, case.weights)
    f, a, p, ww = _dev(engine, case.feats), _dev(engine, case.ali), _dev(engine, id2pdf), _dev(engine, w)
    mu = _dev(engine, gaussian_means(case.am))
    occ = torch.zeros(5, dtype=torch.float64, device=engine.device)
    full = torch.zeros((5, 13, 13), dtype=torch.float64, device=engine.device)
    tot = torch.zeros(2, dtype=torch.float64, device=engine.device)
    call = lambda n, *ptrs: engine.lib.mfa_mllt_acc_batch(engine.ctx, ptrs[0], n, ptrs[1], ptrs[2], ptrs[3], len(w), *ptrs[4:])
    good = [_ptr(f), _ptr(a), _ptr(p), _ptr(ww), _ptr(mu), _ptr(occ), _ptr(full), _ptr(tot)]
    for k in range(8):
        with pytest.raises(MfaHipError, match="NULL"):
            check(engine.ctx, call(4, *[None if i == k else v for i, v in enumerate(good)]), "mfa_mllt_acc_batch")
    with pytest.raises(MfaHipError, match="frames in one call"):
        check(engine.ctx, call(2 ** 31, *good), "mfa_mllt_acc_batch")
    torch.cuda.synchronize()
    assert not occ.any() and not full.any() and not tot.any()
    _small_call_is_right(engine)
