"""MLLT statistics (csrc/mllt_acc.hip, its host twin csrc/mllt_acc_host.cpp): the float64 restatement of the contract of
include/mfa_hip.h ("MLLT statistics"), a derived bound on what the float32 softmax may put between it and an implementation
of the contract, and the cases tests/test_mllt_cpu.py (host twin) and tests/test_gpu_mllt_acc.py (device) share.

The bound.  full[g][i][j] = Σ_t γ_tg · d_ti · d_tj with d = x − μ_g formed in float32 — one rounding, which the contract
prescribes, so the restatement forms the same float32 d and the d's carry no error at all.  What remains:

  posteriors       tests/gmm_acc_ref.py bounds an implementation's γ̂ against the float64 γ: |Δγ_tg| ≤ γ_tg·δ(t, g) + w·2⁻¹²⁵
                   with δ(t, g) = expm1(2 e_t) + u·(|d_g| + D̄_t + n + 12) (its docstring has every term: the chain's error e_t,
                   the rounded exponent, expf, the sum, 1/s and the two products).  The same formulas are evaluated here.
  products         γ̂·d_i is exact in double (24 + 24 bits), (γ̂·d_i)·d_j enters an fma: no rounding before the addition.  So a
                   term's error is Δγ_tg · |d_ti · d_tj| and nothing else.
  sums             the double accumulation of the T_p frames of the pdf, in two different orders (the restatement's and the
                   implementation's): each addition rounds a partial sum of magnitude at most S_ij = Σ_t γ_tg·|d_ti·d_tj| by
                   2⁻⁵³ relative, so 2·T_p·2⁻⁵³·S_ij.
  together         B_full[g][i][j] = Σ_t (γ_tg·δ(t, g) + w_t·2⁻¹²⁵)·|d_ti·d_tj| + 2·T_p·2⁻⁵³·S_ij.
occ and tot are the GMM statistics' and keep tests/gmm_acc_ref.py's bounds.  Nothing here is measured on the code under test.

Two implementations of the contract (device and twin) run the same float32 chain: they differ by expf / logf, the order of
the softmax sum and the order of the double sums only — tests/test_gpu_gmm_acc.py derives 13.5·ε32 per posterior for that,
and the same propagation through |d_i·d_j| gives (13.5·ε32 + 2·T_p·2⁻⁵³)·S_ij.

Exact cases.  ``integer_case``: integer features and means, inverse variances powers of two (so means_invvars / inv_vars is
the integer mean exactly), weights 1, one Gaussian per pdf (γ = 1 exactly): every term is an integer and every sum stays far
below 2⁵³ — any order of summation gives the same bits.  ``one_hot_case``: the construction of
tests/test_gpu_gmm_acc.one_hot_case (means 40 deviations apart in every coordinate, frames within 3 deviations of one
component: exactly one-hot posteriors) on a dyadic grid — deviations ½, 1 or 2, frames at multiples of 1/16 of a deviation,
weights 1 and ½ — so that every term γ·d_i·d_j is a multiple of 2⁻¹¹ below 2⁶ and the sums of tens of thousands of them are
exact in double.  That is what makes bit-equality between the device's chunked sums and the twin's running sum a fact of
the contract, where real-valued frames would only allow the summation bound."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.stats import gaussian_means
from tests import gmm_acc_ref as R
from tests import helpers

U32, U64, EPS32 = R.U32, R.U64, R.EPS32
DEVICE_VS_TWIN = 13.5          # ε32 per posterior between two implementations of the contract: tests/test_gpu_gmm_acc.py


def mllt_acc(feats, pdf, weight, am):
    """The MLLT statistics in float64, grouped by pdf, and the bound of the module docstring.  Returns a dict: occ [G], full
    [G, D, D], tot [2], S_full = Σ γ|d_i d_j|, B_full, n_frames [G], post [T, largest pdf]."""
    x32 = np.asarray(feats, np.float32)
    x_all = x32.astype(np.float64)
    T, D = x_all.shape
    pdf = np.asarray(pdf, np.int64)
    w_all = np.asarray(weight, np.float64)
    gc, mi, iv = (np.asarray(v, np.float64) for v in (am.gconsts, am.means_invvars, am.inv_vars))
    mu32 = gaussian_means(am)
    G = gc.shape[0]
    out = dict(occ=np.zeros(G), full=np.zeros((G, D, D)), S_full=np.zeros((G, D, D)), B_full=np.zeros((G, D, D)),
               n_frames=np.zeros(G, np.int64), post=np.zeros((T, int(np.diff(am.pdf_offsets).max()))))
    tot = np.zeros(2)
    live = (w_all != 0) & (pdf >= 0)
    for p in np.unique(pdf[live]):
        rows = np.nonzero(live & (pdf == p))[0]
        g0, g1 = int(am.pdf_offsets[p]), int(am.pdf_offsets[p + 1])
        n, Tp = g1 - g0, len(rows)
        x, w = x_all[rows], w_all[rows]
        x2 = x * x
        ll = gc[None, g0:g1] + x @ mi[g0:g1].T - 0.5 * x2 @ iv[g0:g1].T
        mag = np.abs(gc)[None, g0:g1] + np.abs(x) @ np.abs(mi[g0:g1]).T + 0.5 * x2 @ np.abs(iv[g0:g1]).T
        e = (2 * D + 1) * U32 * mag.max(axis=1)
        mx = ll.max(axis=1)
        d = ll - mx[:, None]
        ex = np.exp(d)
        s = ex.sum(axis=1)
        sm = ex / s[:, None]
        post = sm * w[:, None]
        dbar = (sm * np.abs(d)).sum(axis=1)
        delta = np.expm1(2 * e)[:, None] + U32 * (np.abs(d) + dbar[:, None] + n + 12)
        dpost = post * delta + w[:, None] * 2.0 ** -125
        out["post"][rows, :n] = post
        out["n_frames"][g0:g1] = Tp
        out["occ"][g0:g1] = post.sum(axis=0)
        for g in range(n):
            df = (x32[rows] - mu32[g0 + g][None, :]).astype(np.float64)         # the contract's float32 difference
            ad = np.abs(df)
            out["full"][g0 + g] = (post[:, g, None] * df).T @ df
            S = (post[:, g, None] * ad).T @ ad
            out["S_full"][g0 + g] = S
            out["B_full"][g0 + g] = (dpost[:, g, None] * ad).T @ ad + 2 * Tp * U64 * S
        tot += [(w * (mx + np.log(s))).sum(), w.sum()]
    out["tot"] = tot
    return out


def check_against_float64(case, st, what):
    """``st`` (host twin or device) against the restatement under its bound; occ and tot under tests/gmm_acc_ref.py's."""
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = mllt_acc(case.feats, pdf, fw, case.am)
    gref = R.gmm_acc(case.feats, pdf, fw, case.am)
    err = np.abs(st.full - ref["full"])
    assert np.isfinite(st.full).all(), what
    worst = float(np.max(err / np.where(ref["B_full"] > 0, ref["B_full"], 1.0)))
    print(f"{what}: worst |full - float64| / bound = {worst:.4f}; occ {np.max(np.abs(st.occ - gref['occ']) / np.where(gref['B_occ'] > 0, gref['B_occ'], 1.0)):.4f}")
    assert (err <= ref["B_full"]).all(), (what, worst)
    assert (np.abs(st.occ - gref["occ"]) <= gref["B_occ"]).all(), what
    assert abs(st.tot_like - gref["tot"][0]) <= gref["B_tot"], what
    assert st.tot_count == float(fw[pdf >= 0].astype(np.float64).sum()), what
    assert np.array_equal(st.full, np.swapaxes(st.full, 1, 2)), what
    return ref


# ---- exact cases ------------------------------------------------------------------------------------------------------------
def integer_case(dim, counts, seed=0) -> R.AccCase:
    """Single-Gaussian pdfs with ``counts[p]`` frames each, shuffled; integers throughout (module docstring)."""
    rng = np.random.default_rng(7000 + 31 * dim + seed)
    P = len(counts)
    mean = rng.integers(-4, 5, size=(P, dim)).astype(np.float64)
    iv = 2.0 ** rng.integers(-2, 3, size=(P, dim))
    gc = -0.5 * (dim * np.log(2 * np.pi) - np.log(iv).sum(axis=1) + (mean * mean * iv).sum(axis=1))
    am = M.DiagGmmModel(dim, gc.astype(np.float32), (mean * iv).astype(np.float32), iv.astype(np.float32),
                        np.arange(P + 1, dtype=np.int32))
    assert np.array_equal(gaussian_means(am), mean.astype(np.float32))
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    feats = rng.integers(-8, 9, size=(len(pdfs), dim)).astype(np.float32)
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    return R.AccCase(f"integers dim {dim}", am, helpers.fmllr_tm(P), feats, ali, np.ones(2 * P + 1, np.float32))


def integer_expect(case):
    """(occ, full) of an integer case in float64 numpy: exact whatever the order."""
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    mu = gaussian_means(case.am).astype(np.float64)
    P, D = case.am.num_gauss, case.am.dim
    occ, full = np.zeros(P), np.zeros((P, D, D))
    for p in range(P):
        d = case.feats[pdf == p].astype(np.float64) - mu[p]
        occ[p] = d.shape[0]
        full[p] = d.T @ d
    assert np.abs(full).max() < 2.0 ** 40
    return occ, full


ONE_HOT_SIZES = [1, 2, 5, 63, 64, 65, 128]


@lru_cache(maxsize=None)
def one_hot_case(dim, counts, sizes=None):
    """Pdfs of ``sizes`` Gaussians (a tuple; default ONE_HOT_SIZES) with ``counts`` frames; returns (case, gauss [T]: the
    Gaussian of every frame)."""
    rng = np.random.default_rng(9100 + dim)
    sizes = ONE_HOT_SIZES if sizes is None else list(sizes)
    P = len(sizes)
    assert len(counts) == P
    dev = 2.0 ** rng.integers(-1, 2, size=dim)
    gconsts, mi, iv, means, offs = [], [], [], [], [0]
    for n in sizes:
        w = rng.dirichlet(np.full(n, 2.0)) if n > 1 else np.ones(1)
        step = rng.permutation(n)[:, None] * np.ones((1, dim))
        mean = 40.0 * (step - (n - 1) / 2.0) * dev[None, :]
        var = np.tile(dev * dev, (n, 1))
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean / var).astype(np.float32)); iv.append((1.0 / var).astype(np.float32))
        means.append(mean); offs.append(offs[-1] + n)
    am = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    means = np.concatenate(means)
    assert np.array_equal(gaussian_means(am).astype(np.float64), means)            # dyadic: exact in float32
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    gauss = np.array([rng.integers(offs[p], offs[p + 1]) for p in pdfs])
    u = rng.integers(-48, 49, size=(len(pdfs), dim)) / 16.0
    feats64 = means[gauss] + u * dev[None, :]
    feats = feats64.astype(np.float32)
    assert np.array_equal(feats.astype(np.float64), feats64)
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    weights = rng.choice(np.array([1.0, 0.5], np.float32), size=2 * P + 1)
    return R.AccCase(f"one-hot dim {dim}", am, helpers.fmllr_tm(P), feats, ali, weights), gauss


def one_hot_expect(case, gauss):
    """(occ, full) of a one-hot case with all of a frame's weight on ``gauss[t]``: exact in float64 whatever the order."""
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    mu = gaussian_means(case.am).astype(np.float64)
    Gn, D = case.am.num_gauss, case.am.dim
    occ, full = np.zeros(Gn), np.zeros((Gn, D, D))
    took = pdf >= 0
    for g in np.unique(gauss[took]):
        rows = np.flatnonzero(took & (gauss == g))
        d = case.feats[rows].astype(np.float64) - mu[g]
        w = fw[rows].astype(np.float64)
        occ[g] = w.sum()
        full[g] = (w[:, None] * d).T @ d
    return occ, full


@lru_cache(maxsize=None)
def grouped_soft_case(dim) -> R.AccCase:
    """Soft posteriors at the Gaussian counts where the device kernel changes its path — 1, 2, 5, 63, 64, 65 and 128: one and
    two posterior rounds, one to eight groups of 16 Gaussians, a group of one —: a random model whose Gaussians overlap, every frame
    drawn from a Gaussian of its own pdf; the 128- and the 65-Gaussian pdf get 600 and 530 frames (two chunks of the occ / totals
    sums), weights 1, 0.5 and 0.3, some frames that take no part."""
    rng = np.random.default_rng(8300 + dim)
    sizes = ONE_HOT_SIZES
    P = len(sizes)
    gconsts, mi, iv, offs = [], [], [], [0]
    for n in sizes:                      # helpers.random_gmm with the means √(3 / dim) apart: neighbours overlap at every dim
        w = rng.dirichlet(np.ones(n)) if n > 1 else np.ones(1)
        mean = rng.normal(0, np.sqrt(3.0 / dim), size=(n, dim))
        var = rng.uniform(0.5, 4.0, size=(n, dim))
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean / var).astype(np.float32)); iv.append((1.0 / var).astype(np.float32))
        offs.append(offs[-1] + n)
    am = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    counts = [90, 120, 150, 200, 170, 530, 600]
    pdfs = rng.permutation(np.repeat(np.arange(P), counts))
    feats = helpers.fmllr_draw(rng, am, pdfs)
    n_tids = 2 * P + 1
    weights = rng.choice(np.array([1.0, 0.5, 0.3], np.float32), size=n_tids).astype(np.float32)
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    odd = rng.permutation(len(pdfs))[:60]
    ali[odd[:20]] = 0
    ali[odd[20:40]] = n_tids + rng.integers(0, 5, size=20)
    ali[odd[40:]] = -1 - rng.integers(0, 5, size=20)
    return R.AccCase(f"grouped soft dim {dim}", am, helpers.fmllr_tm(P), feats, ali, weights)
