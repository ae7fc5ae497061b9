"""The bound of tests/gmm_ref.py on the reference side, without a GPU: on every model, utterance and pdf list the GPU tests of
tests/test_gpu_gmm_shapes.py score, the project's C++ oracle (float32 fmaf chain, Kaldi's log-sum-exp with its cutoff) lies
within B of the float64 reference — far inside, so the bound is left for the kernels' own arithmetic — and the skewed
models really are skewed."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import gmm_ref as R
from tests.test_gmm_pack_cpu import _pack


def _ratio(am, feats, pdf_list):
    ref = R.ref64(feats, am, pdf_list)
    orc = O.gmm_loglikes(feats, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pdf_list)
    assert np.isfinite(ref).all() and np.isfinite(orc).all()
    return float((np.abs(orc.astype(np.float64) - ref) / R.bound(feats, am, pdf_list, ref)).max()), float(np.abs(ref).max())


@pytest.mark.parametrize("case", R.all_cases(), ids=lambda c: c.name.replace(" ", "-"))
def test_oracle_within_bound_of_float64(case):
    worst, big = 0.0, 0.0
    for x, pl in zip(case.feats, R.sorted_lists(case.am, case.lists)):
        r, m = _ratio(case.am, x, pl)
        worst, big = max(worst, r), max(big, m)
    print(f"{case.name}: worst |oracle - ref64| / B = {worst:.4f}, max |LL| = {big:.4g}")
    assert worst <= 1.0


def test_oracle_within_bound_wide_models(fx):
    rng = np.random.default_rng(1)
    for am in R.wide_models(fx.mono_tm.num_pdfs):
        x = rng.normal(0, 3, size=(100, am.dim)).astype(np.float32)
        worst, big = _ratio(am, x, np.arange(am.num_pdfs, dtype=np.int32))
        print(f"wide dim {am.dim}, {int(np.diff(am.pdf_offsets).max())} Gaussians at most: worst / B = {worst:.4f}, max |LL| = {big:.4g}")
        assert worst <= 1.0


def test_oracle_within_bound_at_the_f16_range_edge():
    case = R.range_case()
    fscale, dim = _pack(case.am)["fscale"], case.am.dim
    for name, k, target, declined in R.RANGE_VARIANTS:
        feats = R.range_feats(case, fscale, k, target)
        x = feats[0]
        xt = np.zeros(len(fscale), np.float32)
        xt[:dim], xt[dim: 2 * dim] = x[300], x[300] * x[300]
        sv = xt * fscale                                                  # float32, as split_features forms it
        # the moved value lands where it was aimed, and the kernels' range test on this frame says what the variant expects
        assert abs(float(sv[k]) - target) < 5.0 and (float(abs(sv[k])) <= 65000.0) == (target < 65000.0)
        assert bool((np.abs(sv) > 65000.0).any()) == declined
        others = np.delete(np.arange(len(x)), 300)
        assert np.abs(np.concatenate([x[others], x[others] ** 2], axis=1) * fscale[None, : 2 * dim]).max() < 30000.0
        worst, big = _ratio(case.am, x, R.sorted_lists(case.am, case.lists)[0])
        print(f"{name}: scaled operand {float(sv[k]):.1f}, largest {float(np.abs(sv).max()):.4g}, worst / B = {worst:.4f}, max |LL| = {big:.4g}")
        assert worst <= 1.0


@pytest.mark.parametrize("dim", R.DIMS_SKEWED)
def test_skewed_models_are_skewed(dim):
    case = R.skewed_case(dim)
    sk, am = case.sk, case.am
    iv = am.inv_vars.astype(np.float64)
    spread = iv.max(axis=0).max() / iv.min(axis=0).min()
    col = iv.mean(axis=0)
    assert col.max() / col.min() >= 1e6, col.max() / col.min()           # per-column inv_var spread
    # a component under Kaldi's cutoff in some cell: its log-likelihood more than −ln ε below the pdf's best
    x = np.concatenate(case.feats).astype(np.float64)
    ll = am.gconsts.astype(np.float64)[None, :] + x @ am.means_invvars.T.astype(np.float64) - 0.5 * (x * x) @ iv.T
    cutoff = np.log(np.finfo(np.float32).eps)
    under = forced_under = 0
    for p in range(am.num_pdfs):
        a, b = am.pdf_offsets[p], am.pdf_offsets[p + 1]
        below = ll[:, a:b] < ll[:, a:b].max(axis=1, keepdims=True) + cutoff
        under += int(below.sum())
        forced_under += int(below[:, sk.forced[a:b]].sum())
    assert under > 0 and forced_under > 0
    # the duplicated components are there, bit for bit, and tie the maximum somewhere
    assert len(sk.dup) == sum(1 for g in R.SIZES_SKEWED if g >= 4)
    ties = 0
    for a, b in sk.dup:
        assert am.gconsts[a] == am.gconsts[b] and np.array_equal(am.means_invvars[a], am.means_invvars[b])
        assert np.array_equal(am.inv_vars[a], am.inv_vars[b])
        p = int(np.searchsorted(am.pdf_offsets, a, side="right") - 1)
        g0, g1 = am.pdf_offsets[p], am.pdf_offsets[p + 1]
        ties += int((ll[:, a] == ll[:, g0:g1].max(axis=1)).sum())
    assert ties > 0
    print(f"skewed dim {dim}: inv_var spread {spread:.3g} (column means {col.max() / col.min():.3g}), {under} component cells under "
          f"the cutoff ({forced_under} of the forced weights), {ties} cells whose maximum is the duplicated pair")
