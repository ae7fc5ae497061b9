"""The two-feature host twin of the GMM statistics (mfa_debug_gmm_acc_twofeats_host, csrc/gmm_acc_host.cpp) without a GPU:
against the float64 restatement under the bound tests/gmm_acc2_ref.py restates, the facts that need no reference at all
(equal matrices, swapped matrices, frames that take no part, adding up, refusals), and the twin's translation unit under
the host sanitizers as a stand-alone program (nothing is preloaded anywhere)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd.engine import GmmStats, gmm_statistics_host, gmm_statistics_twofeats_host
from tests import gmm_acc2_ref as R2
from tests import gmm_ref, helpers

ROOT = Path(__file__).resolve().parents[1]


def _same_bits(a, b):
    return (a.occ.tobytes() == b.occ.tobytes() and a.mean_acc.tobytes() == b.mean_acc.tobytes() and a.var_acc.tobytes() == b.var_acc.tobytes()
            and (a.tot_like, a.tot_count) == (b.tot_like, b.tot_count) and np.array_equal(a.tid_count, b.tid_count))


def check_against_float64(case, st, what):
    """``st`` (two-feature host twin or device) against the two-matrix restatement under its bound; prints the worst ratios."""
    pdf, fw = R2.frame_tables(case.tm, case.ali, case.weights)
    ref = R2.gmm_acc2(case.feats, case.feats_sum, pdf, fw, case.am)
    worst = {}
    for name, got, want, bound in (("occ", st.occ, ref["occ"], ref["B_occ"]), ("mean", st.mean_acc, ref["mean"], ref["B_mean"]),
                                   ("var", st.var_acc, ref["var"], ref["B_var"])):
        err = np.abs(got - want)
        assert np.isfinite(got).all(), (what, name)
        worst[name] = float(np.max(err / np.where(bound > 0, bound, 1.0)))
        assert (err <= bound).all(), (what, name, worst[name])
    worst["tot"] = abs(st.tot_like - ref["tot"][0]) / ref["B_tot"]
    print(f"{what}: |got - float64| / bound: " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert abs(st.tot_like - ref["tot"][0]) <= ref["B_tot"], (what, worst)
    assert st.tot_count == float(fw[pdf >= 0].astype(np.float64).sum()), what          # Σ w: exact
    assert np.array_equal(st.tid_count, R2.tid_counts(case.ali, pdf, len(case.weights))), what
    return ref


@pytest.mark.parametrize("dim", gmm_ref.DIMS_SKEWED)
def test_host_twin_against_float64(dim):
    case = R2.skewed_case2(dim)
    assert (case.feats != case.feats_sum).all()
    st = gmm_statistics_twofeats_host(case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights)
    ref = check_against_float64(case, st, f"host twin, {case.name}")
    assert ref["n_frames"].max() >= 700


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_equal_matrices_give_the_one_feature_twin(dim):
    case = R2.skewed_case2(dim)
    one = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    assert _same_bits(gmm_statistics_twofeats_host(case.am, case.feats, case.feats.copy(), case.ali, case.tm, case.weights), one)
    assert _same_bits(gmm_statistics_twofeats_host(case.am, case.feats, case.feats, case.ali, case.tm, case.weights), one)


def test_swapping_the_matrices_is_detected_and_the_totals_follow_the_posterior_side():
    case = R2.skewed_case2(40)
    st, post = gmm_statistics_twofeats_host(case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights, want_post=True)
    swapped = gmm_statistics_twofeats_host(case.am, case.feats_sum, case.feats, case.ali, case.tm, case.weights)
    live = st.occ > 0
    assert live.any() and (st.mean_acc[live] != swapped.mean_acc[live]).any(axis=1).all()
    for first, second in ((case.feats, case.feats_sum), (case.feats_sum, case.feats)):
        two = gmm_statistics_twofeats_host(case.am, first, second, case.ali, case.tm, case.weights)
        one, post1 = gmm_statistics_host(case.am, first, case.ali, case.tm, case.weights, want_post=True)
        assert (two.tot_like, two.tot_count) == (one.tot_like, one.tot_count)
        assert two.occ.tobytes() == one.occ.tobytes() and np.array_equal(two.tid_count, one.tid_count)
        if first is case.feats:
            assert np.array_equal(post, post1)
    # and the sums are the posteriors of the first matrix over the rows of the second, in frame order
    g = int(np.argmax(st.occ))
    p = int(np.searchsorted(case.am.pdf_offsets, g, side="right") - 1)
    pdf, _ = R2.frame_tables(case.tm, case.ali, case.weights)
    rows = np.flatnonzero(pdf == p)
    gamma = post[rows, g - int(case.am.pdf_offsets[p])].astype(np.float64)
    want = (gamma[:, None] * case.feats_sum[rows].astype(np.float64)).sum(axis=0)
    S = (gamma[:, None] * np.abs(case.feats_sum[rows].astype(np.float64))).sum(axis=0)
    assert (np.abs(st.mean_acc[g] - want) <= 2 * len(rows) * R2.U64 * S).all()


def test_frames_that_take_no_part_leave_no_trace():
    case = R2.skewed_case2(40)
    rng = np.random.default_rng(5)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(rng.normal(size=G), rng.normal(size=(G, D)), rng.normal(size=(G, D)), 3.25, 7.5,
                     rng.integers(0, 9, size=n_tids).astype(np.int64))
    ali = np.concatenate([np.zeros(50), np.full(50, n_tids), np.full(50, n_tids + 1000), np.full(50, -3), np.full(50, 4)]).astype(np.int32)
    assert case.weights[4] == 0
    nan = np.full((len(ali), D), np.nan, np.float32)          # never read, either of them
    st = gmm_statistics_twofeats_host(case.am, nan, nan.copy(), ali, case.tm, case.weights, into=start.copy())
    assert _same_bits(st, start)
    keep = R2.frame_tables(case.tm, case.ali, case.weights)[0] >= 0
    full = gmm_statistics_twofeats_host(case.am, case.feats, case.feats_sum, case.ali, case.tm, case.weights, into=start.copy())
    only = gmm_statistics_twofeats_host(case.am, case.feats[keep], case.feats_sum[keep], case.ali[keep], case.tm, case.weights, into=start.copy())
    assert _same_bits(full, only)


def test_into_and_iadd_add_up():
    case = R2.skewed_case2(39)
    args = (case.tm, case.weights)
    whole = gmm_statistics_twofeats_host(case.am, case.feats, case.feats_sum, case.ali, *args)
    cut = 1237
    head = gmm_statistics_twofeats_host(case.am, case.feats[:cut], case.feats_sum[:cut], case.ali[:cut], *args)
    chained = gmm_statistics_twofeats_host(case.am, case.feats[cut:], case.feats_sum[cut:], case.ali[cut:], *args, into=head.copy())
    # the twin sums in frame order from the caller's values: a chain over two calls is the one call, bit for bit
    assert _same_bits(chained, whole)
    tail = gmm_statistics_twofeats_host(case.am, case.feats[cut:], case.feats_sum[cut:], case.ali[cut:], *args)
    added = head.copy()
    added += tail
    pdf, fw = R2.frame_tables(case.tm, case.ali, case.weights)
    ref = R2.gmm_acc2(case.feats, case.feats_sum, pdf, fw, case.am)
    T2 = 2.0 * ref["n_frames"] * R2.U64                 # the same addends in another association
    assert (np.abs(added.occ - whole.occ) <= T2 * ref["occ"]).all()
    assert (np.abs(added.mean_acc - whole.mean_acc) <= T2[:, None] * ref["S_mean"]).all()
    assert (np.abs(added.var_acc - whole.var_acc) <= T2[:, None] * ref["var"]).all()
    assert abs(added.tot_like - whole.tot_like) <= 2 * len(pdf) * R2.U64 * ref["S_tot"]
    assert added.tot_count == whole.tot_count and np.array_equal(added.tid_count, whole.tid_count)


def test_twin_refuses_what_the_contract_excludes():
    lib = _lib.lib()
    am = helpers.random_gmm(np.random.default_rng(1), 5, [129])
    st = GmmStats.zeros(129, 5, 3)
    x = np.zeros((1, 5), np.float32)
    with pytest.raises(_lib.MfaHipError, match="128"):          # −2
        gmm_statistics_twofeats_host(am, x, x.copy(), np.array([1], np.int32), helpers.fmllr_tm(1), into=st)
    assert lib.mfa_debug_gmm_acc_twofeats_host(0, 0, None, None, None, None, None, None, 0, None, None, None, 0, None, None, None, None,
                                               None, None, 0) == -1
    # a NULL second matrix with frames: −1, and nothing written; without frames it is not looked at
    am = helpers.random_gmm(np.random.default_rng(2), 5, [2, 3])
    from montreal_forced_aligner_amd.engine import model_arrays
    po, gc, mi, iv = model_arrays(am)
    pdf, w = np.zeros(1, np.int32), np.ones(1, np.float32)
    occ, mean, var, tot = np.zeros(5), np.zeros((5, 5)), np.zeros((5, 5)), np.zeros(2)
    head = (5, 2, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data)
    tail = (occ.ctypes.data, mean.ctypes.data, var.ctypes.data, tot.ctypes.data, None, None, 0)
    assert lib.mfa_debug_gmm_acc_twofeats_host(*head, x.ctypes.data, None, 1, pdf.ctypes.data, w.ctypes.data, None, 0, *tail) == -1
    assert not occ.any() and not tot.any()
    assert lib.mfa_debug_gmm_acc_twofeats_host(*head, None, None, 0, None, None, None, 0, *tail) == 0
    assert lib.mfa_debug_gmm_acc_twofeats_host(*head, x.ctypes.data, x.ctypes.data, 1, pdf.ctypes.data, w.ctypes.data, None, 0, *tail) == 0
    assert tot[1] == 1.0
    with pytest.raises(_lib.MfaHipError, match="shape"):
        gmm_statistics_twofeats_host(am, np.zeros((2, 5), np.float32), np.zeros((3, 5), np.float32), np.ones(2, np.int32), helpers.fmllr_tm(2))
    with pytest.raises(_lib.MfaHipError, match="no matrix"):
        gmm_statistics_twofeats_host(am, np.zeros((2, 5), np.float32), None, np.ones(2, np.int32), helpers.fmllr_tm(2))


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "gmm_acc2_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "gmm_acc2_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "gmm_acc_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout
