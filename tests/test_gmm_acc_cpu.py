"""The host twin of the GMM statistics (mfa_debug_gmm_acc_host, csrc/gmm_acc_host.cpp over csrc/gmm_acc_math.hpp) without a
GPU: against the float64 restatement under the bound tests/gmm_acc_ref.py derives, the facts that need no reference at all,
and the twin's translation unit under the host sanitizers as a stand-alone program (nothing is preloaded anywhere)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd.engine import GmmStats, gmm_statistics_host
from tests import gmm_acc_ref as R
from tests import gmm_ref

ROOT = Path(__file__).resolve().parents[1]


def check_against_float64(case, st, what):
    """``st`` (host twin or device) against the restatement under its bound; prints the worst ratios."""
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    ref = R.gmm_acc(case.feats, pdf, fw, case.am)
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
    assert np.array_equal(st.tid_count, R.tid_counts(case.ali, pdf, len(case.weights))), what
    return ref


@pytest.mark.parametrize("dim", gmm_ref.DIMS_SKEWED)
def test_host_twin_against_float64(dim):
    case = R.skewed_case(dim)
    st = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    ref = check_against_float64(case, st, f"host twin, {case.name}")
    # Σ_g occ of a pdf = the summed weights of its frames: the posteriors of a frame sum to w within n roundings each
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    for p in range(case.am.num_pdfs):
        a, b = int(case.am.pdf_offsets[p]), int(case.am.pdf_offsets[p + 1])
        wsum = float(fw[pdf == p].astype(np.float64).sum())
        assert abs(st.occ[a:b].sum() - wsum) <= (b - a + 12) * R.U32 * wsum + 1e-300, p
    assert ref["n_frames"].max() >= 700


def test_frames_that_take_no_part_leave_no_trace():
    case = R.skewed_case(40)
    rng = np.random.default_rng(5)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    start = GmmStats(rng.normal(size=G), rng.normal(size=(G, D)), rng.normal(size=(G, D)), 3.25, 7.5,
                     rng.integers(0, 9, size=n_tids).astype(np.int64))
    ali = np.concatenate([np.zeros(50), np.full(50, n_tids), np.full(50, n_tids + 1000), np.full(50, -3), np.full(50, 4)]).astype(np.int32)
    assert case.weights[4] == 0
    feats = np.full((len(ali), D), np.nan, np.float32)          # never read
    st = gmm_statistics_host(case.am, feats, ali, case.tm, case.weights, into=start.copy())
    for a, b in ((st.occ, start.occ), (st.mean_acc, start.mean_acc), (st.var_acc, start.var_acc), (st.tid_count, start.tid_count)):
        assert a.tobytes() == b.tobytes()
    assert (st.tot_like, st.tot_count) == (3.25, 7.5)
    # and with real frames in between: the same bits as without the odd ones
    keep = R.frame_tables(case.tm, case.ali, case.weights)[0] >= 0
    full = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights, into=start.copy())
    only = gmm_statistics_host(case.am, case.feats[keep], case.ali[keep], case.tm, case.weights, into=start.copy())
    assert full.mean_acc.tobytes() == only.mean_acc.tobytes() and full.occ.tobytes() == only.occ.tobytes()
    assert full.var_acc.tobytes() == only.var_acc.tobytes() and (full.tot_like, full.tot_count) == (only.tot_like, only.tot_count)
    assert np.array_equal(full.tid_count, only.tid_count)


def test_twin_refuses_what_the_contract_excludes():
    lib = _lib.lib()
    from tests import helpers
    am = helpers.random_gmm(np.random.default_rng(1), 5, [129])
    st = GmmStats.zeros(129, 5, 3)
    with pytest.raises(_lib.MfaHipError, match="128"):
        gmm_statistics_host(am, np.zeros((1, 5), np.float32), np.array([1], np.int32), helpers.fmllr_tm(1), into=st)
    assert lib.mfa_debug_gmm_acc_host(0, 0, None, None, None, None, None, 0, None, None, None, 0, None, None, None, None, None, None, 0) == -1
    assert lib.mfa_gmm_acc_chunk_frames() >= 64 and lib.mfa_gmm_acc_max_dim() >= 48


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "gmm_acc_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "gmm_acc_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "gmm_acc_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout
