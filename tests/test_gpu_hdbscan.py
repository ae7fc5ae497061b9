"""The HDBSCAN stage on the device against its host twins: core scores and spanning-tree edges bit for bit on integer vectors
across the shapes at which the sweep changes path; on random data the stored scores are bit-symmetric and the twins, run on
that stored matrix, give the device's core scores and tree exactly; forced column passes and repeated runs give the same bits;
the round count; the path in random order; a NaN row; two far blobs; the refusals."""
import math

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import stats
from tests import hdbscan_ref as R

pytestmark = pytest.mark.gpu


def device_tree(engine, metric, x, k, model=None, want_v=False):
    pf = stats.core_scores(engine, metric, x, k, model, want_v=want_v)
    t = stats.mreach_mst(engine, metric if metric != "cosine" else "euclidean", pf["y"], pf["q"], pf["core"])
    return pf, t


def same_tree(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("lo", "hi", "score")) and a["found"] == b["found"]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130, 300])
def test_exact_tier_equals_the_twin_bit_for_bit(engine, n):
    for D in (1, 3, 4, 5, 50):
        x = R.integer_points(n, D, 1000 * n + D)
        for metric in ("euclidean", "dot"):
            for k in (0, 1, 4, 64):
                pf, t = device_tree(engine, metric, x, k)
                host = stats.core_scores_host(metric, x, k)
                assert np.array_equal(pf["y"].cpu().numpy(), host["y"]) and np.array_equal(pf["q"].cpu().numpy(), host["q"]), (D, metric, k)
                assert np.array_equal(pf["core"].cpu().numpy(), host["core"]), (D, metric, k)
                assert same_tree(t, stats.mreach_mst_host(metric, host["y"], host["q"], host["core"])), (D, metric, k)
                assert t["rounds"] <= (math.ceil(math.log2(n)) + 1 if n > 1 else 0)


@pytest.mark.parametrize("name", ["grid", "all_equal"])
def test_tie_rules_on_the_device(engine, name):
    x = {"grid": R.grid(12), "all_equal": R.all_equal(150)}[name]
    for k in (0, 4):
        pf, t = device_tree(engine, "euclidean", x, k)
        host = stats.core_scores_host("euclidean", x, k)
        assert np.array_equal(pf["core"].cpu().numpy(), host["core"])
        assert same_tree(t, stats.mreach_mst_host("euclidean", host["y"], host["q"], host["core"]))


@pytest.mark.parametrize("metric", ["plda", "euclidean", "dot"])
def test_random_data_symmetry_and_the_twins_on_the_stored_matrix(engine, metric):
    rng = np.random.default_rng(41)
    n, D = 300, 50
    x = rng.standard_normal((n, D)) + rng.integers(0, 4, (n, 1)) * 2.0
    model = R.model(D, 5)
    for k in (4, 17):
        pf, t = device_tree(engine, metric, x, k, model, want_v=True)
        v = pf["v"].cpu().numpy()
        assert np.isfinite(v).all() and np.array_equal(v, v.T)                  # the symmetry claim on the hardware
        y, q, core = (pf[key].cpu().numpy() for key in ("y", "q", "core"))
        host = stats.core_scores_host(metric, x, k, model, v=v)
        assert np.array_equal(core, host["core"])
        assert same_tree(t, stats.mreach_mst_host(metric, y, q, core, v=v))
        assert t["found"] == n - 1 and R.is_spanning_tree(n, t["lo"], t["hi"])
        np.testing.assert_allclose(y, host["y"], rtol=1e-15, atol=0)
        bound = R.pair_bound(metric, x, model.psi)
        y_r, q_r, w_r = R.pair_form(metric, x, model.psi)
        assert (np.abs(v - R.scores(y_r, q_r, w_r)) <= bound).all()


def test_forced_passes_and_repeated_runs_give_the_same_bits(engine, monkeypatch):
    rng = np.random.default_rng(43)
    x = rng.standard_normal((300, 5)) + rng.integers(0, 3, (300, 1)) * 3.0
    runs = []
    for cols in (None, "64", "128", None):
        if cols is None:
            monkeypatch.delenv("MFA_PLDA_PASS_COLS", raising=False)
        else:
            monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
        pf, t = device_tree(engine, "euclidean", x, 4, want_v=True)
        runs.append((pf["v"].cpu().numpy(), pf["core"].cpu().numpy(), t))
    for v, core, t in runs[1:]:
        assert np.array_equal(v, runs[0][0]) and np.array_equal(core, runs[0][1]) and same_tree(t, runs[0][2])
        assert t["rounds"] == runs[0][2]["rounds"]


def test_round_count_on_connected_data(engine):
    rng = np.random.default_rng(47)
    for n in (100, 300, 1000):
        x = rng.standard_normal((n, 8))
        _, t = device_tree(engine, "euclidean", x, 4)
        assert t["found"] == n - 1 and 1 <= t["rounds"] <= math.ceil(math.log2(n)) + 1


def test_the_path_in_random_order(engine):
    x, perm = R.path(300, 1, seed=3)
    _, t = device_tree(engine, "euclidean", x, 0)
    got = sorted((min(perm[a], perm[b]), max(perm[a], perm[b])) for a, b in zip(t["lo"].tolist(), t["hi"].tolist()))
    assert got == [(i, i + 1) for i in range(299)]


def test_a_nan_row_is_noise_and_the_rest_is_unchanged(engine):
    from montreal_forced_aligner_amd import cluster as CL
    x, _ = R.blobs((40, 40, 40), 5, 51, spread=10.0)
    bad = np.concatenate([x[:50], [[np.nan] * 5], x[50:]])
    pf, t = device_tree(engine, "euclidean", bad, 4)
    core = pf["core"].cpu().numpy()
    assert core[50] == -np.inf and np.isfinite(np.delete(core, 50)).all()
    assert t["found"] == 119 and t["score"][-1] == -np.inf and 50 in (t["lo"][-1], t["hi"][-1])
    kw = dict(distance_threshold=0.0, min_cluster_size=10, engine=engine)
    labels, clean = CL.hdbscan_matrix(bad, "euclidean", **kw), CL.hdbscan_matrix(x, "euclidean", **kw)
    assert labels[50] == -1 and np.array_equal(np.delete(labels, 50), clean)


def test_two_far_blobs_are_joined_by_one_edge(engine):
    x, truth = R.blobs((70, 60), 6, 53, spread=40.0)
    _, t = device_tree(engine, "euclidean", x, 4)
    crossing = [e for e, (a, b) in enumerate(zip(t["lo"].tolist(), t["hi"].tolist())) if truth[a] != truth[b]]
    assert crossing == [128]                                                  # one edge, the tree's longest


def test_refusals(engine):
    x = torch.zeros((4, 3), dtype=torch.float64, device=engine.device)
    out = torch.zeros((4, 3), dtype=torch.float64, device=engine.device)
    q, core = torch.zeros(4, dtype=torch.float64, device=engine.device), torch.zeros(4, dtype=torch.float64, device=engine.device)
    lo, hi = torch.zeros(3, dtype=torch.int32, device=engine.device), torch.zeros(3, dtype=torch.int32, device=engine.device)
    with pytest.raises(_lib.MfaHipError, match="neighbours"):
        engine._launch_hdbscan_core(x, 1, None, 65, out, q, core, None)
    with pytest.raises(_lib.MfaHipError, match="neighbours"):
        engine._launch_hdbscan_core(x, 1, None, -1, out, q, core, None)
    with pytest.raises(_lib.MfaHipError, match="metric"):
        engine._launch_hdbscan_core(x, 3, None, 1, out, q, core, None)
    with pytest.raises(_lib.MfaHipError, match="NULL"):
        engine._launch_hdbscan_core(x, 0, None, 1, out, q, core, None)       # plda without psi
    with pytest.raises(_lib.MfaHipError, match="NULL"):
        engine._launch_hdbscan_core(x, 1, None, 1, out, q, None, None)
    with pytest.raises(_lib.MfaHipError, match="dimension"):
        engine._launch_hdbscan_core(torch.zeros((2, 1025), dtype=torch.float64, device=engine.device), 1, None, 1,
                                    torch.zeros((2, 1025), dtype=torch.float64, device=engine.device), q, core, None)
    psi = torch.tensor([1.0, -2.0, 1.0], dtype=torch.float64, device=engine.device)
    with pytest.raises(_lib.MfaHipError, match="psi"):
        engine._launch_hdbscan_core(x, 0, psi, 1, out, q, core, None)
    with pytest.raises(_lib.MfaHipError, match="metric"):
        engine._launch_hdbscan_mst(out, q, core, 7, lo, hi, q)
    with pytest.raises(_lib.MfaHipError, match="NULL"):
        engine._launch_hdbscan_mst(out, q, core, 1, lo, None, q)
    with pytest.raises(_lib.MfaHipError, match="neighbours"):
        stats.core_scores(engine, "euclidean", x, 65)
    engine._launch_hdbscan_core(x, 1, None, 1, out, q, core, None)           # the context stays usable
    assert (core.cpu().numpy() == 0.0).all()
    assert engine._launch_hdbscan_mst(out, q, core, 1, lo, hi, torch.zeros(3, dtype=torch.float64, device=engine.device)) == (3, 1)
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 1), (0, 2), (0, 3)]
