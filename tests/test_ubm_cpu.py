"""The diagonal-UBM stage without a GPU: the host twins (mfa_debug_ubm_gselect_host, mfa_debug_ubm_acc_host: csrc/ubm_host.cpp
over csrc/ubm_math.hpp and csrc/gmm_acc_math.hpp) against the float64 restatement under the bounds tests/ubm_ref.py derives,
the facts that need no reference, the host layer (``ubm``, ``kaldi_io``), ``DubmTrainer`` on the host backend, and the twins'
translation unit under the host sanitizers as a stand-alone program (nothing is preloaded anywhere)."""
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib, kaldi_io
from montreal_forced_aligner_amd import ubm as U
from montreal_forced_aligner_amd.stats import GmmStats, gaussian_selection_host, ubm_statistics_host
from montreal_forced_aligner_amd.train import DubmTrainer, UbmHostBackend
from tests import ubm_ref as R

ROOT = Path(__file__).resolve().parents[1]


# ---- selection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,dim,n", ((256, 39, 30), (2048, 40, 30), (64, 13, 20), (130, 48, 64)))
def test_twin_selection_against_float64(G, dim, n):
    ubm, x = R.case(G, dim, 2000)
    gs, like = gaussian_selection_host(x, ubm, n)
    ll, e = R.loglikes(x, ubm)
    amb = R.ambiguous(ll, e, n)
    print(f"G {G} dim {dim} n {n}: {100 * amb.mean():.2f} % of frames set aside as boundary-ambiguous")
    assert amb.mean() <= 0.05                                            # a condition on the inputs, not a measurement
    want = R.select(ll, n)
    assert np.array_equal(np.sort(gs[~amb], axis=1), np.sort(want[~amb], axis=1))
    along = np.take_along_axis(ll, gs.astype(np.int64), axis=1)
    assert (np.diff(along, axis=1) <= 2 * e[:, None]).all()              # non-increasing up to 2·e_t, on every frame
    assert all(len(set(row)) == n for row in gs[amb])
    LL, bound = R.frame_loglike(ll, e, gs)
    assert (np.abs(like - LL) <= bound).all()


def test_ties_and_lists_longer_than_the_model():
    ubm, x = R.case(64, 13, 200)
    dup = U.DiagUbm(*(np.concatenate([a, a]) for a in (ubm.weights, ubm.means_invvars, ubm.inv_vars, ubm.gconsts)))
    gs, _ = gaussian_selection_host(x, dup, 8)
    assert (gs[:, 0::2] == gs[:, 1::2] + 64).all()                       # a Gaussian's copy, the larger index, comes first
    small, y = R.case(5, 13, 50)
    gs, like = gaussian_selection_host(y, small, 64 + 36)
    ll, e = R.loglikes(y, small)
    assert gs.shape == (50, 5) and (np.sort(gs, axis=1) == np.arange(5)).all()
    assert (np.diff(np.take_along_axis(ll, gs.astype(np.int64), axis=1), axis=1) <= 2 * e[:, None]).all()
    assert (np.abs(like - R.frame_loglike(ll, e, gs)[0]) <= R.frame_loglike(ll, e, gs)[1]).all()


def test_selection_survives_nan_and_infinite_rows():
    ubm, x = R.case(130, 48, 40)
    x = x.copy()
    x[3] = np.nan
    x[7, 5] = np.inf
    x[8] = -np.inf
    gs, _ = gaussian_selection_host(x, ubm, 30)
    assert ((gs >= 0) & (gs < 130)).all() and all(len(set(row)) == 30 for row in gs)


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def _weights(rng, T):
    return rng.choice(np.array([1.0, 0.5, 0.25, 0.0], np.float32), size=T, p=[0.6, 0.2, 0.15, 0.05])


@pytest.mark.parametrize("G,dim,n", ((256, 39, 30), (2048, 40, 30), (130, 40, None), (3, 13, 2)))
def test_statistics_twin_against_float64(G, dim, n):
    ubm, x = R.case(G, dim, 2000)
    x = x[:700]
    gs = None if n is None else gaussian_selection_host(x, ubm, n)[0]
    w = _weights(np.random.default_rng(G), 700)
    ref = R.ubm_acc(x, ubm, gs, w)
    if gs is None:
        st = ubm_statistics_host(x, ubm, None, w)
    else:
        st, post = ubm_statistics_host(x, ubm, gs, w, want_post=True)
        assert (np.abs(post - ref["post"]) <= ref["B_post"]).all()
    R.check_stats(st, ref, f"host twin, G {G} n {n}")


def test_statistics_twin_exact_tiers():
    rng = np.random.default_rng(2)
    T = 3000
    ubm = R.random_ubm(rng, 130, 40)
    x = rng.integers(-8, 9, size=(T, 40)).astype(np.float32)
    w = rng.choice(np.array([1.0, 0.5], np.float32), size=T)
    g = rng.integers(-2, 133, size=(T, 1)).astype(np.int32)              # some outside the model
    st, post = ubm_statistics_host(x, ubm, g, w, want_post=True)
    ok = (g[:, 0] >= 0) & (g[:, 0] < 130)
    assert np.array_equal(post[:, 0], np.where(ok, w, np.float32(0)))    # γ = w exactly
    xd = x.astype(np.float64)
    occ, mean, var = np.zeros(130), np.zeros((130, 40)), np.zeros((130, 40))
    np.add.at(occ, g[ok, 0], w[ok].astype(np.float64))
    np.add.at(mean, g[ok, 0], w[ok, None] * xd[ok])
    np.add.at(var, g[ok, 0], w[ok, None] * xd[ok] * xd[ok])
    assert np.array_equal(st.occ, occ) and np.array_equal(st.mean_acc, mean) and np.array_equal(st.var_acc, var)
    one = R.random_ubm(rng, 1, 40)                                       # the dense path with one Gaussian
    st = ubm_statistics_host(x, one, None, w)
    assert st.occ[0] == w.astype(np.float64).sum() and np.array_equal(st.mean_acc[0], (w[:, None] * xd).sum(axis=0))
    assert np.array_equal(st.var_acc[0], (w[:, None] * xd * xd).sum(axis=0)) and st.tot_count == st.occ[0]


def test_idle_frames_and_unselected_gaussians_leave_no_trace():
    ubm, x = R.case(130, 40, 600)
    rng = np.random.default_rng(77)
    gs = gaussian_selection_host(x, ubm, 10)[0].copy()
    gs[:, 3] = -1
    gs[gs == 17] = 130
    w = np.ones(600, np.float32)
    idle = rng.permutation(600)[:90]
    w[idle[:45]] = 0.0
    gs[idle[45:]] = np.array([-1, 130, 999, -5, 130, 131, -1, -1, 2 ** 30, -2], np.int32)
    start = GmmStats(rng.normal(size=130), rng.normal(size=(130, 40)), rng.normal(size=(130, 40)), 1.5, -2.5, np.zeros(1, np.int64))
    st, post = ubm_statistics_host(x, ubm, gs, w, into=start.copy(), want_post=True)
    assert st.occ[17] == start.occ[17] and np.array_equal(st.mean_acc[17], start.mean_acc[17])
    assert (post[idle] == 0).all() and (post[:, 3] == 0).all()
    keep = np.setdiff1d(np.arange(600), idle)
    assert R.bits(ubm_statistics_host(x[keep], ubm, gs[keep], w[keep], into=start.copy())) == R.bits(st)
    assert R.bits(ubm_statistics_host(x[idle], ubm, gs[idle], w[idle], into=start.copy())) == R.bits(start)
    assert R.bits(ubm_statistics_host(x[:0], ubm, gs[:0], None, into=start.copy())) == R.bits(start)


def test_twins_refuse_what_the_contract_excludes():
    lib = _lib.lib()
    z = np.zeros(64 * 70, np.float32)
    gs = np.zeros(70, np.int32)
    d = np.zeros(70 * 4)
    p = lambda a: a.ctypes.data
    sel = lambda T, dim, G, n, out=gs: lib.mfa_debug_ubm_gselect_host(p(z), T, dim, G, p(z), p(z), p(z), n, None if out is None else p(out), None)
    acc = lambda T, dim, G, n, g=gs, post=None, occ=d: lib.mfa_debug_ubm_acc_host(
        p(z), T, dim, G, p(z), p(z), p(z), n, None if g is None else p(g), None, None if occ is None else p(occ), p(d), p(d), p(d),
        None if post is None else p(post))
    assert sel(1, 4, 70, 4) == 0 and acc(1, 4, 70, 4) == 0
    assert sel(1, 0, 70, 4) == -1 and sel(1, 49, 70, 4) == -2 and sel(1, 4, 0, 4) == -3 and sel(1, 4, 2049, 4) == -3
    assert sel(1, 4, 70, 0) == -4 and sel(1, 4, 70, 65) == -4 and sel(1, 4, 64, 1000) == 0
    assert sel(2 ** 31, 4, 70, 4) == -5 and sel(1, 4, 70, 4, out=None) == -1
    assert acc(1, 49, 70, 4) == -2 and acc(1, 4, 2049, 4) == -3 and acc(1, 4, 70, 65) == -4 and acc(1, 4, 70, 0) == -4
    assert acc(1, 4, 70, 0, g=None) == 0                                 # n is ignored on the dense path
    assert acc(1, 4, 70, 4, g=None, post=z) == -1 and acc(1, 4, 70, 4, occ=None) == -1 and acc(2 ** 31, 4, 70, 4) == -5


# ---- host layer ---------------------------------------------------------------------------------------------------------------
def test_init_split_update_known_answers():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(500, 5)) * np.array([1.0, 2.0, 0.5, 3.0, 1.5])
    m = U.init_from_random_frames(x, 7, np.random.default_rng(0))
    var = (x * x).mean(axis=0) - x.mean(axis=0) ** 2
    assert m.num_gauss == 7 and np.allclose(m.variances, var[None], rtol=1e-6) and np.allclose(m.weights, 1 / 7)
    rows = [int(np.flatnonzero(np.all(np.isclose(x, mu, rtol=1e-5, atol=1e-6), axis=1))[0]) for mu in m.means]
    assert len(set(rows)) == 7                                           # distinct frames as means
    with pytest.raises(ValueError):
        U.init_from_random_frames(x[:3], 7)
    s = U.split(m, 10, 0.1, np.random.default_rng(1))
    assert s.num_gauss == 10 and abs(float(s.weights.astype(np.float64).sum()) - 1) < 1e-6
    assert np.isclose(np.sort(s.weights)[0], 1 / 14, rtol=1e-6) and np.allclose(s.variances, var[None], rtol=1e-6)
    assert U.split(m, 7) is m
    big = U.split(m, 300, 0.1, np.random.default_rng(1))                 # beyond mix_up's default of 128 per pdf
    assert big.num_gauss == 300
    with pytest.raises(ValueError):
        U.split(m, 2049)
    # update: two Gaussians with known statistics, a third below the occupancy floor is removed, the last one never is
    two = U.DiagUbm.from_parameters([0.5, 0.3, 0.2], np.zeros((3, 2)), np.ones((3, 2)))
    st = GmmStats.zeros(3, 2, 1)
    st.occ[:] = [100.0, 300.0, 2.0]
    st.mean_acc[:] = [[100.0, 200.0], [-300.0, 0.0], [1.0, 1.0]]
    st.var_acc[:] = [[200.0, 500.0], [600.0, 150.0], [1.0, 1.0]]
    new, updated, removed, floored = U.update(two, st, True)
    assert (new.num_gauss, updated, removed, floored) == (2, 2, 1, 0)
    assert np.allclose(new.means, [[1.0, 2.0], [-1.0, 0.0]]) and np.allclose(new.variances, [[1.0, 1.0], [1.0, 0.5]])
    assert np.allclose(new.weights, [0.25, 0.75]) and abs(float(new.weights.sum()) - 1) < 1e-6
    kept = U.update(two, st, False)[0]
    assert kept.num_gauss == 3 and abs(float(kept.weights.astype(np.float64).sum()) - 1) < 1e-6
    st.occ[:] = [1.0, 2.0, 3.0]                                          # every Gaussian below the floor: one survives
    assert U.update(two, st, True)[0].num_gauss == 1


def test_init_schedules_by_hand():
    start, sched = U.init_schedule()                                     # 256 Gaussians, half of them first, 20 iterations
    assert start == 128 and sched == [min(256, 128 + 12 * (i + 1)) for i in range(20)] and sched[9] == 248 and sched[10] == 256
    start, sched = U.init_schedule(rule="reference")                     # min(256, cur, 12) never exceeds cur
    assert start == 128 and sched == [128] * 20
    assert U.init_schedule(16, 0.5, 4) == (8, [12, 16, 16, 16])
    assert U.init_schedule(16, 0.0, 4) == (16, [16] * 4) and U.init_schedule(16, 2.0, 4)[0] == 16
    with pytest.raises(ValueError):
        U.init_schedule(rule="other")


def test_diag_gmm_and_gselect_archive_round_trips(tmp_path):
    from montreal_forced_aligner_amd import kalpy_api as KA

    ubm, _ = R.case(65, 13, 10)
    ubm.write(tmp_path / "a.dubm")
    back = U.DiagUbm.read(tmp_path / "a.dubm")
    assert all(np.array_equal(a, b) for a, b in zip(back.arrays(), ubm.arrays())) and np.array_equal(back.weights, ubm.weights)
    buf = io.BytesIO()
    kaldi_io.write_diag_gmm(buf, ubm.gconsts, ubm.weights, ubm.means_invvars, ubm.inv_vars)
    gc, w, mi, iv = kaldi_io.read_diag_gmm(kaldi_io.BinaryReader(buf.getvalue()))
    assert np.array_equal(gc, ubm.gconsts) and np.array_equal(mi, ubm.means_invvars)
    entries = [("utt-a", [[3, 1, 2], [0, 5, 4]]), ("utt-b", [[7, 8, 9]]), ("utt-c", [])]
    KA.GselectArchive.write(tmp_path / "gselect.ark", entries)
    ar = KA.GselectArchive(tmp_path / "gselect.ark")
    assert list(ar) == entries and ar["utt-b"] == [[7, 8, 9]] and "utt-c" in ar and "utt-d" not in ar
    assert np.array_equal(ar.matrix("utt-a"), [[3, 1, 2], [0, 5, 4]])
    raw = dict(kaldi_io.read_ark((tmp_path / "gselect.ark").read_bytes(), "int_vector_vector"))
    assert [v.tolist() for v in raw["utt-a"]] == entries[0][1]


# ---- trainer ------------------------------------------------------------------------------------------------------------------
def check_trainer(tr, directory):
    """What both corpora and both backends are held to."""
    assert len(tr.loglikes) == tr.num_iterations and len(tr.models) == tr.num_iterations + 1
    final = U.DiagUbm.read(Path(directory) / "final.dubm")
    assert all(np.array_equal(a, b) for a, b in zip(final.arrays(), tr.ubm.arrays()))
    assert sorted(p.name for p in Path(directory).iterdir()) == sorted([f"{i}.dubm" for i in range(1, tr.num_iterations + 2)] + ["final.dubm"])
    return final


def test_trainer_on_a_known_mixture(tmp_path):
    _truth, utts = R.mixture8()
    tr = DubmTrainer(num_iterations=4, num_gselect=8, num_gaussians=8, num_iterations_init=4, initial_gaussian_proportion=0.5,
                     num_frames=5000, backend=UbmHostBackend(batch_frames=6000)).train(utts, tmp_path)
    print("init", np.round(tr.init_loglikes, 4), "train", np.round(tr.loglikes, 4))
    assert tr.backend.num_frames == 20000 and len(tr.backend.batches) == 4
    # every Gaussian is selected, so this is EM and its guarantee holds: up to the float32 evaluation of the likelihood
    assert all(b >= a - 1e-4 * abs(a) for a, b in zip(tr.loglikes, tr.loglikes[1:]))
    final = check_trainer(tr, tmp_path)
    assert final.num_gauss == 8
    assert tr.loglikes[-1] > tr.init_loglikes[0]


def test_trainer_on_the_reference_recording(tmp_path):
    utts = R.wav_features()
    tr = DubmTrainer(num_iterations=2, num_gselect=30, num_gaussians=16, num_iterations_init=4, backend=UbmHostBackend())
    tr.train(utts, tmp_path)
    print("init", np.round(tr.init_loglikes, 4), "select", round(tr.select_loglike, 4), "train", np.round(tr.loglikes, 4))
    check_trainer(tr, tmp_path)
    assert tr.loglikes[-1] > tr.init_loglikes[0]
    assert sum(g.shape[0] for _k, g in tr.backend.selections()) == tr.backend.num_frames


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "ubm_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "ubm_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "ubm_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout
