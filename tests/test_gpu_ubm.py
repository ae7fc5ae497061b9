"""The diagonal-UBM stage on the device (csrc/ubm.hip): Gaussian selection and the global statistics, at the shapes where the
kernels can go wrong — G from 1 to 2048 around the rounds of 64, lists of 1 to 64, dims 13 – 48, frame counts around the
selection's tile and the statistics' slab.

Selection: the device's indices are the host twin's bit for bit (both run csrc/gmm_acc_math.hpp and csrc/ubm_math.hpp on the
same float32 inputs); the frame log-likelihood is held to the float64 restatement under the bound tests/ubm_ref.py derives.
Statistics: two exact tiers — a list of one Gaussian (γ = w exactly) and the dense path with one Gaussian, on small-integer
features with weights 1 and ½, where every addend and every partial sum is exact in double, so the result is float64's bit
for bit whatever the order — and a soft tier against the float64 restatement under its bound, with the twin within twice
that bound (either side within it once)."""
import ctypes

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.stats import (GmmStats, gaussian_selection, gaussian_selection_host, ubm_statistics,
                                               ubm_statistics_host)
from montreal_forced_aligner_amd.ubm import DiagUbm
from tests import ubm_ref as R

pytestmark = pytest.mark.gpu


def _dev(e, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _tile(engine):
    return int(engine.lib.mfa_ubm_gselect_tile_frames())


def _slab(engine):
    return int(engine.lib.mfa_ubm_acc_slab_frames())


def device_select(engine, x, ubm, n):
    gs, ll = gaussian_selection(engine, _dev(engine, x), ubm, n)
    return gs.cpu().numpy(), ll.cpu().numpy()


def device_stats(engine, x, ubm, gselect=None, weight=None, into=None, want_post=False):
    r = ubm_statistics(engine, _dev(engine, x), ubm, _dev(engine, gselect), _dev(engine, weight), into=into, want_post=want_post)
    return (r[0], r[1].cpu().numpy()) if want_post else r


def check_selection(engine, ubm, x, n, what):
    gs_d, ll_d = device_select(engine, x, ubm, n)
    gs_h, ll_h = gaussian_selection_host(x, ubm, n)
    assert gs_d.shape == (x.shape[0], min(n, ubm.num_gauss)), what
    assert np.array_equal(gs_d, gs_h), (what, int((gs_d != gs_h).any(axis=1).sum()))
    ll, e = R.loglikes(x, ubm)
    LL, bound = R.frame_loglike(ll, e, gs_d)
    worst = float(np.max(np.abs(ll_d - LL) / bound))
    print(f"{what}: worst |device loglike - float64| / bound = {worst:.4f}; twin {float(np.max(np.abs(ll_h - LL) / bound)):.4f}")
    assert (np.abs(ll_d - LL) <= bound).all(), (what, worst)
    assert (np.abs(ll_d.astype(np.float64) - ll_h) <= 2 * bound).all(), what


# ---- selection --------------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(1, 1, 13), (2, 1, 39), (2, 20, 40), (63, 20, 13), (64, 64, 48), (65, 30, 40), (65, 64, 39), (130, 64, 48),
                 (130, 30, 13), (256, 30, 39), (256, 1, 40), (2048, 30, 40), (2048, 64, 48), (2048, 20, 13)]


@pytest.mark.parametrize("G,n,dim", SELECT_SHAPES)
def test_selection_is_the_twins_bit_for_bit(engine, G, n, dim):
    ubm, x = R.case(G, dim, 3 * _tile(engine) + 1)
    check_selection(engine, ubm, x, n, f"G {G} n {n} dim {dim}")


def test_selection_frame_counts_around_a_tile(engine):
    tile = _tile(engine)
    ubm, x = R.case(130, 40, 3 * tile + 1)
    for T in (1, tile - 1, tile, tile + 1):
        check_selection(engine, ubm, x[:T], 30, f"{T} frames")


def test_selection_without_loglike(engine):
    ubm, x = R.case(65, 40, 100)
    gs = torch.full((100, 20), -7, dtype=torch.int32, device=engine.device)
    engine._launch_ubm_gselect(_dev(engine, x), tuple(_dev(engine, a) for a in ubm.arrays()), 20, gs, None)
    assert np.array_equal(gs.cpu().numpy(), gaussian_selection_host(x, ubm, 20)[0])


def test_selection_survives_nan_and_infinite_rows(engine):
    ubm, x = R.case(130, 39, 3 * _tile(engine) + 1)
    x = x.copy()
    x[5] = np.nan
    x[70, 3] = np.inf
    x[71, :] = -np.inf
    x[130, 0] = np.nan
    bad = np.array([5, 70, 71, 130])
    gs, _ = device_select(engine, x, ubm, 30)
    assert ((gs >= 0) & (gs < 130)).all()
    assert all(len(set(row)) == 30 for row in gs[bad])
    good = np.setdiff1d(np.arange(x.shape[0]), bad)
    assert np.array_equal(gs[good], gaussian_selection_host(x[good], ubm, 30)[0])


def test_ties_come_out_larger_index_first(engine):
    ubm, x = R.case(65, 13, 50)
    dup = DiagUbm(*(np.concatenate([a, a]) for a in (ubm.weights, ubm.means_invvars, ubm.inv_vars, ubm.gconsts)))
    gs, _ = device_select(engine, x, dup, 6)
    assert np.array_equal(gs, gaussian_selection_host(x, dup, 6)[0])
    assert (gs[:, 0::2] == gs[:, 1::2] + 65).all()          # every Gaussian's copy, the larger index, right before it


# ---- statistics, exact tiers --------------------------------------------------------------------------------------------------
def _integer_case(rng, G, dim, T):
    ubm = R.random_ubm(rng, G, dim)
    x = rng.integers(-8, 9, size=(T, dim)).astype(np.float32)
    w = rng.choice(np.array([1.0, 0.5], np.float32), size=T)
    return ubm, x, w


def _exact_sums(x, w, g, G):
    x = x.astype(np.float64)
    occ, mean, var = np.zeros(G), np.zeros((G, x.shape[1])), np.zeros((G, x.shape[1]))
    ok = (g >= 0) & (g < G)
    np.add.at(occ, g[ok], w[ok].astype(np.float64))
    np.add.at(mean, g[ok], w[ok, None] * x[ok])
    np.add.at(var, g[ok], w[ok, None] * x[ok] * x[ok])
    return occ, mean, var, float(w[ok].astype(np.float64).sum())


@pytest.mark.parametrize("G,dim", ((130, 40), (2048, 13), (3, 48)))
def test_a_list_of_one_gaussian_is_exact(engine, G, dim):
    T = 2 * _slab(engine) + 77
    rng = np.random.default_rng(41 + G)
    ubm, x, w = _integer_case(rng, G, dim, T)
    g = rng.integers(0, G, size=(T, 1)).astype(np.int32)
    g[rng.permutation(T)[:50], 0] = rng.choice(np.array([-1, G, G + 5, -2 ** 31], np.int64), size=50).astype(np.int32)
    st, post = device_stats(engine, x, ubm, g, w, want_post=True)
    occ, mean, var, wsum = _exact_sums(x, w, g[:, 0], G)
    assert np.array_equal(st.occ, occ) and np.array_equal(st.mean_acc, mean) and np.array_equal(st.var_acc, var)
    assert st.tot_count == wsum
    ok = (g[:, 0] >= 0) & (g[:, 0] < G)
    assert np.array_equal(post[:, 0], np.where(ok, w, np.float32(0)))
    twin = ubm_statistics_host(x, ubm, g, w)
    assert np.array_equal(twin.occ, occ) and np.array_equal(twin.mean_acc, mean) and np.array_equal(twin.var_acc, var)
    ref = R.ubm_acc(x, ubm, g, w)
    assert abs(st.tot_like - ref["tot"][0]) <= ref["B_tot"] and abs(twin.tot_like - ref["tot"][0]) <= ref["B_tot"]


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_the_dense_path_with_one_gaussian_is_exact(engine, dim):
    T = _slab(engine) + 5
    ubm, x, w = _integer_case(np.random.default_rng(dim), 1, dim, T)
    w[::7] = 0.0
    st = device_stats(engine, x, ubm, None, w)
    occ, mean, var, wsum = _exact_sums(x, w, np.where(w != 0, 0, -1), 1)
    assert np.array_equal(st.occ, occ) and np.array_equal(st.mean_acc, mean) and np.array_equal(st.var_acc, var)
    assert st.tot_count == wsum


# ---- statistics, soft tier --------------------------------------------------------------------------------------------------
def check_soft(engine, ubm, x, gs, w, what):
    ref = R.ubm_acc(x, ubm, gs, w)
    if gs is None:
        st = device_stats(engine, x, ubm, None, w)
        twin = ubm_statistics_host(x, ubm, None, w)
    else:
        st, post = device_stats(engine, x, ubm, gs, w, want_post=True)
        twin, post_h = ubm_statistics_host(x, ubm, gs, w, want_post=True)
        assert (np.abs(post - ref["post"]) <= ref["B_post"]).all(), what
        assert (np.abs(post.astype(np.float64) - post_h) <= 2 * ref["B_post"]).all(), what
        assert (post[~ref["live"]] == 0).all(), what
    R.check_stats(st, ref, what + ", device")
    for got, want, bound in ((st.occ, twin.occ, ref["B_occ"]), (st.mean_acc, twin.mean_acc, ref["B_mean"]),
                             (st.var_acc, twin.var_acc, ref["B_var"])):
        assert (np.abs(got - want) <= 2 * bound).all(), what
    assert abs(st.tot_like - twin.tot_like) <= 2 * ref["B_tot"], what
    assert st.tot_count == twin.tot_count, what
    return st


def _weights(rng, T):
    return rng.choice(np.array([1.0, 0.5, 0.25, 0.0], np.float32), size=T, p=[0.6, 0.2, 0.15, 0.05])


@pytest.mark.parametrize("G,dim", ((256, 39), (2048, 40)))
def test_soft_statistics_over_a_selection(engine, G, dim):
    ubm, x = R.case(G, dim, 600)
    gs = gaussian_selection_host(x, ubm, 30)[0]
    check_soft(engine, ubm, x, gs, _weights(np.random.default_rng(G), 600), f"n 30 of {G}")
    assert R.ubm_acc(x, ubm, gs)["occ"].min() == 0 or G == 256      # at 2048 some Gaussian goes unselected


def test_soft_statistics_dense(engine):
    ubm, x = R.case(130, 40, 600)
    check_soft(engine, ubm, x, None, _weights(np.random.default_rng(130), 600), "dense G 130")


def test_slab_edges(engine):
    slab = _slab(engine)
    ubm, x = R.case(3, 13, 2 * slab + 3)
    gs = gaussian_selection_host(x, ubm, 2)[0]
    w = _weights(np.random.default_rng(3), x.shape[0])
    for T in (slab - 1, slab, slab + 1, 2 * slab + 3):
        check_soft(engine, ubm, x[:T], gs[:T], w[:T], f"{T} frames, n 2 of 3")
        check_soft(engine, ubm, x[:T], None, w[:T], f"{T} frames, dense 3")


# ---- determinism, additivity, passes ----------------------------------------------------------------------------------------
def test_determinism_additivity_and_passes(engine, monkeypatch):
    slab = _slab(engine)
    ubm, x = R.case(130, 40, 3 * slab + 11)
    gs = gaussian_selection_host(x, ubm, 20)[0]
    w = _weights(np.random.default_rng(9), x.shape[0])
    for sel in (gs, None):
        sub = lambda a, b: (x[a:b], ubm, None if sel is None else sel[a:b], w[a:b])
        whole = device_stats(engine, *sub(0, None))
        assert R.bits(device_stats(engine, *sub(0, None))) == R.bits(whole)
        part = device_stats(engine, *sub(0, 2 * slab))
        part = device_stats(engine, *sub(2 * slab, None), into=part)
        assert R.bits(part) == R.bits(whole)
        monkeypatch.setenv("MFA_UBM_PASS_SLABS", "1")
        assert R.bits(device_stats(engine, *sub(0, None))) == R.bits(whole)
        monkeypatch.delenv("MFA_UBM_PASS_SLABS")


# ---- accumulator hygiene ----------------------------------------------------------------------------------------------------
def _random_into(rng, G, D):
    return GmmStats(rng.normal(size=G), rng.normal(size=(G, D)), rng.normal(size=(G, D)), float(rng.normal()), float(rng.normal()),
                    np.zeros(1, np.int64))


def test_accumulators_are_added_to_and_idle_frames_leave_no_trace(engine):
    ubm, x = R.case(130, 40, 600)
    rng = np.random.default_rng(77)
    gs = gaussian_selection_host(x, ubm, 10)[0].copy()
    gs[:, 3] = -1                                      # an entry outside the model in every list
    gs[gs == 17] = 130                                 # Gaussian 17 is selected by nobody
    w = np.ones(600, np.float32)
    idle = rng.permutation(600)[:90]
    w[idle[:45]] = 0.0
    gs[idle[45:]] = np.array([-1, 130, 999, -5, 130, 131, -1, -1, 2 ** 30, -2], np.int32)
    start = _random_into(rng, 130, 40)
    st, post = device_stats(engine, x, ubm, gs, w, into=start.copy(), want_post=True)
    # added to: minus the start it is the statistics from zero, up to the rounding of the additions onto the start
    zero = device_stats(engine, x, ubm, gs, w)
    for got, s0, z in ((st.occ, start.occ, zero.occ), (st.mean_acc, start.mean_acc, zero.mean_acc), (st.var_acc, start.var_acc, zero.var_acc)):
        assert (np.abs(got - (s0 + z)) <= 4 * R.U64 * (np.abs(s0) + np.abs(z))).all()
    # Gaussian 17 keeps the caller's bits
    assert st.occ[17] == start.occ[17] and np.array_equal(st.mean_acc[17], start.mean_acc[17]) and np.array_equal(st.var_acc[17], start.var_acc[17])
    assert (post[idle] == 0).all() and (post[:, 3] == 0).all()
    # the idle frames leave no trace: whatever their rows hold, the bits are the same (the frames keep their places: the
    # instruction's own order over a step's 4 frames is not part of the contract)
    other = x.copy()
    other[idle] = rng.normal(0.0, 50.0, size=(90, 40)).astype(np.float32)
    assert R.bits(device_stats(engine, other, ubm, gs, w, into=start.copy())) == R.bits(st)
    # a batch of idle frames alone changes nothing
    assert R.bits(device_stats(engine, x[idle], ubm, gs[idle], w[idle], into=start.copy())) == R.bits(start)
    assert R.bits(device_stats(engine, x[idle[:45]], ubm, None, w[idle[:45]], into=start.copy())) == R.bits(start)


def test_an_empty_batch_writes_nothing(engine):
    ubm, _ = R.case(65, 40, 100)
    start = _random_into(np.random.default_rng(1), 65, 40)
    x = np.zeros((0, 40), np.float32)
    assert R.bits(device_stats(engine, x, ubm, np.zeros((0, 20), np.int32), None, into=start.copy())) == R.bits(start)
    assert R.bits(device_stats(engine, x, ubm, None, None, into=start.copy())) == R.bits(start)
    gs, ll = device_select(engine, x, ubm, 20)
    assert gs.shape == (0, 20) and ll.shape == (0,)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_a_message_and_a_usable_context(engine):
    ubm, x = R.case(65, 40, 100)
    good = gaussian_selection_host(x, ubm, 20)[0]

    def still_works():
        assert np.array_equal(device_select(engine, x, ubm, 20)[0], good)

    def model(G, dim):
        return tuple(torch.zeros(s, dtype=torch.float32, device=engine.device) for s in ((G,), (G, dim), (G, dim)))

    def select(T, dim, G, n, out=True, mdl=None):
        feats = torch.zeros((T, dim), dtype=torch.float32, device=engine.device)
        gs = torch.zeros((T, max(min(n, G), 1)), dtype=torch.int32, device=engine.device) if out else None
        engine._launch_ubm_gselect(feats, mdl or model(G, dim), n, gs, None)

    def acc(T, dim, G, n, gselect=True, post=False, accs=True):
        feats = torch.zeros((T, dim), dtype=torch.float32, device=engine.device)
        gs = torch.zeros((T, max(n, 1)), dtype=torch.int32, device=engine.device) if gselect else None
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=engine.device) if accs else None
        p = torch.zeros((T, max(n, 1)), dtype=torch.float32, device=engine.device) if post else None
        engine._launch_ubm_acc(feats, model(G, dim), n, gs, None, z(G), z(G, dim), z(G, dim), z(2), p)

    cases = [("dim", lambda: select(4, 49, 8, 4)), ("Gaussians", lambda: select(4, 13, 2049, 4)),
             ("per frame", lambda: select(4, 13, 8, 0)), ("per frame", lambda: select(4, 13, 100, 65)),
             ("NULL output", lambda: select(4, 13, 8, 4, out=False)),
             ("dim", lambda: acc(4, 49, 8, 4)), ("Gaussians", lambda: acc(4, 13, 2049, 4)), ("per frame", lambda: acc(4, 13, 100, 65)),
             ("per frame", lambda: acc(4, 13, 8, 0)), ("d_post needs", lambda: acc(4, 13, 8, 4, gselect=False, post=True)),
             ("NULL accumulator", lambda: acc(4, 13, 8, 4, accs=False))]
    for word, call in cases:
        with pytest.raises(MfaHipError, match=word):
            call()
        still_works()
    select(4, 13, 64, 165)                                   # min(num_gselect, G) = 64: fine
    # 2^31 frames: refused before anything is read
    m = model(8, 13)
    rc = engine.lib.mfa_ubm_gselect_batch(engine.ctx, ctypes.c_void_p(m[1].data_ptr()), 2 ** 31, 13, 8, ctypes.c_void_p(m[0].data_ptr()),
                                          ctypes.c_void_p(m[1].data_ptr()), ctypes.c_void_p(m[2].data_ptr()), 4,
                                          ctypes.c_void_p(m[1].data_ptr()), None)
    assert rc != 0 and b"2^31" in engine.lib.mfa_last_error(engine.ctx)
    still_works()
