"""The host half of model adaptation (montreal_forced_aligner_amd/adapt.py): smoothing towards the old model, the mean update
with its two thresholds, the gconsts, the model file round trip and the transition update — float64 numpy, no GPU.

The round trip of a mean.  With all-zero statistics smoothing leaves occ = τ and mean_acc = τ·μ, μ = fl32(mi / iv) widened to
double; the update forms fl32(fl64(τ·μ) / τ): two float64 roundings on a float32 value, far inside half a float32 ulp, so μ
comes back exactly.  The stored row is then mi' = fl32(μ·iv) = mi·(1 + δ₁)(1 + δ₂), |δ| ≤ 2⁻²⁴: |mi' − mi| ≤ 2·2⁻²⁴·|mi|(1 + 2⁻²⁴),
and a float32 ulp is at least 2⁻²⁴·|mi|: at most 2 ulp (differences of neighbouring floats are whole ulps)."""
import io

import numpy as np
import pytest

import synth_workload as SW
from montreal_forced_aligner_amd import adapt as A
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.engine import GmmStats


def _raw(rng, dim, sizes):
    """A fresh model through synth_workload._gauss, in the per-pdf form, with its float64 means, variances and weights."""
    gcs, ws, mis, ivs, par = [], [], [], [], []
    for n in sizes:
        w = rng.dirichlet(np.ones(n)) if n > 1 else np.ones(1)
        mean, var = rng.normal(0, 3, size=(n, dim)), rng.uniform(0.5, 4.0, size=(n, dim))
        g = [SW._gauss(mean[i], var[i], w[i]) for i in range(n)]
        gcs.append(np.array([x[0] for x in g], np.float32)); mis.append(np.stack([x[1] for x in g])); ivs.append(np.stack([x[2] for x in g]))
        ws.append(w.astype(np.float32)); par.append((mean, var, w))
    return K.RawAmDiagGmm(dim, gcs, ws, mis, ivs), par


def _zeros(raw, n_tids=1):
    return GmmStats.zeros(int(A.pdf_offsets(raw)[-1]), raw.dim, n_tids)


def test_zero_statistics_give_the_model_back():
    raw, _ = _raw(np.random.default_rng(1), 40, [1, 4, 17, 33])
    new, updated, kept = A.map_update(raw, A.ismooth_from_model(raw, _zeros(raw), 20.0))
    assert (updated, kept) == (55, 0) and new.dim == raw.dim
    for p in range(raw.num_pdfs):
        assert new.weights[p].tobytes() == raw.weights[p].tobytes() and new.inv_vars[p].tobytes() == raw.inv_vars[p].tobytes()
        a, b = raw.means_invvars[p], new.means_invvars[p]
        assert b.dtype == np.float32
        assert (np.abs(a - b) <= 2 * np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()
        # and the mean itself is exactly the model's: fl32(mi / iv) before, the value mi' was formed from after
        mu = a / raw.inv_vars[p]
        assert np.array_equal(b, mu * raw.inv_vars[p])


def test_single_gaussian_with_known_sums():
    dim, tau, n = 5, 20.0, 137
    rng = np.random.default_rng(2)
    mean = rng.normal(0, 3, size=dim).astype(np.float32).astype(np.float64)
    g = SW._gauss(mean, np.ones(dim))                      # variance 1: means_invvars is the mean itself
    raw = K.RawAmDiagGmm(dim, [np.array([g[0]])], [np.ones(1, np.float32)], [g[1][None]], [g[2][None]])
    x = rng.normal(1.0, 1.0, size=(n, dim))
    st = _zeros(raw)
    st.occ[0], st.mean_acc[0], st.var_acc[0] = n, x.sum(axis=0), (x * x).sum(axis=0)
    sm = A.ismooth_from_model(raw, st, tau)
    assert sm.occ[0] == n + tau and np.array_equal(sm.var_acc[0], st.var_acc[0] + tau * (1.0 + mean * mean))
    new, updated, kept = A.map_update(raw, sm)
    want = (x.sum(axis=0) + tau * mean) / (n + tau)
    assert (updated, kept) == (1, 0)
    assert np.array_equal(new.means_invvars[0][0], want.astype(np.float32))
    assert st.occ[0] == n                                   # the caller's statistics are left alone


def _two(occ_small, occ_big):
    raw, _ = _raw(np.random.default_rng(3), 4, [2])
    st = _zeros(raw)
    st.occ[:] = [occ_small, occ_big]
    st.mean_acc[:] = st.occ[:, None] * np.array([[1.0, 2.0, 3.0, 4.0], [-1.0, 0.5, 0.0, 2.0]])
    new, updated, kept = A.map_update(raw, st)            # τ = 0: no smoothing
    return raw, new, updated, kept


def test_occupancy_threshold_from_both_sides():
    raw, new, updated, kept = _two(10.0, 50.0)
    assert (updated, kept) == (1, 1) and new.means_invvars[0][0].tobytes() == raw.means_invvars[0][0].tobytes()
    raw, new, updated, kept = _two(np.nextafter(10.0, 11.0), 50.0)
    assert (updated, kept) == (2, 0)
    assert np.array_equal(new.means_invvars[0][0], np.array([1, 2, 3, 4], np.float32) * raw.inv_vars[0][0])


def test_weight_share_threshold_from_both_sides():
    raw, new, updated, kept = _two(29.0, 3.0e6)           # 29 / 3 000 029 = 9.67e-6: above 10 frames, below the share
    assert (updated, kept) == (1, 1) and new.means_invvars[0][0].tobytes() == raw.means_invvars[0][0].tobytes()
    raw, new, updated, kept = _two(31.0, 3.0e6)           # 31 / 3 000 031 = 1.03e-5
    assert (updated, kept) == (2, 0)


def test_gconsts_follow_the_model_formula_and_bad_ones_raise():
    raw, par = _raw(np.random.default_rng(4), 39, [1, 5, 32])
    new, _, _ = A.map_update(raw, A.ismooth_from_model(raw, _zeros(raw), 20.0))
    for p in range(raw.num_pdfs):
        # synth_workload._gauss's formula on the parameters the new model stores (float32, widened)
        iv, mi, w = new.inv_vars[p].astype(np.float64), new.means_invvars[p].astype(np.float64), new.weights[p].astype(np.float64)
        want = np.array([SW._gauss(mi[i] / iv[i], 1.0 / iv[i], w[i])[0] for i in range(len(w))])
        # two float64 evaluations of one expression (ln var against −ln inv_var, mean²·inv against mi²/inv): 1e-13 apart,
        # so the same float32 unless a tie lies between them: at most one float32 spacing
        assert (np.abs(new.gconsts[p] - want) <= np.spacing(np.abs(want))).all()
        assert new.gconsts[p].dtype == np.float32
    bad = K.RawAmDiagGmm(raw.dim, raw.gconsts, [w.copy() for w in raw.weights], raw.means_invvars, raw.inv_vars)
    bad.weights[1][2] = 0.0
    with pytest.raises(ValueError, match="not finite"):
        A.map_update(bad, _zeros(raw))


def _tm(states):
    """One phone with the given HMM states; tuples (phone 1, state, pdf = state)."""
    topo = K.HmmTopology(np.array([1], np.int32), np.array([-1, 0], np.int32), [states])
    n = sum(1 for s in states if s.transitions)
    tuples = np.array([(1, hs, hs, hs) for hs in range(n)], np.int32)
    return K.RawTransitionModel(topo, tuples, SW._log_probs(topo, tuples))


def test_written_model_reads_back_bit_for_bit():
    rng = np.random.default_rng(5)
    raw, _ = _raw(rng, 13, [1, 3, 9])
    st = _zeros(raw)
    st.occ[:] = rng.uniform(0, 40, size=13)
    st.mean_acc[:] = st.occ[:, None] * rng.normal(size=(13, 13))
    new, _, _ = A.adapt_model(raw, st, 20.0)
    tm = _tm([K.HmmState(i, i, [(i, 0.75), (i + 1, 0.25)]) for i in range(3)] + [K.HmmState(-1, -1, [])])
    tm2 = A.transition_update(tm, np.array([0, 30, 10, 2, 1, 0, 9]))
    buf = io.BytesIO()
    K.write_model(buf, tm2, new)
    rtm, ram = K.read_model(buf.getvalue())
    assert rtm.log_probs.tobytes() == tm2.log_probs.tobytes() and np.array_equal(rtm.tuples, tm2.tuples)
    for name in ("gconsts", "weights", "means_invvars", "inv_vars"):
        for a, b in zip(getattr(new, name), getattr(ram, name)):
            assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), name
    soa = M.DiagGmmModel.from_raw(ram)
    assert soa.weights.tobytes() == np.concatenate(new.weights).tobytes()
    assert np.array_equal(np.concatenate(A.raw_from_soa(soa).weights), soa.weights)


def test_transition_update():
    f32 = np.float32
    states = [K.HmmState(0, 0, [(0, 0.5), (1, 0.25), (2, 0.25)]),     # three transitions: ids 1, 2, 3
              K.HmmState(1, 1, [(1, 0.75), (2, 0.25)]),              # ids 4, 5
              K.HmmState(2, 2, [(3, 1.0)]),                          # a single transition: id 6
              K.HmmState(3, 3, [(3, 0.75), (4, 0.25)]),              # ids 7, 8
              K.HmmState(-1, -1, [])]
    tm = _tm(states)
    old = tm.log_probs.copy()
    cnt = np.array([0, 6, 3, 1, 40, 0, 1000, 3, 1])
    new = A.transition_update(tm, cnt)
    assert np.array_equal(tm.log_probs, old), "the caller's model is left alone"
    # hand-computed three-way case: 0.6, 0.3, 0.1 are above the floor and sum to one (within rounding) all three times
    p = (np.array([6, 3, 1]) / 10.0).astype(f32)
    for _ in range(3):
        p = np.maximum(p / f32(f32(p[0] + p[1]) + p[2]), f32(0.01))
    assert np.array_equal(new.log_probs[1:4], np.array([M._logf(v) for v in p], f32))
    assert np.allclose(np.exp(new.log_probs[1:4]), [0.6, 0.3, 0.1], rtol=1e-6)
    # a zero count: floored at 0.01; three rounds of {normalise, floor} on (1, 0): (1, .01) → (1/1.01, .01) → (…/…, .01)
    q = np.array([1.0, 0.0], f32)
    for _ in range(3):
        q = np.maximum(q / f32(q[0] + q[1]), f32(0.01))
    assert q[1] == f32(0.01) and np.array_equal(new.log_probs[4:6], np.array([M._logf(v) for v in q], f32))
    assert new.log_probs[6] == old[6], "a state with a single transition keeps its probability"
    assert np.array_equal(new.log_probs[7:9], old[7:9]), "a total below 5 leaves the state untouched"
    assert new.log_probs[0] == old[0]
    at5 = A.transition_update(tm, np.array([0, 0, 0, 0, 0, 0, 0, 4, 1]))
    assert not np.array_equal(at5.log_probs[7:9], old[7:9]) and np.array_equal(at5.log_probs[1:7], old[1:7])
    with pytest.raises(ValueError):
        A.transition_update(tm, cnt[:-1])
