"""The i-vector extractor stage without a GPU: the host twins (mfa_debug_ivector_*_host: csrc/ivector_host.cpp over
csrc/ivector_math.hpp) against the float64 restatement under the bounds tests/ivector_ref.py derives, the host layer
(``ivector``, ``kaldi_io``), ``IvectorTrainer`` on the host backend, and the twins' translation unit under the host sanitizers as
a stand-alone program (nothing is preloaded anywhere)."""
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib, kaldi_io
from montreal_forced_aligner_amd import ivector as IV
from montreal_forced_aligner_amd.kaldi_io import pack_lower, unpack_lower
from montreal_forced_aligner_amd.stats import (ivector_estep_host, ivector_utterance_statistics_host, prune_posteriors_host)
from montreal_forced_aligner_amd.train import IvectorHostBackend, IvectorTrainer
from tests import ivector_ref as R

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


# ---- pruning ------------------------------------------------------------------------------------------------------------------
def test_pruning_by_hand():
    post = np.array([[0.01, 0.02, 0.005, 0.0],          # all below min_post: the largest survives alone
                     [0.02, 0.01, 0.02, 0.001],         # a tie for the largest: the first in list order
                     [0.025, 0.9, 0.075, 0.0],          # exactly at min_post: it stays
                     [0.0, 0.0, 0.0, 0.0],              # a frame that took no part
                     [0.5, 0.25, 0.125, 0.125]], f32)
    out = prune_posteriors_host(post, 0.025, 1.0)
    assert np.array_equal(out[0], f32([0, 1, 0, 0])) and np.array_equal(out[1], f32([1, 0, 0, 0]))
    s = f32(f32(f32(0.025) + f32(0.9)) + f32(0.075))
    assert np.array_equal(out[2], f32([f32(0.025) / s, f32(0.9) / s, f32(0.075) / s, 0]))
    assert not out[3].any() and np.array_equal(out[4], post[4])
    assert np.array_equal(prune_posteriors_host(post, 0.025, 5.0)[4], post[4] * f32(5))
    zero = prune_posteriors_host(post, 0.0, 1.0)        # min_post = 0: nothing is dropped, every frame renormalised
    assert (zero[[0, 1, 2, 4]] > 0).sum() == 3 + 4 + 3 + 4 and not zero[3].any()
    assert np.array_equal(zero[0], f32([f32(0.01) / f32(0.035), f32(0.02) / f32(0.035), f32(0.005) / f32(0.035), 0]) * f32(1))


def test_pruning_twin_against_the_rule():
    rng = np.random.default_rng(1)
    for n in (1, 20, 64):
        raw = rng.random((500, n)).astype(f32) ** 4
        post = raw / raw.sum(axis=1, keepdims=True)
        post[::17] = 0
        for min_post, scale in ((0.025, 5.0), (0.3, 1.0), (0.0, 2.0)):
            assert np.array_equal(prune_posteriors_host(post, min_post, scale), R.prune(post, min_post, scale)), (n, min_post)
    nan = np.array([[np.nan, 0.5, 0.5], [np.nan, np.nan, 0.01], [np.nan, np.nan, np.nan]], f32)
    out = prune_posteriors_host(nan, 0.025, 1.0)
    assert np.array_equal(out, f32([[0, 0.5, 0.5], [0, 0, 1], [0, 0, 0]]))


# ---- utterance statistics -----------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 200)


@pytest.mark.parametrize("G,D,n", ((1, 1, 1), (5, 13, 20), (65, 48, 64), (256, 13, 20)))
def test_statistics_twin_against_float64(G, D, n):
    x, off, gs, p = R.random_case(G, D, n, LENGTHS, seed=G)
    ref = R.utt_stats(x, off, gs, p, G)
    gamma, X, S = ivector_utterance_statistics_host(x, off, gs, p, G, want_S=True)
    R.check_utt_stats(gamma, X, S, ref, f"host twin G {G} D {D} n {n}")
    assert not gamma[0].any() and not X[0].any()
    cap = float(np.median(ref["gamma"].sum(axis=1)))
    refc = R.utt_stats(x, off, gs, p, G, max_count=cap)
    gc, Xc, _ = ivector_utterance_statistics_host(x, off, gs, p, G, max_count=cap)
    R.check_utt_stats(gc, Xc, None, refc, "host twin with max_count", capped=True)
    assert (gc.sum(axis=1) <= cap * (1 + (G + 4) * R.u)).all() and np.array_equal(gc[1], gamma[1])


def test_statistics_twin_exact_on_integer_data():
    x, off, gs, p = R.random_case(65, 13, 20, LENGTHS, seed=3, integer=True)
    ref = R.utt_stats(x, off, gs, p, 65)
    gamma, X, S = ivector_utterance_statistics_host(x, off, gs, p, 65, want_S=True)
    assert np.array_equal(gamma, ref["gamma"]) and np.array_equal(X, ref["X"]) and np.array_equal(S, ref["S"])
    again = ivector_utterance_statistics_host(x, off, gs, p, 65, S=S.copy())[2]      # S is added to
    assert np.array_equal(again, 2 * S)


# ---- E-step -------------------------------------------------------------------------------------------------------------------
def _estep_case(G, D, Rd, lengths, seed=0):
    x, off, gs, p = R.random_case(G, D, min(G, 4), lengths, seed=seed)
    gamma, X, S = ivector_utterance_statistics_host(x, off, gs, p, G, want_S=True)
    return R.random_model(G, D, Rd, seed), gamma, X, S


@pytest.mark.parametrize("G,D,Rd", ((4, 3, 1), (4, 3, 5), (8, 13, 16), (8, 13, 17), (5, 7, 40), (4, 3, 192)))
def test_estep_twin_against_float64(G, D, Rd):
    lengths = (30, 0, 1) if Rd == 192 else (30, 0, 1, 65, 120)
    model, gamma, X, S = _estep_case(G, D, Rd, lengths, seed=Rd)
    refs = R.estep(model, gamma, X)
    st = IV.IvectorStats.zeros(G, D, Rd)
    mean, var, aux = ivector_estep_host(model, gamma, X, into=st, want_var=True)
    R.check_estep(mean, var, refs, model, f"host twin R {Rd}")
    acc, mag, n = R.accumulate(model, gamma, X, mean, var)
    R.check_accumulators(st, acc, mag, n, f"host twin R {Rd}")
    assert n == len(lengths) - 1
    # the empty utterance: the prior's own mean, the identity, log det 0
    assert np.array_equal(mean[1], np.eye(Rd)[0] * model.prior_offset) and np.array_equal(var[1], pack_lower(np.eye(Rd)))
    assert aux[1, 1] == 0.0
    # extraction: the same mean without accumulators
    assert R.bits(ivector_estep_host(model, gamma, X)[0]) == R.bits(mean)
    # the objective's pieces
    for r, a in zip(refs, aux):
        assert abs(a[1] - np.linalg.slogdet(r["Q"])[1]) <= 1e-9 * max(1.0, abs(a[1]))


def test_estep_twin_keeps_a_nan_utterance_to_itself():
    model, gamma, X, S = _estep_case(4, 3, 5, (30, 20, 10))
    clean = ivector_estep_host(model, gamma, X, want_var=True)
    g2, X2 = gamma.copy(), X.copy()
    X2[1, 2, 1] = np.nan
    st = IV.IvectorStats.zeros(4, 3, 5)
    mean, var, aux = ivector_estep_host(model, g2, X2, into=st, want_var=True)
    assert np.isnan(mean[1]).all() and R.bits(mean[[0, 2]], var[[0, 2]]) == R.bits(clean[0][[0, 2]], clean[1][[0, 2]])
    assert st.n == 2 and np.isfinite(st.Rq).all() and np.isfinite(st.Y).all() and np.isfinite(st.iscat).all()


def test_twins_refuse_what_the_contract_excludes():
    lib = _lib.lib()
    d, f, g = np.zeros(64), np.zeros(64, f32), np.zeros(64, np.int32)
    one = np.array([0, 1], np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    utt = lambda D, G, n, gam=d: lib.mfa_debug_ivector_utt_stats_host(p(f), p(one), 1, D, G, n, p(g), p(f), 0.0, p(gam), p(d), None)
    assert utt(3, 4, 2) == 0 and utt(0, 4, 2) == -2 and utt(49, 4, 2) == -2 and utt(1, 0, 2) == -3 and utt(1, 2049, 2) == -3
    assert utt(1, 4, 0) == -4 and utt(1, 4, 65) == -4 and utt(1, 4, 2, gam=None) == -1
    es = lambda Rd, mean=d, acc=(None,) * 6: lib.mfa_debug_ivector_estep_host(p(d), p(d), 1, 1, 1, Rd, p(d), p(d), 1.0, p(mean), None, None,
                                                                              *(p(a) for a in acc))
    assert es(1) == 0 and es(0) == -6 and es(193) == -6 and es(1, mean=None) == -1 and es(1, acc=(d, None, None, None, None, None)) == -1
    assert lib.mfa_debug_ivector_prune_post_host(p(f), 2, 65, 0.0, 1.0, p(f)) == -4
    assert lib.mfa_debug_ivector_prune_post_host(p(f), 2 ** 31, 4, 0.0, 1.0, p(f)) == -5


# ---- host layer ---------------------------------------------------------------------------------------------------------------
def test_initialisation_known_answers():
    from montreal_forced_aligner_amd import ubm as U
    ubm = U.DiagUbm.from_parameters([0.25, 0.75], [[1.0, -2.0, 4.0], [0.5, 0.0, -1.0]], [[1.0, 4.0, 0.25], [2.0, 0.5, 1.0]])
    m = IV.IvectorExtractorModel.from_diag_ubm(ubm, 3, np.random.default_rng(0))
    assert m.prior_offset == 100.0 and np.allclose(m.M[:, :, 0] * 100.0, ubm.means, rtol=1e-7)
    assert np.array_equal(m.sigma_inv[0], np.diag(ubm.inv_vars[0].astype(np.float64))) and np.array_equal(m.w_vec, ubm.weights.astype(np.float64))
    draws = np.random.default_rng(0).standard_normal((2, 3, 3))
    assert np.array_equal(m.M[:, :, 1:], draws[:, :, 1:])
    W, Up = m.derived()
    assert np.allclose(W[1], m.sigma_inv[1] @ m.M[1]) and np.allclose(unpack_lower(Up, 3)[0], m.M[0].T @ m.sigma_inv[0] @ m.M[0])
    with pytest.raises(ValueError):
        IV.IvectorExtractorModel.from_diag_ubm(ubm, 193)


def test_ie_round_trip_and_packed_io(tmp_path):
    m = R.random_model(5, 4, 3, seed=9)
    m.write(tmp_path / "a.ie")
    back = IV.IvectorExtractorModel.read(tmp_path / "a.ie")
    assert R.bits(back.M, back.sigma_inv, back.w_vec) == R.bits(m.M, m.sigma_inv, m.w_vec) and back.prior_offset == m.prior_offset
    buf = io.BytesIO()
    tri = np.arange(10.0)
    kaldi_io.write_sp_matrix(buf, tri, 4)
    kaldi_io.write_sp_matrix(buf, tri.astype(f32), 4)
    kaldi_io.write_double(buf, 2.5)
    r = kaldi_io.BinaryReader(buf.getvalue())
    a, b = kaldi_io.read_sp_matrix(r), kaldi_io.read_sp_matrix(r)
    assert a.dtype == np.float64 and b.dtype == f32 and np.array_equal(a, tri) and np.array_equal(b, tri) and r.float32() == 2.5
    full = unpack_lower(tri, 4)
    assert full[2, 1] == full[1, 2] == 4.0 and np.array_equal(pack_lower(full), tri)
    post = [[(3, 0.5), (1, 0.5)], [], [(7, 1.0)]]
    kaldi_io.write_table(tmp_path / "post.ark", [("utt-a", post), ("utt-b", [])], "posterior")
    assert dict(kaldi_io.read_ark((tmp_path / "post.ark").read_bytes(), "posterior")) == {"utt-a": post, "utt-b": []}


def test_stats_are_additive():
    model, gamma, X, S = _estep_case(4, 3, 5, (30, 20, 10, 40))
    whole = IV.IvectorStats.zeros(4, 3, 5)
    ivector_estep_host(model, gamma, X, into=whole)
    a, b = IV.IvectorStats.zeros(4, 3, 5), IV.IvectorStats.zeros(4, 3, 5)
    ivector_estep_host(model, gamma[:2], X[:2], into=a)
    ivector_estep_host(model, gamma[2:], X[2:], into=b)
    a += b
    assert a.n == whole.n == 4
    for k in ("gamma", "Y", "Rq", "isum", "iscat"):
        assert np.allclose(getattr(a, k), getattr(whole, k), rtol=1e-13, atol=0)
    assert np.isclose(a.quad, whole.quad, rtol=1e-13) and np.isclose(a.logdet, whole.logdet, rtol=1e-13)
    with pytest.raises(ValueError):
        a += IV.IvectorStats.zeros(4, 3, 6)
    # continued on the twin, the chain of additions is the whole batch's, bit for bit
    c = IV.IvectorStats.zeros(4, 3, 5)
    ivector_estep_host(model, gamma[:2], X[:2], into=c)
    ivector_estep_host(model, gamma[2:], X[2:], into=c)
    assert R.bits(c.gamma, c.Y, c.Rq, c.isum, c.iscat) == R.bits(whole.gamma, whole.Y, whole.Rq, whole.isum, whole.iscat)


# ---- update on data from a known model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known():
    truth = R.true_model()
    x, off, comp = R.draw(truth)
    ubm = R.ubm_of(x, comp, truth.num_gauss)
    gamma, X, S = ivector_utterance_statistics_host(x, off, comp[:, None], np.ones((len(comp), 1), f32), truth.num_gauss, want_S=True)
    return dict(truth=truth, x=x, off=off, comp=comp, ubm=ubm, gamma=gamma, X=X, S=S)


def _em(known, model, iterations, **kw):
    objs, counts = [], []
    for _ in range(iterations):
        st = IV.IvectorStats.zeros(model.num_gauss, model.dim, model.ivector_dim)
        ivector_estep_host(model, known["gamma"], known["X"], into=st)
        st.S = known["S"]
        objs.append(IV.objective(model, st))
        model, *c = IV.update(model, st, **kw)
        counts.append(tuple(c))
    return model, objs, counts


def test_update_never_lowers_the_objective(known):
    start = IV.IvectorExtractorModel.from_diag_ubm(known["ubm"], 2, np.random.default_rng(0))
    model, objs, counts = _em(known, start, 6)
    print("objective per frame:", np.round(objs, 5), "counts", counts)
    assert all(c == (4, 0, 0) for c in counts)                          # every Gaussian updated, none skipped, nothing floored
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(objs, objs[1:]))   # EM's guarantee, over 5 updates
    truth_st = IV.IvectorStats.zeros(4, 3, 2)
    ivector_estep_host(known["truth"], known["gamma"], known["X"], into=truth_st)
    truth_st.S = known["S"]
    assert objs[-1] > objs[0] and objs[-1] <= IV.objective(known["truth"], truth_st) + 0.05


def test_objective_is_the_marginal_by_brute_force(known):
    """One utterance, R = 1: the integral over w by quadrature against the closed form."""
    truth = R.true_model(G=2, D=2, R=1, seed=3, offset=1.5)
    x, off, comp = R.draw(truth, n_utt=1, frames=(6, 6), seed=4)
    gamma, X, S = ivector_utterance_statistics_host(x, off, comp[:, None], np.ones((6, 1), f32), 2, want_S=True)
    st = IV.IvectorStats.zeros(2, 2, 1)
    ivector_estep_host(truth, gamma, X, into=st)
    st.S = S
    closed = IV.objective(truth, st) * 6
    w = np.linspace(-20, 20, 400001)
    sigma = np.linalg.inv(truth.sigma_inv)
    logp = -0.5 * (w - truth.prior_offset) ** 2 - 0.5 * np.log(2 * np.pi)
    for t in range(6):
        i = comp[t]
        d = x[t].astype(np.float64)[None, :] - w[:, None] * truth.M[i][:, 0][None, :]
        logp += -0.5 * np.einsum("wd,de,we->w", d, truth.sigma_inv[i], d) - 0.5 * np.linalg.slogdet(2 * np.pi * sigma[i])[1]
    mx = logp.max()
    e = np.exp(logp - mx)
    brute = mx + np.log(float((e[1:] + e[:-1]).sum()) * 0.5 * (w[1] - w[0]))
    assert abs(closed - brute) <= 1e-7 * abs(brute)


def test_prior_update_whitens_the_ivectors(known):
    start = IV.IvectorExtractorModel.from_diag_ubm(known["ubm"], 2, np.random.default_rng(0))
    model, _, _ = _em(known, start, 2)
    st = IV.IvectorStats.zeros(4, 3, 2)
    mean, var, _ = ivector_estep_host(model, known["gamma"], known["X"], into=st, want_var=True)
    V, offset = IV.prior_transform(st)
    # the i-vectors' distributions mapped by V: mean offset·e₀ and unit covariance, to the rounding of R-term products
    mu = mean @ V.T
    sc = np.einsum("ab,ubc,dc->uad", V, unpack_lower(var, 2), V) + mu[:, :, None] * mu[:, None, :]
    m = mu.mean(axis=0)
    C = sc.mean(axis=0) - np.outer(m, m)
    scale = np.abs(V).max() ** 2 * np.abs(unpack_lower(st.iscat, 2)).max() / st.n
    tol = (400 + 16) * R.u * max(scale, 1.0) * 4
    assert np.abs(m - offset * np.eye(2)[0]).max() <= tol and np.abs(C - np.eye(2)).max() <= tol
    # M_i·V⁻¹ with the new offset is what update returns
    new = IV.update(model, st, update_variances=False)[0]
    only_m = IV.update(model, st, update_variances=False, update_prior=False)[0]
    assert np.allclose(new.M, only_m.M @ np.linalg.inv(V), rtol=1e-12, atol=0) and new.prior_offset == offset


def test_a_rotation_of_the_ivector_space_leaves_the_objective_unchanged(known):
    """M_i·V⁻¹ for an orthogonal V that keeps e₀ is the same model in other coordinates."""
    truth = R.true_model(G=4, D=3, R=3, seed=8)
    x, off, comp = R.draw(truth, n_utt=30, seed=2)
    gamma, X, S = ivector_utterance_statistics_host(x, off, comp[:, None], np.ones((len(comp), 1), f32), 4, want_S=True)
    c, s = np.cos(0.7), np.sin(0.7)
    V = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    turned = IV.IvectorExtractorModel(truth.w_vec, truth.M @ np.linalg.inv(V), truth.sigma_inv, truth.prior_offset)
    objs = []
    for m in (truth, turned):
        st = IV.IvectorStats.zeros(4, 3, 3)
        ivector_estep_host(m, gamma, X, into=st)
        st.S = S
        objs.append(IV.objective(m, st))
    assert abs(objs[0] - objs[1]) <= 1e-12 * abs(objs[0])


def test_degenerate_reflection():
    """T·m already along e₀: the reflection is the identity."""
    st = IV.IvectorStats.zeros(1, 1, 3)
    st.n = 10.0
    m = np.array([4.0, 0.0, 0.0])
    C = np.diag([1.0, 1.0, 1.0])
    st.isum = m * st.n
    st.iscat = pack_lower(C + np.outer(m, m)) * st.n
    V, offset = IV.prior_transform(st)
    assert offset == pytest.approx(4.0, rel=1e-14) and np.allclose(np.abs(V), np.eye(3), atol=1e-14)
    assert np.allclose(V @ m, [4.0, 0, 0], atol=1e-13)
    st.isum = np.array([0.0, 3.0, 0.0]) * st.n                           # and the general case: e₁ is taken to e₀
    st.iscat = pack_lower(C + np.outer(st.isum / st.n, st.isum / st.n)) * st.n
    V, offset = IV.prior_transform(st)
    assert np.allclose(V @ (st.isum / st.n), [3.0, 0, 0], atol=1e-13) and np.allclose(V @ V.T, np.eye(3), atol=1e-13)


def test_update_skips_low_counts_and_floors(known):
    model = IV.IvectorExtractorModel.from_diag_ubm(known["ubm"], 2, np.random.default_rng(0))
    st = IV.IvectorStats.zeros(4, 3, 2)
    ivector_estep_host(model, known["gamma"], known["X"], into=st)
    st.S = known["S"]
    new, updated, skipped, floored = IV.update(model, st, gaussian_min_count=float(np.sort(st.gamma)[1]) + 1.0, update_prior=False)
    low = np.argsort(st.gamma)[:2]
    assert (updated, skipped) == (2, 2) and np.array_equal(new.M[low], model.M[low]) and np.array_equal(new.sigma_inv[low], model.sigma_inv[low])
    _, _, _, floored = IV.update(model, st, variance_floor_factor=50.0)
    assert floored > 0


# ---- trainer ------------------------------------------------------------------------------------------------------------------
def test_trainer_on_the_host_backend(known, tmp_path):
    off = known["off"]
    utts = [(f"utt{i:03d}", known["x"][off[i]: off[i + 1]]) for i in range(len(off) - 1)]
    known["ubm"].write(tmp_path / "final.dubm")
    seen = []
    tr = IvectorTrainer(num_iterations=3, subsample=1, ivector_dimension=2, num_gselect=2, min_post=0.025,
                        backend=IvectorHostBackend(batch_frames=4000))
    tr.on_statistics = lambda i, model, st: seen.append((i, st.n))
    tr.train(utts, tmp_path / "final.dubm", tmp_path)
    print("objective per frame:", np.round(tr.objectives, 5))
    assert len(tr.backend.batches) > 1 and seen == [(1, 400.0), (2, 400.0), (3, 400.0)]
    assert len(tr.objectives) == 3 and all(b >= a - 1e-9 * abs(a) for a, b in zip(tr.objectives, tr.objectives[1:]))
    assert all(c == (4, 0, 0) for c in tr.update_counts)
    final = IV.IvectorExtractorModel.read(tmp_path / "final.ie")
    assert R.bits(final.M, final.sigma_inv) == R.bits(tr.model.M, tr.model.sigma_inv) and final.prior_offset == tr.model.prior_offset
    assert sorted(p.name for p in tmp_path.glob("*.ie")) == ["1.ie", "2.ie", "3.ie", "4.ie", "final.ie"]
    with pytest.raises(ValueError):
        IvectorTrainer(backend=IvectorHostBackend()).train([], known["ubm"])


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------
def test_twins_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "ivector_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "ivector_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "ivector_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout
