"""MLLT without a GPU: the host twin of the statistics (mfa_debug_mllt_acc_host) against the float64 restatement of
tests/mllt_ref.py — bit-equal where the contract makes every sum exact, under the derived bound where posteriors are soft —,
``mllt.mllt_accs`` against the brute-force triple loop, ``mllt.estimate_mllt`` against the properties of the row update
(monotone, the auxiliary function's gain, EM's guarantee on generated data, stationarity), ``transform_means`` /
``compose_transforms``, the twin's translation unit under the host sanitizers as a stand-alone program (nothing is preloaded
anywhere), and ``LdaTrainer`` with an MLLT schedule on a host backend."""
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib, adapt, kaldi_io, mllt
from montreal_forced_aligner_amd.stats import MlltStats, gaussian_means, gmm_statistics_host, mllt_statistics_host, silence_weights
from tests import gmm_acc_ref as R
from tests import gmm_ref, helpers
from tests import mllt_ref as MR

ROOT = Path(__file__).resolve().parents[1]
CHUNK = int(_lib.lib().mfa_mllt_acc_chunk_frames())


def host(case, **kw):
    return mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights, **kw)


# ---- the twin against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 8, 13, 16, 17, 40, 48))
def test_twin_is_bit_equal_on_integer_cases(dim):
    counts = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 7, 130] if dim in (13, 48) else [0, 1, 63, 64, 65, 7, 130]
    case = MR.integer_case(dim, counts)
    st = host(case)
    occ, full = MR.integer_expect(case)
    assert st.occ.tobytes() == occ.tobytes() and st.full.tobytes() == full.tobytes()
    assert st.tot_count == float(sum(counts)) and np.isfinite(st.tot_like)
    assert not st.full[0].any()                                            # the pdf without a frame


@pytest.mark.parametrize("dim", (13, 40, 48))
def test_twin_is_bit_equal_on_one_hot_mixtures(dim):
    case, gauss = MR.one_hot_case(dim, (40, 60, 77, 150, 90, 120, 200))
    st, post = host(case, want_post=True)
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    expect = np.zeros_like(post)
    expect[np.arange(len(gauss)), gauss - case.am.pdf_offsets[pdf]] = fw
    assert np.array_equal(post, expect), "host twin: posteriors are not exactly one-hot"
    occ, full = MR.one_hot_expect(case, gauss)
    assert st.occ.tobytes() == occ.tobytes() and st.full.tobytes() == full.tobytes()


@pytest.mark.parametrize("dim", gmm_ref.DIMS_SKEWED)
def test_twin_soft_posteriors_under_the_derived_bound(dim):
    case = R.skewed_case(dim)
    st = host(case)
    ref = MR.check_against_float64(case, st, f"host twin, {case.name}")
    assert ref["n_frames"].max() >= 700
    # occ and tot are the GMM statistics twin's, bit for bit
    g = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    assert st.occ.tobytes() == g.occ.tobytes() and (st.tot_like, st.tot_count) == (g.tot_like, g.tot_count)


def test_frames_that_take_no_part_leave_no_trace():
    case = R.skewed_case(40)
    rng = np.random.default_rng(5)
    G, D, n_tids = case.am.num_gauss, case.am.dim, len(case.weights)
    sym = rng.normal(size=(G, D, D))
    start = MlltStats(rng.normal(size=G), sym + np.swapaxes(sym, 1, 2), 3.25, 7.5)
    P = case.am.num_pdfs
    # id 0, ids outside the table (either side), an id of weight 0; then a table that names a pdf the model lacks
    ali = np.concatenate([np.zeros(50), np.full(50, n_tids), np.full(50, n_tids + 1000), np.full(50, -3), np.full(50, 4)]).astype(np.int32)
    assert case.weights[4] == 0
    feats = np.full((len(ali), D), np.nan, np.float32)          # never read
    st = mllt_statistics_host(case.am, feats, ali, case.tm, case.weights, into=start.copy())
    assert st.occ.tobytes() == start.occ.tobytes() and st.full.tobytes() == start.full.tobytes()
    assert (st.tot_like, st.tot_count) == (3.25, 7.5)
    more = helpers.fmllr_tm(P + 1)                              # transition-ids 2P + 1, 2P + 2: pdf P, which the model lacks
    st = mllt_statistics_host(case.am, feats[:20], np.full(20, 2 * P + 1, np.int32), more, None, into=start.copy())
    assert st.occ.tobytes() == start.occ.tobytes() and st.full.tobytes() == start.full.tobytes() and st.tot_count == 7.5
    # and with real frames in between: the same bits as without the odd ones
    keep = R.frame_tables(case.tm, case.ali, case.weights)[0] >= 0
    full = host(case)
    only = mllt_statistics_host(case.am, case.feats[keep], case.ali[keep], case.tm, case.weights)
    assert full.full.tobytes() == only.full.tobytes() and full.occ.tobytes() == only.occ.tobytes()
    assert (full.tot_like, full.tot_count) == (only.tot_like, only.tot_count)


def test_into_and_iadd_add_up():
    case, _gauss = MR.one_hot_case(13, (40, 60, 77, 150, 90, 120, 200))    # exact sums: adding up is bit-equal
    whole = host(case)
    cut = 311
    half = mllt_statistics_host(case.am, case.feats[:cut], case.ali[:cut], case.tm, case.weights)
    rest = mllt_statistics_host(case.am, case.feats[cut:], case.ali[cut:], case.tm, case.weights)
    into = mllt_statistics_host(case.am, case.feats[cut:], case.ali[cut:], case.tm, case.weights, into=half.copy())
    assert into.full.tobytes() == whole.full.tobytes() and into.occ.tobytes() == whole.occ.tobytes()
    assert into.tot_count == whole.tot_count
    total = half.copy()
    total += rest
    assert total.full.tobytes() == whole.full.tobytes() and total.occ.tobytes() == whole.occ.tobytes()
    assert total.tot_count == whole.tot_count and abs(total.tot_like - whole.tot_like) <= 1e-9 * abs(whole.tot_like)
    assert half.tot_count + rest.tot_count == whole.tot_count and half.full.tobytes() != whole.full.tobytes()
    assert whole.loglike_per_frame == whole.tot_like / whole.tot_count
    z = MlltStats.zeros(3, 4)
    assert z.shape == (3, 4, 4) and z.loglike_per_frame == 0.0
    with pytest.raises(ValueError, match="different models"):
        z += MlltStats.zeros(3, 5)


def test_twin_refusals():
    lib = _lib.lib()
    assert lib.mfa_mllt_acc_max_dim() == 48 and CHUNK >= 64 and CHUNK % int(lib.mfa_gmm_acc_chunk_frames()) == 0
    rng = np.random.default_rng(1)
    big = helpers.random_gmm(rng, 5, [129])
    with pytest.raises(_lib.MfaHipError, match="128"):
        mllt_statistics_host(big, np.zeros((1, 5), np.float32), np.array([1], np.int32), helpers.fmllr_tm(1))
    wide = helpers.random_gmm(rng, 49, [2])
    with pytest.raises(_lib.MfaHipError, match="48"):
        mllt_statistics_host(wide, np.zeros((1, 49), np.float32), np.array([1], np.int32), helpers.fmllr_tm(1))
    ok = helpers.random_gmm(rng, 5, [2, 3])
    with pytest.raises(ValueError, match="into"):
        mllt_statistics_host(ok, np.zeros((1, 5), np.float32), np.array([1], np.int32), helpers.fmllr_tm(2), into=MlltStats.zeros(5, 6))
    with pytest.raises(_lib.MfaHipError, match="features"):
        mllt_statistics_host(ok, np.zeros((2, 5), np.float32), np.array([1], np.int32), helpers.fmllr_tm(2))
    assert lib.mfa_debug_mllt_acc_host(0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, None, 0) == -1
    with pytest.raises(ValueError, match=r"\[G\] and \[G, D, D\]"):
        MlltStats(np.zeros(3), np.zeros((3, 4, 5)))


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "mllt_acc_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "mllt_acc_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "mllt_acc_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout


# ---- mllt_accs ------------------------------------------------------------------------------------------------------------------
def test_mllt_accs_against_the_triple_loop():
    rng = np.random.default_rng(11)
    D, sizes = 6, [3, 1, 4]
    am = helpers.random_gmm(rng, D, sizes)
    pdfs = rng.integers(0, len(sizes), size=90)
    feats = helpers.fmllr_draw(rng, am, pdfs)
    ali = (2 * pdfs + 1).astype(np.int32)
    tm = helpers.fmllr_tm(len(sizes))
    st, post = mllt_statistics_host(am, feats, ali, tm, want_post=True)
    beta, G = mllt.mllt_accs(st, am)
    mu, iv = gaussian_means(am), am.inv_vars.astype(np.float64)
    want, occ = np.zeros((D, D, D)), 0.0
    for t in range(len(ali)):
        g0 = int(am.pdf_offsets[pdfs[t]])
        for g in range(sizes[pdfs[t]]):
            gamma = float(post[t, g])
            d = (feats[t] - mu[g0 + g]).astype(np.float64)
            occ += gamma
            for j in range(D):
                want[j] += gamma * iv[g0 + g, j] * np.outer(d, d)
    assert abs(beta - occ) <= 1e-12 * occ
    assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
    raw = adapt.raw_from_soa(am)                                # a RawAmDiagGmm is taken as well
    assert np.array_equal(mllt.mllt_accs(st, raw)[1], G)
    with pytest.raises(ValueError, match="do not fit"):
        mllt.mllt_accs(MlltStats.zeros(3, D), am)


# ---- estimate_mllt --------------------------------------------------------------------------------------------------------------
def generated(D, n_gauss, frames, seed, spread=1.0):
    """x = A z with Gaussian-dependent diagonal covariances of z; the model's means and (diagonal) variances are the data's
    own, per generating Gaussian.  Returns (x [T, D], labels [T], weights [n], means [n, D], vars [n, D])."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(D, D)) + 2.0 * np.eye(D)
    lab = rng.integers(0, n_gauss, size=frames)
    m = spread * rng.normal(size=(n_gauss, D))
    v = np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=(n_gauss, D)))
    z = m[lab] + np.sqrt(v[lab]) * rng.normal(size=(frames, D))
    x = z @ A.T
    means = np.stack([x[lab == g].mean(axis=0) for g in range(n_gauss)])
    var = np.stack([x[lab == g].var(axis=0) for g in range(n_gauss)])
    w = np.bincount(lab, minlength=n_gauss) / frames
    return x, lab, w, means, var


def component_loglikes(x, w, means, var, Mat):
    """[T, n] log w_g + log N(M x; M μ_g, diag(var_g)) + log|det M|: the density of x under the transformed model."""
    y, mu = x @ Mat.T, means @ Mat.T
    logdet = np.linalg.slogdet(Mat)[1]
    d2 = ((y[:, None, :] - mu[None]) ** 2 / var[None]).sum(axis=2)
    return np.log(w)[None] - 0.5 * (x.shape[1] * np.log(2 * np.pi) + np.log(var).sum(axis=1)[None] + d2) + logdet


def accs_of(x, post, means, var):
    full = np.stack([((post[:, g, None] * (x - means[g])).T @ (x - means[g])) for g in range(means.shape[0])])
    st = MlltStats(post.sum(axis=0), full)
    return mllt.mllt_accs(st, SimpleNamespace(inv_vars=1.0 / var, pdf_offsets=np.array([0, means.shape[0]])))


def residual(beta, G, Mat):
    """max_j ‖beta·(M⁻ᵀ)_j − G_j m_j‖ / ‖G_j m_j‖: zero at a stationary point of the auxiliary function."""
    C = np.linalg.inv(Mat).T
    return max(np.linalg.norm(beta * C[j] - G[j] @ Mat[j]) / np.linalg.norm(G[j] @ Mat[j]) for j in range(Mat.shape[0]))


@pytest.mark.parametrize("D", (5, 13, 40))
def test_estimate_hard_classes_gain_is_the_auxiliary_gain(D):
    x, lab, w, means, var = generated(D, 4, 3000 + 100 * D, 100 + D)
    post = np.eye(4)[lab]
    beta, G = accs_of(x, post, means, var)
    Mat, impr, count, trace = mllt.estimate_mllt(beta, G, dtype=np.float64)
    assert count == beta == len(lab) and len(trace) == 200 and trace[-1] == impr
    assert all(b >= a for a, b in zip(trace, trace[1:])) and trace[0] > 0                 # non-decreasing
    q = mllt.objective(beta, G, Mat) - mllt.objective(beta, G, np.eye(D))
    assert abs(impr - q) <= 1e-9 * abs(q)
    # with hard classes the auxiliary function IS the log-likelihood: the actual gain per frame equals objf_impr / count
    ll = lambda Mt: component_loglikes(x, w, means, var, Mt)[np.arange(len(lab)), lab].mean()
    gain = ll(Mat) - ll(np.eye(D))
    print(f"D {D}: gain per frame {gain:.6f}, objf_impr / count {impr / count:.6f}")
    assert abs(gain - impr / count) <= 1e-10 * abs(gain)
    # the default result is the float32 rounding of the same matrix
    m32, impr32, _c, _t = mllt.estimate_mllt(beta, G)
    assert m32.dtype == np.float32 and np.array_equal(m32, Mat.astype(np.float32)) and impr32 == impr
    # stationarity: closer after 200 sweeps than after 20 (the ascent is slow: not asserted to be tiny)
    r200, r20 = residual(beta, G, Mat), residual(beta, G, mllt.estimate_mllt(beta, G, num_sweeps=20, dtype=np.float64)[0])
    print(f"D {D}: stationarity residual after 20 sweeps {r20:.3g}, after 200 {r200:.3g}")
    assert r200 < r20


@pytest.mark.parametrize("D", (5, 13, 40))
def test_estimate_soft_posteriors_em_guarantee(D):
    x, _lab, w, means, var = generated(D, 4, 3000 + 100 * D, 200 + D, spread=0.7)
    c = component_loglikes(x, w, means, var, np.eye(D))
    tot = np.logaddexp.reduce(c, axis=1)
    post = np.exp(c - tot[:, None])
    assert 0.02 < (post.max(axis=1) < 0.9).mean()                                         # really soft
    beta, G = accs_of(x, post, means, var)
    Mat, impr, count, _trace = mllt.estimate_mllt(beta, G, dtype=np.float64)
    gain = np.logaddexp.reduce(component_loglikes(x, w, means, var, Mat), axis=1).mean() - tot.mean()
    print(f"D {D}: true gain per frame {gain:.4f}, auxiliary gain {impr / count:.4f}")
    assert impr > 0 and gain >= impr / count - 1e-12 * abs(gain)


def test_estimate_scaled_identities_and_refusals():
    rng = np.random.default_rng(3)
    D, beta = 7, 1234.5
    g = rng.uniform(0.1, 9.0, size=D)
    G = beta * g[:, None, None] * np.eye(D)[None]
    Mat, impr, _count, _trace = mllt.estimate_mllt(beta, G, dtype=np.float64)
    assert np.abs(Mat - np.diag(g ** -0.5)).max() <= 1e-12
    assert abs(impr - (mllt.objective(beta, G, Mat) - mllt.objective(beta, G, np.eye(D)))) <= 1e-9 * abs(impr)
    before = G.copy()
    mllt.estimate_mllt(beta, G, num_sweeps=2)
    assert np.array_equal(G, before)                                                     # the caller's array is not touched
    with pytest.raises(ValueError, match="beta"):
        mllt.estimate_mllt(0.0, G)
    bad = G.copy()
    bad[3, 2, 2] = -1.0
    with pytest.raises(ValueError, match=r"G\[3\] is not positive definite"):
        mllt.estimate_mllt(beta, bad)
    with pytest.raises(ValueError, match="not \\[D, D, D\\]"):
        mllt.estimate_mllt(beta, G[:, :3])


# ---- transform_means and compose_transforms ---------------------------------------------------------------------------------------
def test_transform_means_and_compose_transforms():
    rng = np.random.default_rng(21)
    D = 9
    am = helpers.random_gmm(rng, D, [3, 1, 5])
    raw = adapt.raw_from_soa(am)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))                                          # orthogonal: |det| = 1
    new = mllt.transform_means(raw, Q.astype(np.float32))
    Q = Q.astype(np.float32).astype(np.float64)
    assert new.dim == D and [w.shape for w in new.weights] == [w.shape for w in raw.weights]
    u = 2.0 ** -24
    x = rng.normal(0, 3.0, size=(50, D))
    y = x @ Q.T
    for p in range(3):
        assert np.array_equal(new.inv_vars[p], raw.inv_vars[p]) and np.array_equal(new.weights[p], raw.weights[p])
        assert np.array_equal(new.gconsts[p], adapt.gconsts(new.weights[p], new.means_invvars[p], new.inv_vars[p]))
        iv = raw.inv_vars[p].astype(np.float64)
        mu = raw.means_invvars[p].astype(np.float64) / iv
        mu_new = new.means_invvars[p].astype(np.float64) / iv
        # means: M μ rounded to float32, then μ'·iv rounded to float32: two roundings of |μ'|
        assert (np.abs(mu_new - mu @ Q.T) <= 3 * u * np.abs(mu @ Q.T) + 1e-30).all()
        for g in range(mu.shape[0]):
            # x under mean μ and precision Mᵀ diag(iv) M (the normaliser is diag(iv)'s: |det M| = 1) …
            prec = Q.T @ np.diag(iv[g]) @ Q
            d = x - mu[g]
            want = np.log(float(raw.weights[p][g])) - 0.5 * (D * np.log(2 * np.pi) - np.log(iv[g]).sum()
                                                              + np.einsum("ta,ab,tb->t", d, prec, d))
            # … against M x under the transformed model as its float32 parameters define it
            got = float(new.gconsts[p][g]) + y @ new.means_invvars[p][g].astype(np.float64) - 0.5 * (y * y) @ iv[g]
            # the float32 roundings of μ' (3u·|μ'| per coordinate, weighted by iv·|y − μ'|, and by iv·|μ'| inside the gconst)
            # and of the gconst itself
            lim = (3 * u * iv[g] * np.abs(mu_new[g]) * (np.abs(y - mu_new[g]) + np.abs(mu_new[g]))).sum(axis=1) \
                + 2 * u * abs(float(new.gconsts[p][g])) + 1e-12
            assert (np.abs(got - want) <= lim).all(), (p, g, np.abs(got - want).max(), lim.min())
    with pytest.raises(ValueError, match="dimension 9"):
        mllt.transform_means(raw, np.eye(8))
    a, b = rng.normal(size=(D, D)), rng.normal(size=(D, 4 * D))
    c = mllt.compose_transforms(a.astype(np.float32), b.astype(np.float32))
    assert c.shape == (D, 4 * D) and c.dtype == np.float32
    assert np.array_equal(c, (a.astype(np.float32).astype(np.float64) @ b.astype(np.float32).astype(np.float64)).astype(np.float32))
    with pytest.raises(ValueError, match="affine"):
        mllt.compose_transforms(a, np.hstack([b, np.ones((D, 1))]), True)
    with pytest.raises(ValueError, match="not square"):
        mllt.compose_transforms(b, b)
    with pytest.raises(ValueError, match="does not apply"):
        mllt.compose_transforms(a, b.T)


# ---- LdaTrainer with an MLLT schedule on the host backend -----------------------------------------------------------------------------
def _host_backend(corpus):
    from tests import lda_case
    from tests import train_mono_case as TC
    from montreal_forced_aligner_amd.model import DiagGmmModel, TransitionModel

    class MlltHostBackend(lda_case.LdaHostBackend):
        """``LdaHostBackend`` plus the two calls of an MLLT iteration, on the twins."""

        def mllt_accumulate(self, raw_tm, raw_am):
            tm = TransitionModel(raw_tm)
            return mllt_statistics_host(DiagGmmModel.from_raw(raw_am), self.feats, np.concatenate(self.ali), tm,
                                        silence_weights(tm, TC.silence_ids(), 0.0))

        def set_transform(self, lda):
            self.set_lda(lda)

    return MlltHostBackend(corpus)


@pytest.fixture(scope="module")
def mono_model():
    from montreal_forced_aligner_amd.train import MonophoneTrainer
    from tests import train_mono_case as TC

    corpus = TC.train_corpus()
    mono = MonophoneTrainer(lexicon=corpus.world.lexicon, topology=TC.topology(), backend=TC.HostBackend(corpus),
                            silence_phones=TC.silence_ids(), num_iterations=6, max_gaussians=208).train()
    return corpus, mono


def _model_bytes(tr, tmp):
    return b"".join(p.read_bytes() for p in tr.write(tmp))


def test_lda_trainer_with_mllt_on_the_host_backend(mono_model, tmp_path):
    from montreal_forced_aligner_amd import train
    from tests import train_mono_case as TC

    corpus, mono = mono_model
    prev = (mono.raw_tm, mono.raw_am, mono.tree)
    assert train.REFERENCE_MLLT_ITERATIONS == (2, 4, 6, 12)
    kw = dict(lexicon=corpus.world.lexicon, previous=prev, silence_phones=TC.silence_ids(), max_gaussians=208)
    for bad in ((0,), (6,), (2, -1)):
        with pytest.raises(ValueError, match="mllt_iterations"):
            train.LdaTrainer(backend=_host_backend(corpus), num_iterations=5, mllt_iterations=bad, **kw)
    tr = train.LdaTrainer(backend=_host_backend(corpus), num_iterations=5, mllt_iterations=(2, 4), **kw)
    first = None

    def keep_first(lda, *a):
        nonlocal first
        first = np.array(lda, np.float32) if first is None else first

    set_lda = tr.backend.set_lda
    tr.backend.set_lda = lambda lda, *a: (keep_first(lda), set_lda(lda, *a))[1]
    tr.train()
    h = tr.history
    assert [e["iteration"] for e in h] == list(range(6))
    assert [("mllt" in e) for e in h] == [False, False, True, False, True, False]
    assert len(tr.mllt_mats) == 2 and all(m.shape == (40, 40) and m.dtype == np.float32 for m in tr.mllt_mats)
    for e in (h[2], h[4]):
        assert set(e["mllt"]) == {"objf_impr_per_frame", "logdet", "count"} and e["mllt"]["objf_impr_per_frame"] > 0
        assert 0 < e["mllt"]["count"] < e["frames"]                        # silence weighs 0 in the MLLT statistics only
    assert tr.logdet_total == h[2]["mllt"]["logdet"] + h[4]["mllt"]["logdet"]
    assert h[2]["mllt"]["logdet"] == float(np.linalg.slogdet(tr.mllt_mats[0].astype(np.float64))[1])
    # loglike + the log-determinants so far does not fall across an MLLT iteration (same alignments, no mix-up at this
    # schedule: em_violations' rule and allowance, on the comparable quantity)
    assert tr.realignment_iterations == [] and not any(e["mixed_up"] for e in h)
    run, comparable = 0.0, []
    for e in h:
        run += e["mllt"]["logdet"] if "mllt" in e else 0.0
        comparable.append(dict(e, loglike=e["loglike"] + run))
    checked, badits = TC.em_violations(comparable)
    print([(e["iteration"], round(e["loglike"], 4)) for e in comparable])
    assert checked == [1, 2, 3, 4, 5] and badits == []
    assert comparable[2]["loglike"] > comparable[1]["loglike"] and comparable[4]["loglike"] > comparable[3]["loglike"]
    # the written lda.mat is the product of the estimated matrices and the initial LDA
    want = mllt.compose_transforms(tr.mllt_mats[1], mllt.compose_transforms(tr.mllt_mats[0], first))
    paths = tr.write(tmp_path / "mllt")
    assert np.array_equal(kaldi_io.read_matrix_file(paths[2].read_bytes()), want) and np.array_equal(tr.lda_mat, want)
    assert not np.array_equal(want, first)
    _tm, raw_am = kaldi_io.read_model(paths[0].read_bytes())
    assert raw_am.dim == 40 and raw_am.num_pdfs == 208


def test_an_empty_schedule_is_the_loop_without_mllt(mono_model, tmp_path):
    from montreal_forced_aligner_amd import train
    from tests import lda_case
    from tests import train_mono_case as TC

    corpus, mono = mono_model
    kw = dict(lexicon=corpus.world.lexicon, previous=(mono.raw_tm, mono.raw_am, mono.tree), silence_phones=TC.silence_ids(),
              max_gaussians=208, num_iterations=2)
    # a backend WITHOUT the two MLLT calls: an empty schedule never asks for them
    plain = train.LdaTrainer(backend=lda_case.LdaHostBackend(corpus), **kw).train()
    empty = train.LdaTrainer(backend=_host_backend(corpus), mllt_iterations=(), **kw).train()
    assert plain.mllt_iterations == () and plain.history == empty.history and not any("mllt" in e for e in plain.history)
    assert plain.logdet_total == 0.0 and plain.mllt_mats == []
    assert _model_bytes(plain, tmp_path / "a") == _model_bytes(empty, tmp_path / "b")
    # the loop by hand, as it stood before the schedule existed: statistics → update, nothing in between
    hand = train.LdaTrainer(backend=lda_case.LdaHostBackend(corpus), **kw)
    hand._iterate = lambda failed, beam: None
    hand.train()
    for it in (1, 2):
        hand.iteration = it
        hand._update(hand.backend.accumulate(hand.raw_tm, hand.raw_am), hand.history[0]["failed"], False)
    assert hand.history == plain.history and _model_bytes(hand, tmp_path / "c") == _model_bytes(plain, tmp_path / "a")
