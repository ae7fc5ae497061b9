"""The i-vector extractor stage on the device (csrc/ivector.hip) at the shapes where the kernels can go wrong: G around the
blocks of 64 Gaussians, dims 1 – 48, lists of 1 – 64, utterance lengths around the tile of 64 frames (0 and 1 among them), R
around the 16-wide blocks of the matrix instruction and once at the limit of 192, 1 – 70 utterances around the chunks.

Pruning is the host twin's bit for bit (one function).  The statistics are exact on integer data — the twin's and float64's
bits — and within the bound of tests/ivector_ref.py of the longdouble restatement on real data.  The E-step is held to the exact
Q and lin through its residuals, to the twin within the distance two such solves can have, and its accumulators to the
longdouble sums of its own μ and Var; chunking and repetition must not change a bit."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import ivector as IV
from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.stats import (ivector_estep, ivector_estep_host, ivector_utterance_statistics,
                                               ivector_utterance_statistics_host, prune_posteriors, prune_posteriors_host)
from tests import ivector_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
LENGTHS = (0, 1, 63, 64, 65, 200)


def _dev(e, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def device_stats(engine, x, off, gs, p, G, **kw):
    gamma, X, S = ivector_utterance_statistics(engine, _dev(engine, x), off, _dev(engine, gs), _dev(engine, p), G, **kw)
    return gamma.cpu().numpy(), X.cpu().numpy(), None if S is None else S.cpu().numpy()


# ---- pruning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 20, 64))
def test_pruning_is_the_twins_bit_for_bit(engine, n):
    rng = np.random.default_rng(n)
    raw = rng.random((1000, n)).astype(f32) ** 4
    post = raw / raw.sum(axis=1, keepdims=True)
    post[::17] = 0
    post[5, 0] = np.nan
    for min_post, scale in ((0.025, 5.0), (0.3, 1.0), (0.0, 2.0)):
        want = prune_posteriors_host(post, min_post, scale)
        got = prune_posteriors(engine, _dev(engine, post), min_post, scale)
        assert R.bits(got.cpu().numpy()) == R.bits(want), (n, min_post)
        same = _dev(engine, post)
        assert prune_posteriors(engine, same, min_post, scale, inplace=True) is same and R.bits(same.cpu().numpy()) == R.bits(want)


# ---- utterance statistics -----------------------------------------------------------------------------------------------------
STAT_SHAPES = [(1, 1, 1), (5, 13, 20), (65, 48, 64), (256, 13, 20), (256, 48, 1), (65, 1, 64), (5, 48, 64), (1, 13, 20)]


@pytest.mark.parametrize("G,D,n", STAT_SHAPES)
def test_statistics_exact_on_integer_data(engine, G, D, n):
    x, off, gs, p = R.random_case(G, D, n, LENGTHS, seed=G + D, integer=True)
    want = ivector_utterance_statistics_host(x, off, gs, p, G, want_S=True)
    got = device_stats(engine, x, off, gs, p, G, want_S=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not got[0][0].any() and not got[1][0].any()                   # the utterance without frames


@pytest.mark.parametrize("G,D,n", STAT_SHAPES)
def test_statistics_within_the_bound_on_real_data(engine, G, D, n):
    x, off, gs, p = R.random_case(G, D, n, LENGTHS, seed=G + D)
    ref = R.utt_stats(x, off, gs, p, G)
    gamma, X, S = device_stats(engine, x, off, gs, p, G, want_S=True)
    R.check_utt_stats(gamma, X, S, ref, f"device G {G} D {D} n {n}")


def test_statistics_max_count(engine):
    x, off, gs, p = R.random_case(65, 13, 20, LENGTHS, seed=4)
    plain = R.utt_stats(x, off, gs, p, 65)
    cap = float(np.median(plain["gamma"].sum(axis=1)))
    ref = R.utt_stats(x, off, gs, p, 65, max_count=cap)
    gamma, X, _ = device_stats(engine, x, off, gs, p, 65, max_count=cap)
    R.check_utt_stats(gamma, X, None, ref, "device with max_count", capped=True)
    free = device_stats(engine, x, off, gs, p, 65)
    small = plain["gamma"].sum(axis=1) < cap * 0.99
    assert small.any() and R.bits(gamma[small], X[small]) == R.bits(free[0][small], free[1][small])


def test_scatter_added_in_two_calls_equals_one(engine, monkeypatch):
    slab = int(engine.lib.mfa_ivector_scatter_slab_frames())
    lengths = (slab // 2, slab - slab // 2, 500, 0, 700, slab + 3)
    x, off, gs, p = R.random_case(65, 13, 20, lengths, seed=8)
    one = device_stats(engine, x, off, gs, p, 65, want_S=True)[2]
    cut, t = 2, int(off[2])
    assert t == slab
    S = torch.zeros((65, 13 * 14 // 2), dtype=torch.float64, device=engine.device)
    ivector_utterance_statistics(engine, _dev(engine, x[:t]), off[: cut + 1], _dev(engine, gs[:t]), _dev(engine, p[:t]), 65, S=S)
    ivector_utterance_statistics(engine, _dev(engine, x[t:]), off[cut:] - t, _dev(engine, gs[t:]), _dev(engine, p[t:]), 65, S=S)
    assert R.bits(S.cpu().numpy()) == R.bits(one)
    monkeypatch.setenv("MFA_IVECTOR_PASS_SLABS", "1")                    # every slab a pass of its own
    assert R.bits(device_stats(engine, x, off, gs, p, 65, want_S=True)[2]) == R.bits(one)
    start = np.random.default_rng(0).normal(size=one.shape)             # S is added to, never overwritten
    monkeypatch.delenv("MFA_IVECTOR_PASS_SLABS")
    again = device_stats(engine, x[:0], off[:1], gs[:0], p[:0], 65, S=_dev(engine, start))[2]
    assert R.bits(again) == R.bits(start)


# ---- E-step -------------------------------------------------------------------------------------------------------------------
def estep_case(G, D, Rd, n_utt, seed=0):
    rng = np.random.default_rng(seed + 1000)
    lengths = [0 if i % 9 == 4 else int(rng.integers(1, 40)) for i in range(n_utt)]
    if n_utt == 1:
        lengths = [30]
    x, off, gs, p = R.random_case(G, D, min(G, 4), lengths, seed=seed)
    gamma, X, _ = ivector_utterance_statistics_host(x, off, gs, p, G)
    return R.random_model(G, D, Rd, seed), gamma, X


def device_estep(engine, model, gamma, X, into=None, want_var=True):
    mean, var, aux = ivector_estep(engine, model, _dev(engine, gamma), _dev(engine, X), into=into, want_var=want_var)
    return mean.cpu().numpy(), None if var is None else var.cpu().numpy(), aux.cpu().numpy()


@pytest.mark.parametrize("G,D,Rd,n_utt", ((4, 3, 1, 3), (8, 13, 5, 70), (65, 13, 16, 1), (8, 13, 17, 3), (5, 7, 40, 70), (4, 3, 192, 3)))
def test_estep_against_the_twin_and_float64(engine, G, D, Rd, n_utt):
    model, gamma, X = estep_case(G, D, Rd, n_utt, seed=Rd)
    refs = R.estep(model, gamma, X)
    st = IV.IvectorStats.zeros(G, D, Rd)
    mean, var, aux = device_estep(engine, model, gamma, X, into=st)
    R.check_estep(mean, var, refs, model, f"device R {Rd} U {n_utt}")
    twin_st = IV.IvectorStats.zeros(G, D, Rd)
    tmean, tvar, taux = ivector_estep_host(model, gamma, X, into=twin_st, want_var=True)
    worst = 0.0
    for un, r in enumerate(refs):
        bound = R.mean_distance_bound(r, tmean[un], tvar[un], model)
        dist = float(np.linalg.norm(mean[un] - tmean[un]))
        worst = max(worst, dist / bound)
        assert dist <= bound, (un, dist, bound)
        assert abs(aux[un, 1] - taux[un, 1]) <= R.logdet_distance_bound(r, model), un
    print(f"R {Rd} U {n_utt}: worst ‖μ_device − μ_twin‖ / bound = {worst:.3e}")
    acc, mag, n = R.accumulate(model, gamma, X, mean, var)
    R.check_accumulators(st, acc, mag, n, f"device R {Rd} U {n_utt}")
    assert st.n == twin_st.n == sum(1 for g in gamma if g.any())


def test_estep_chunks_and_repeats_give_equal_bits(engine, monkeypatch):
    model, gamma, X = estep_case(8, 13, 17, 70, seed=2)

    def run():
        st = IV.IvectorStats.zeros(8, 13, 17)
        st.gamma += 0.5; st.Rq += 0.25; st.Y -= 0.125; st.isum += 1.0; st.iscat += 2.0; st.n = 3.0     # added to, not overwritten
        mean, var, aux = device_estep(engine, model, gamma, X, into=st)
        return R.bits(mean, var, aux, st.gamma, st.Y, st.Rq, st.isum, st.iscat, np.array([st.n]))

    default = run()
    assert run() == default                                              # two calls, the same bits
    for chunk in ("1", "7"):
        monkeypatch.setenv("MFA_IVECTOR_PASS_UTTS", chunk)
        assert run() == default, chunk
    monkeypatch.delenv("MFA_IVECTOR_PASS_UTTS")
    st = IV.IvectorStats.zeros(8, 13, 17)
    device_estep(engine, model, gamma, X, into=st)
    assert st.n == sum(1 for g in gamma if g.any())


def test_accumulators_leave_the_means_alone(engine):
    model, gamma, X = estep_case(8, 13, 17, 70, seed=3)
    extraction = device_estep(engine, model, gamma, X, want_var=False)
    assert extraction[1] is None
    with_acc = device_estep(engine, model, gamma, X, into=IV.IvectorStats.zeros(8, 13, 17))
    assert R.bits(extraction[0], extraction[2]) == R.bits(with_acc[0], with_acc[2])


def test_empty_and_nan_utterances_disturb_no_neighbour(engine):
    model, gamma, X = estep_case(8, 13, 17, 7, seed=5)
    clean_st = IV.IvectorStats.zeros(8, 13, 17)
    keep = [0, 1, 3, 5, 6]
    clean = device_estep(engine, model, gamma[keep], X[keep], into=clean_st)
    g2, X2 = gamma.copy(), X.copy()
    g2[2], X2[2] = 0.0, 0.0                                              # an utterance without statistics
    X2[4, 3, 2] = np.nan                                                 # and one that is not finite
    st = IV.IvectorStats.zeros(8, 13, 17)
    mean, var, aux = device_estep(engine, model, g2, X2, into=st)
    assert R.bits(mean[keep], var[keep], aux[keep]) == R.bits(*clean)
    assert np.array_equal(mean[2], np.eye(17)[0] * model.prior_offset) and np.isnan(mean[4]).all()
    assert st.n == 5 and all(np.isfinite(a).all() for a in (st.gamma, st.Y, st.Rq, st.isum, st.iscat))
    # the five that take part sit in other steps of the products than in the clean batch: the sums agree to the bound
    acc, mag, n = R.accumulate(model, g2, X2, mean, var)
    R.check_accumulators(st, acc, mag, n, "with an empty and a NaN utterance")
    g3 = gamma.copy()
    g3[4, 1] = np.nan
    mean3, _, _ = device_estep(engine, model, g3, X)
    assert np.isnan(mean3[4]).all() and R.bits(mean3[keep]) == R.bits(clean[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_context_usable(engine):
    lib, ctx, dev = engine.lib, engine.ctx, engine.device
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    good = estep_case(4, 3, 5, 3)

    def usable():
        m, g, X = good
        assert np.isfinite(device_estep(engine, m, g, X)[0]).all()

    def refused(rc, word):
        assert rc != 0 and word in lib.mfa_last_error(ctx).decode(), lib.mfa_last_error(ctx)
        usable()

    f, gs = z(64, 64, dt=torch.float32), z(64, 64, dt=torch.int32)
    off = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    d = z(4096)
    utt = lambda D, G, n, feats=f, gamma=d: lib.mfa_ivector_utt_stats_batch(ctx, ptr(feats), ptr(off), 1, 1, D, G, n, ptr(gs), ptr(f), 0.0,
                                                                            ptr(gamma), ptr(d), None)
    refused(utt(0, 4, 2), "dim"); refused(utt(49, 4, 2), "dim")
    refused(utt(3, 0, 2), "Gaussians"); refused(utt(3, 2049, 2), "Gaussians")
    refused(utt(3, 4, 0), "entries"); refused(utt(3, 4, 65), "entries")
    refused(utt(3, 4, 2, feats=None), "NULL"); refused(utt(3, 4, 2, gamma=None), "NULL")
    refused(lib.mfa_ivector_utt_stats_batch(ctx, ptr(f), ptr(off), 1, 2 ** 31, 3, 4, 2, ptr(gs), ptr(f), 0.0, ptr(d), ptr(d), None), "2^31")
    refused(lib.mfa_ivector_prune_post_batch(ctx, ptr(f), 4, 65, 0.0, 1.0, ptr(f)), "entries")
    refused(lib.mfa_ivector_prune_post_batch(ctx, ptr(f), 2 ** 31, 4, 0.0, 1.0, ptr(f)), "2^31")
    refused(lib.mfa_ivector_prune_post_batch(ctx, ptr(f), 4, 4, 0.0, 1.0, None), "NULL")
    es = lambda D, G, Rd, mean=d, W=d, acc=(None,) * 6: lib.mfa_ivector_estep_batch(ctx, ptr(d), ptr(d), 1, D, G, Rd, ptr(W), ptr(d), 1.0,
                                                                                    ptr(mean), None, None, *(ptr(a) for a in acc))
    refused(es(3, 4, 0), "i-vector dimension"); refused(es(3, 4, 193), "i-vector dimension")
    refused(es(49, 4, 2), "dim"); refused(es(3, 2049, 2), "Gaussians")
    refused(es(3, 4, 2, mean=None), "NULL"); refused(es(3, 4, 2, W=None), "NULL")
    refused(es(3, 4, 2, acc=(d, d, d, None, d, d)), "accumulators")
    assert es(3, 4, 2) == 0 and lib.mfa_ivector_estep_batch(ctx, None, None, 0, 3, 4, 2, None, None, 1.0, None, None, None, *([None] * 6)) == 0
    with pytest.raises(MfaHipError):
        ivector_utterance_statistics(engine, f, np.array([0, 3]), gs, f, 4)      # offsets that do not end at the batch
    usable()
