"""The silhouette stage on the device against its host twin and the restatement: s, a, b and bj bit for bit on integer vectors with
the dot metric across the shapes and cluster layouts at which the consumer changes path; on random data the device under the
derived bound, and the twin run on the device's own stored scores (bit for bit for dot and plda, 1 ulp of the root allowed for
euclidean); scikit-learn; repeated runs and forced column passes; the refusals; ``noise="exclude"``."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import cluster as CL
from montreal_forced_aligner_amd import stats
from tests import hdbscan_ref as H
from tests import silhouette_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("sil", "a", "b", "bj")


def device(engine, metric, x, offsets, model=None, want_v=False):
    r = stats.silhouette(engine, metric, x, offsets, model, want_parts=True, want_v=want_v)
    return {k: (None if v is None or k == "code" else v.cpu().numpy()) for k, v in r.items()}


def blob_case(metric, n=300, D=50, seed=61):
    sizes = [n // 2, n // 4, n // 8, n - n // 2 - n // 4 - n // 8 - 1, 1]
    x, truth = H.blobs(sizes, D, seed, spread=2.0)
    order, offsets = R.sort_by_label(truth)
    x = np.ascontiguousarray(x[order])
    return (np.ascontiguousarray(stats._unit_rows(x)) if metric == "dot" else x), offsets, H.model(D, 5)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130, 300])
def test_exact_tier_equals_the_twin_bit_for_bit(engine, n):
    for D in (1, 3, 4, 5, 50):
        x = H.integer_points(n, D, 3000 * n + D)
        for name, offsets in R.layouts(n).items():
            dev, host = device(engine, "dot", x, offsets), stats.silhouette_host("dot", x, offsets, want_parts=True)
            for key in KEYS:
                assert np.array_equal(dev[key], host[key]), (D, name, key)


@pytest.mark.parametrize("metric", ["plda", "euclidean", "dot"])
def test_random_data_under_the_bound_and_the_twin_on_the_stored_matrix(engine, metric):
    x, offsets, model = blob_case(metric)
    bound, ref = R.bound(metric, x, offsets, model.psi, ulp_root=2)           # the device's root: 1 ulp allowed
    assert bound.max() <= 1e-9
    dev = device(engine, metric, x, offsets, model, want_v=True)
    err = np.abs(dev["sil"] - np.asarray(ref["s"], dtype=np.float64))
    print(f"{metric}: largest bound {bound.max():.3e}, largest error {err.max():.3e}")
    assert (err <= bound).all() and np.array_equal(dev["bj"], ref["bj"])
    v = dev["v"]
    assert np.isfinite(v).all() and np.array_equal(v, v.T)
    y_r, q_r, w_r = H.pair_form(metric, x, model.psi)
    assert (np.abs(v - H.scores(y_r, q_r, w_r)) <= H.pair_bound(metric, x, model.psi)).all()
    host = stats.silhouette_host(metric, x, offsets, model, want_parts=True, v=v)
    equal = all(np.array_equal(dev[k], host[k]) for k in KEYS)
    print(f"{metric}: device and twin on the stored scores bit-equal: {equal}")
    if metric != "euclidean":
        assert equal
    else:
        rb = R.root_bound(stats.score_to_distance("euclidean", v), offsets, ulps=1)
        gap = np.abs(dev["sil"] - host["sil"])
        print(f"euclidean: largest gap to the twin {gap.max():.3e}, its bound {rb.max():.3e}")
        assert (gap <= rb).all() and rb.max() <= 1e-12 and np.array_equal(dev["bj"], host["bj"])


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_against_scikit_learn(engine, metric):
    from sklearn.metrics import silhouette_samples, silhouette_score
    x, _ = H.blobs((100, 80, 70, 50), 50, 67, spread=2.0)
    labels = R.random_labels(300, 5, 68, noise=20, singleton=True)
    got = CL.silhouette_samples(x, labels, metric, engine=engine)
    np.testing.assert_allclose(got, silhouette_samples(x, labels, metric=metric), rtol=0, atol=1e-12)
    assert abs(CL.silhouette_score(x, labels, metric, engine=engine) - silhouette_score(x, labels, metric=metric)) <= 1e-12


def test_plda_through_the_cluster_layer_is_measured_from_the_smallest_distance(engine):
    x, offsets, model = blob_case("plda", n=120, D=16, seed=83)
    labels = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    bound, ref = R.bound("plda", x, offsets, model.psi, from_smallest=True)
    got = CL.silhouette_samples(x, labels, "plda", plda=model, engine=engine)
    assert bound.max() <= 1e-9 and (np.abs(got - np.asarray(ref["s"], dtype=np.float64)) <= bound).all()
    assert (np.abs(got) <= 1.0).all()
    host = CL.silhouette_samples(x, labels, "plda", plda=model, backend="host")
    assert (np.abs(got - host) <= 2 * bound).all()                      # each is within the bound of the restatement


def test_forced_passes_and_repeated_runs_give_the_same_bits(engine, monkeypatch):
    x, offsets, model = blob_case("euclidean", n=300, D=5, seed=77)
    runs = []
    for cols in (None, "64", "128", None):
        if cols is None:
            monkeypatch.delenv("MFA_PLDA_PASS_COLS", raising=False)
        else:
            monkeypatch.setenv("MFA_PLDA_PASS_COLS", cols)
        runs.append(device(engine, "euclidean", x, offsets, want_v=True))
    for r in runs[1:]:
        assert all(np.array_equal(r[k], runs[0][k]) for k in KEYS + ("v",))


def test_refusals_each_followed_by_a_good_call(engine):
    dev = engine.device
    x = torch.arange(12, dtype=torch.float64, device=dev).reshape(6, 2)
    good = torch.tensor([0, 3, 6], dtype=torch.int32, device=dev)
    sil = torch.zeros(6, dtype=torch.float64, device=dev)
    want = stats.silhouette_host("euclidean", x.cpu().numpy(), [0, 3, 6])["sil"]

    def off(values):
        return torch.tensor(values, dtype=torch.int32, device=dev)

    def refused(word, *args):
        with pytest.raises(_lib.MfaHipError, match=word):
            engine._launch_silhouette(*args)
        sil.zero_()
        engine._launch_silhouette(x, 1, None, good, sil, None, None, None, None)          # the context stays usable
        assert np.array_equal(sil.cpu().numpy(), want)

    wide = torch.zeros((3, 1025), dtype=torch.float64, device=dev)
    refused("dimension", wide, 1, None, off([0, 1, 3]), sil, None, None, None, None)
    refused("metric", x, 3, None, good, sil, None, None, None, None)
    refused("NULL", x, 0, None, good, sil, None, None, None, None)                       # plda without psi
    refused("psi", x, 0, torch.tensor([1.0, -2.0], dtype=torch.float64, device=dev), good, sil, None, None, None, None)
    refused("clusters", x, 1, None, off([0, 6]), sil, None, None, None, None)              # C = 1
    refused("clusters", x, 1, None, off(list(range(8))), sil, None, None, None, None)      # C = 7 > N
    refused("offsets", x, 1, None, off([0, 3, 3, 6]), sil, None, None, None, None)         # an empty cluster
    refused("offsets", x, 1, None, off([1, 3, 6]), sil, None, None, None, None)
    refused("offsets", x, 1, None, off([0, 3, 5]), sil, None, None, None, None)
    refused("offsets", x, 1, None, off([0, 4, 2, 6]), sil, None, None, None, None)
    refused("offsets", x, 1, None, off([0, -5, 6]), sil, None, None, None, None)
    refused("offsets", x, 1, None, off([0, 2000000000, 6]), sil, None, None, None, None)
    refused("NULL", x, 1, None, good, None, None, None, None, None)
    lib = _lib.lib()
    assert lib.mfa_silhouette_batch(engine.ctx, None, 1 << 31, 2, 1, None, None, 2, None, None, None, None, None) != 0
    assert b"2^31" in lib.mfa_last_error(engine.ctx)
    assert lib.mfa_silhouette_batch(engine.ctx, None, 0, 2, 1, None, None, 0, None, None, None, None, None) == 0   # N == 0 writes nothing
    engine._launch_silhouette(x, 1, None, good, sil, None, None, None, None)
    assert np.array_equal(sil.cpu().numpy(), want)
    with pytest.raises(ValueError, match="Number of labels is 1"):
        CL.silhouette_samples(x.cpu().numpy(), [4] * 6, "euclidean", engine=engine)


def test_noise_exclude_through_the_cluster_layer(engine):
    x, truth = H.blobs((20, 20, 15), 4, 71, spread=6.0, strays=5)
    got = CL.silhouette_samples(x, truth, "euclidean", noise="exclude", engine=engine)
    host = CL.silhouette_samples(x, truth, "euclidean", noise="exclude", backend="host")
    assert np.isnan(got[truth == -1]).all() and np.array_equal(np.isnan(got), np.isnan(host))
    keep = truth != -1
    order, offsets = R.sort_by_label(truth[keep])
    bound = np.empty(keep.sum())
    bound[order] = R.bound("euclidean", x[keep][order], offsets, ulp_root=2)[0]
    assert (np.abs(got[keep] - host[keep]) <= 2 * bound).all() and bound.max() <= 1e-9
    assert CL.silhouette_score(x, truth, "euclidean", noise="exclude", engine=engine) == np.mean(got[keep])
