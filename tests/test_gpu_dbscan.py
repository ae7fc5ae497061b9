"""DBSCAN on a neighbour bit matrix on the device (mfa_dbscan_from_bits) against its host twin, exactly: the symmetrised words,
labels, core flags, counts and the number of clusters, on the hand-built graphs of tests/dbscan_ref.py, on random graphs at
point counts around the word size, on a path (the largest diameter a graph of its size has), and on an input with stray
padding bits and a cleared diagonal; determinism; the refusals."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.stats import dbscan_from_bits, dbscan_from_bits_host
from tests import dbscan_ref as R

pytestmark = pytest.mark.gpu


def device_equals_twin(engine, words, min_samples, n=None):
    want = dbscan_from_bits_host(words, min_samples, n)
    got = dbscan_from_bits(engine, words, min_samples, n)
    assert np.array_equal(got["bits"].cpu().numpy().view(np.uint64), want["bits"])
    for key in ("labels", "core", "count"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    assert got["n_clusters"] == want["n_clusters"]
    return got, want


@pytest.mark.parametrize("name", sorted(R.hand_built()))
def test_hand_built_graphs(engine, name):
    adj, ms, labels = R.hand_built()[name]
    got, _ = device_equals_twin(engine, R.pack(adj), ms)
    assert got["labels"].cpu().tolist() == labels


@pytest.mark.parametrize("n", R.SIZES)
def test_random_graphs(engine, n):
    for seed in range(3):
        for ms in (1, 3, 5):
            adj = R.random_graph(n, 100 * n + seed)
            got, want = device_equals_twin(engine, R.pack(adj), ms)
            ref = R.dbscan(adj, ms)
            assert np.array_equal(want["labels"], ref["labels"]) and 1 <= got["rounds"] <= n + 1
    dense = R.random_graph(n, 7 * n, density=0.3)
    device_equals_twin(engine, R.pack(dense), 4)


def test_a_path_of_300_points(engine):
    """Every point a core point at min_samples 2, one component: the roots have 299 links to fall.  The rounds are recorded; only
    rounds ≤ N is asserted."""
    n = 300
    got, _ = device_equals_twin(engine, R.pack(R.path(n)), 2)
    assert got["labels"].cpu().tolist() == [0] * n and got["n_clusters"] == 1
    print(f"path of {n}: {got['rounds']} rounds")
    assert got["rounds"] <= n
    perm = np.random.default_rng(1).permutation(n)         # the same path with its points in random index order
    adj = np.zeros((n, n), dtype=bool)
    adj[perm[:-1], perm[1:]] = True
    got, _ = device_equals_twin(engine, R.pack(adj), 2)
    print(f"shuffled path of {n}: {got['rounds']} rounds")
    assert got["rounds"] <= n and got["n_clusters"] == 1
    got, _ = device_equals_twin(engine, R.pack(adj), 3)    # its end points are border points now
    assert got["n_clusters"] == 1 and (got["labels"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("n", [65, 129, 200])
def test_symmetrise_repairs_padding_and_diagonal(engine, n):
    adj = R.random_graph(n, n)
    np.fill_diagonal(adj, False)
    words = R.pack(adj)
    words[:, -1] |= ~np.uint64(0) << np.uint64(n % 64)     # every padding bit set
    got, _ = device_equals_twin(engine, words, 3)
    out = got["bits"].cpu().numpy().view(np.uint64)
    assert not R.padding_bits(out, n).any() and np.array_equal(R.unpack(out, n), R.symmetrise(adj))


def test_two_runs_give_the_same_result(engine):
    adj = R.random_graph(200, 5, density=0.02)
    a = dbscan_from_bits(engine, R.pack(adj), 3)
    b = dbscan_from_bits(engine, R.pack(adj), 3)
    for key in ("labels", "core", "count", "bits"):
        assert torch.equal(a[key], b[key])
    assert a["n_clusters"] == b["n_clusters"]           # the rounds are the schedule's, not the input's: they are not compared
    again = dbscan_from_bits(engine, a["bits"], 3)           # in place on an already symmetric matrix: nothing moves
    assert torch.equal(again["labels"], a["labels"]) and again["bits"].data_ptr() == a["bits"].data_ptr()


def test_refusals_leave_the_context_usable(engine):
    words = torch.from_numpy(R.pack(R.path(5)).view(np.int64)).to(engine.device)
    out = lambda: tuple(torch.empty(5, dtype=torch.int32, device=engine.device) for _ in range(3))
    for ms in (0, -2):
        with pytest.raises(MfaHipError, match="min_samples"):
            engine._launch_dbscan(words, 5, ms, *out())
    for n in (-1, 1 << 31):
        with pytest.raises(MfaHipError, match="points"):
            engine._launch_dbscan(words, n, 2, *out())
    with pytest.raises(MfaHipError, match="NULL array"):
        engine._launch_dbscan(None, 5, 2, *out())
    with pytest.raises(MfaHipError, match="NULL array"):
        engine._launch_dbscan(words, 5, 2, None, *out()[:2])
    with pytest.raises(MfaHipError, match="square"):
        dbscan_from_bits(engine, np.zeros((5, 2), dtype=np.uint64), 2)
    assert engine._launch_dbscan(None, 0, 2, None, None, None) == (0, 0)
    labels, core, count = out()
    assert engine._launch_dbscan(words, 5, 2, labels, core, count)[0] == 1 and labels.cpu().tolist() == [0] * 5
