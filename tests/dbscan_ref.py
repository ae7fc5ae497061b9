"""DBSCAN restated in numpy on a boolean neighbour matrix, the direct form of every metric's distance, and the graphs that
tests/test_cluster_cpu.py and tests/test_gpu_dbscan.py share.  Nothing here imports the package.

The rules (include/mfa_hip.h "Clustering"): an edge is a pair that passes in either direction, the diagonal is set; a core
point has min_samples neighbours, itself included; clusters are the components of the core points over core-core edges,
numbered in ascending order of their smallest index; any other point takes the smallest number among its core neighbours,
−1 without one.  That is scikit-learn's DBSCAN on a precomputed matrix wherever no pair ties with ε."""
import numpy as np


def symmetrise(adj) -> np.ndarray:
    a = np.asarray(adj, dtype=bool)
    a = a | a.T
    np.fill_diagonal(a, True)
    return a


def dbscan(adj, min_samples: int):
    """dict(labels, core, count, n_clusters, adj) from a boolean [N, N] matrix (any: it is symmetrised first)."""
    a = symmetrise(adj)
    n = a.shape[0]
    count = a.sum(axis=1).astype(np.int32)
    core = count >= min_samples
    labels = np.full(n, -1, dtype=np.int32)
    nxt = 0
    for s in range(n):
        if not core[s] or labels[s] >= 0:
            continue
        labels[s] = nxt
        todo = [s]
        while todo:
            i = todo.pop()
            for j in np.flatnonzero(a[i] & core & (labels < 0)):
                labels[j] = nxt
                todo.append(int(j))
        nxt += 1
    for i in np.flatnonzero(~core):
        near = labels[a[i] & core]
        if near.size:
            labels[i] = near.min()
    return dict(labels=labels, core=core.astype(np.int32), count=count, n_clusters=nxt, adj=a)


def pack(adj) -> np.ndarray:
    """A boolean [N, M] matrix as uint64 words [N, ceil(M / 64)]: bit j & 63 of word j >> 6."""
    a = np.asarray(adj, dtype=bool)
    n, m = a.shape
    w = (m + 63) // 64
    padded = np.zeros((n, w * 64), dtype=np.uint8)
    padded[:, :m] = a
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n, w).astype(np.uint64)


def unpack(bits, m: int) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(bits)).view(np.uint64)
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")[:, :m].astype(bool)


def padding_bits(bits, m: int) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(bits)).view(np.uint64)
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")[:, m:]


# ---- the direct form of the distances -------------------------------------------------------------------------------------------
def euclidean(x, y) -> np.ndarray:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2))


def cosine(x, y) -> np.ndarray:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xn = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    yn = y / np.sqrt((y * y).sum(axis=1, keepdims=True))
    return 1.0 - xn @ yn.T


def plda(model, x, y, n=None) -> np.ndarray:
    """−LLR [x, y] by the model's direct formula (montreal_forced_aligner_amd.plda.PldaModel.log_likelihood_ratios)."""
    y = np.asarray(y, dtype=np.float64)
    n = np.ones(y.shape[0], dtype=np.int32) if n is None else n
    return -np.asarray(model.log_likelihood_ratios(y, n, np.asarray(x, dtype=np.float64)), dtype=np.float64)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def from_edges(n: int, edges) -> np.ndarray:
    a = np.zeros((n, n), dtype=bool)
    for i, j in edges:
        a[i, j] = True
    return a


def clique(members):
    return [(i, j) for i in members for j in members if i < j]


def hand_built():
    """name → (adjacency, min_samples, expected labels or None)."""
    g = {}
    # two cliques of 4 (core at min_samples 4) joined only through point 8, which has two neighbours: it stays a border
    # point, the cliques stay two clusters, and 8 takes the lower label
    e = clique([0, 1, 2, 3]) + clique([4, 5, 6, 7]) + [(3, 8), (8, 4)]
    g["joined_through_border"] = (from_edges(9, e), 4, [0, 0, 0, 0, 1, 1, 1, 1, 0])
    # point 4 is a border point with a core neighbour in either cluster: it takes the lower number
    e = clique([0, 1, 2, 3]) + clique([5, 6, 7, 8]) + [(8, 4), (4, 0)]
    g["border_between_two"] = (from_edges(9, e), 4, [0, 0, 0, 0, 0, 1, 1, 1, 1])
    g["all_noise"] = (from_edges(6, [(0, 1), (2, 3)]), 3, [-1] * 6)
    g["one_cluster"] = (from_edges(5, clique(range(5))), 3, [0] * 5)
    g["min_samples_1"] = (from_edges(5, [(0, 1), (3, 4)]), 1, [0, 0, 1, 2, 2])
    # duplicates: three copies of one point and two of another are cliques among themselves
    g["duplicates"] = (from_edges(6, clique([0, 2, 4]) + clique([1, 3])), 3, [0, -1, 0, -1, 0, -1])
    # asymmetric input: only one direction of every edge is present, and no diagonal
    g["asymmetric"] = (from_edges(6, [(1, 0), (1, 2), (2, 0), (4, 3), (5, 4), (3, 5)]), 3, [0, 0, 0, 1, 1, 1])
    return g


def random_graph(n: int, seed: int, density: float = None) -> np.ndarray:
    """An asymmetric random boolean matrix whose expected degree is a handful, so that core, border and noise points all occur."""
    rng = np.random.default_rng(seed)
    p = min(1.0, 2.5 / max(n, 1)) if density is None else density
    return rng.random((n, n)) < p


def path(n: int) -> np.ndarray:
    return from_edges(n, [(i, i + 1) for i in range(n - 1)])


SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)
