"""A numpy restatement of the HDBSCAN stage's contract (include/mfa_hip.h "HDBSCAN"), for tests/test_hdbscan_cpu.py and
tests/test_gpu_hdbscan.py: the pair form from its definition, the core scores by sorting rows, the spanning tree by Kruskal
under the edge order, and the bound that holds the pair form to the sweep's existing scores.

The bound.  Both forms compute the same real number as a sum of at most 3 D + 2 terms: the sweep's c_j + Σ p²A + Σ pB and
the pair form's (q_i + q_j) + w Σ y_i y_j with q a sum of D terms.  A term is a product of the inputs and of coefficients
that carry a few roundings each: for plda a_k, b_k and log1p come from plda_column_term (at most 8 roundings by its comment, 4
more allowed for log1p), √b_k adds one, the two scalings x √b one each, the product one: at most 16 per term; for euclidean and
dot at most 2.  A recursive sum of n terms adds n − 1 roundings to each (Higham, Accuracy and Stability, §4.2), here at most
3 D + 2, and the halvings and w are exact.  So each form is within γ_(3 D + 20) of the bracket
    B(i, j) = Σ |terms|  =  [½ Σ log1p] + Σ a p² + Σ a g² + w Σ |y_i y_j|      (a = ½ a_k for plda, 1 for euclidean, 0 for dot)
and the two differ by at most 2 γ_(3 D + 20) B ≤ γ_(6 D + 40) B.  Nothing here is taken from what the code returns.
"""
import numpy as np

U = 2.0 ** -53
CODES = {"plda": 0, "euclidean": 1, "dot": 2}


def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


def plda_coefficients(psi):
    """a_k, b_k and the constant c of one example against one: a = ψ²/((ψ+1)(2ψ+1)), b = ψ/(2ψ+1), c = ½ Σ log((1+ψ)²/(2ψ+1))."""
    psi = np.asarray(psi, dtype=np.float64)
    return psi * psi / ((psi + 1) * (2 * psi + 1)), psi / (2 * psi + 1), 0.5 * np.log((1 + psi) ** 2 / (2 * psi + 1)).sum()


def pair_form(metric, x, psi=None):
    """(y, q, w) from the definition; sums over k ascending."""
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    q = np.zeros(n)
    if metric == "dot":
        return x.copy(), q, 1.0
    if metric == "euclidean":
        for k in range(D):
            q = q + x[:, k] * x[:, k]
        return x.copy(), -q, 2.0
    a, b, c = plda_coefficients(psi)
    for k in range(D):
        q = q + a[k] * (x[:, k] * x[:, k])
    return x * np.sqrt(b)[None, :], 0.5 * c - 0.5 * q, 1.0


def scores(y, q, w):
    """v [n, n]: (q_i + q_j) + w · Σ_k y_ik y_jk, the sum from 0 over k ascending, one rounding a product and one a sum."""
    s = np.zeros((y.shape[0], y.shape[0]))
    for k in range(y.shape[1]):
        s = s + y[:, k][:, None] * y[:, k][None, :]
    return (q[:, None] + q[None, :]) + w * s


def bracket(metric, x, psi=None):
    x = np.asarray(x, dtype=np.float64)
    if metric == "dot":
        return np.abs(x) @ np.abs(x).T
    if metric == "euclidean":
        sq = (x * x).sum(axis=1)
        return sq[:, None] + sq[None, :] + 2.0 * (np.abs(x) @ np.abs(x).T)
    a, b, c = plda_coefficients(psi)
    sq = 0.5 * ((x * x) * a[None, :]).sum(axis=1)
    return abs(c) + sq[:, None] + sq[None, :] + (np.abs(x) * b[None, :]) @ np.abs(x).T


def pair_bound(metric, x, psi=None):
    return gamma(6 * np.shape(x)[1] + 40) * bracket(metric, x, psi)


def core(v, k: int):
    """The k-th largest finite off-diagonal entry of every row (−inf: fewer than k; k = 0: +inf)."""
    n = v.shape[0]
    out = np.full(n, np.inf if k == 0 else -np.inf)
    for i in range(n if k > 0 else 0):
        row = np.delete(v[i], i)
        row = np.sort(row[np.isfinite(row)])[::-1]
        if row.shape[0] >= k:
            out[i] = row[k - 1]
    return out


def kruskal(v, core_scores):
    """(lo, hi, m) of the spanning forest under the order: larger m, then smaller lo, then smaller hi; pairs with v finite only."""
    n = v.shape[0]
    iu, ju = np.triu_indices(n, 1)
    keep = np.isfinite(v[iu, ju])
    iu, ju = iu[keep], ju[keep]
    m = np.minimum(v[iu, ju], np.minimum(core_scores[iu], core_scores[ju]))
    order = np.lexsort((ju, iu, -m))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    lo, hi, ms = [], [], []
    for e in order.tolist():
        a, b = find(int(iu[e])), find(int(ju[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            lo.append(int(iu[e])); hi.append(int(ju[e])); ms.append(float(m[e]))
    return np.asarray(lo, np.int32), np.asarray(hi, np.int32), np.asarray(ms, np.float64)


# ---- the exact tier's inputs: integer vectors, every sum exact ------------------------------------------------------------------------
def grid(side: int = 6, D: int = 2):
    """The points of a square grid: very many equal distances, every tie rule of the edge order."""
    g = np.stack(np.meshgrid(*[np.arange(float(side))] * 2), axis=-1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((g.shape[0], D - 2))], axis=1) if D > 2 else g


def all_equal(n: int = 20, D: int = 3):
    return np.full((n, D), 3.0)


def path(n: int = 300, D: int = 1, seed=None):
    """n points on a line, gaps 1, 2, 3 repeating (so the tree is the path); ``seed``: in a random index order."""
    pos = np.cumsum(np.tile([1.0, 2.0, 3.0], n // 3 + 1)[:n])
    x = np.zeros((n, D))
    x[:, 0] = pos
    if seed is None:
        return x, np.arange(n)
    perm = np.random.default_rng(seed).permutation(n)
    return x[perm], perm


def integer_points(n: int, D: int, seed: int):
    return np.random.default_rng(seed).integers(-6, 7, size=(n, D)).astype(np.float64)


def blobs(sizes, D: int, seed: int, spread: float = 8.0, strays: int = 0):
    """Gaussian blobs with real coordinates (and uniform strays around them): (x, the blob of every point, −1 a stray)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((len(sizes), D)) * spread
    x = np.concatenate([centres[b] + rng.standard_normal((s, D)) for b, s in enumerate(sizes)])
    truth = np.repeat(np.arange(len(sizes)), sizes)
    if strays:
        x = np.concatenate([x, rng.uniform(-3 * spread, 3 * spread, (strays, D))])
        truth = np.concatenate([truth, np.full(strays, -1)])
    order = rng.permutation(x.shape[0])
    return x[order], truth[order]


def model(D: int, seed: int = 0):
    """What the plda metric needs of a model here: ψ (and the identity transform the device cache uploads with it)."""
    import types
    psi = np.exp(np.random.default_rng(seed).uniform(-2.0, 3.0, D))
    return types.SimpleNamespace(dim=D, psi=psi, transform=np.eye(D), offset=np.zeros(D))


def is_spanning_tree(n: int, lo, hi) -> bool:
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        ra, rb = find(a), find(b)
        if ra == rb or not a < b:
            return False
        parent[ra] = rb
    return len(lo) == n - 1


def same_partition(a, b) -> bool:
    """The same noise set and the same clusters up to their numbers."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[a >= 0].tolist()))
    return len(pairs) == len(set(a[a >= 0].tolist())) == len(set(b[b >= 0].tolist()))
