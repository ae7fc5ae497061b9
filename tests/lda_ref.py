"""A float64 numpy restatement of the LDA statistics' contract (include/mfa_hip.h "LDA statistics") and of the estimate,
for tests/test_lda_cpu.py, tests/test_gpu_lda_acc.py and tests/test_gpu_lda_flow.py.  Spliced vectors come from the oracle
(``cmvn_apply`` then ``splice``), the prune draw is restated here in Python integers, the estimate is brute force on
``numpy.linalg``.  Test-side code: the package imports nothing from here or from oracle/."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from montreal_forced_aligner_amd.stats import LdaStats
from oracle import oracle as O

U64 = 2.0 ** -53
M32 = 0xFFFFFFFF
WEIGHT_SET = np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32)


def fmix(h: int) -> int:
    h &= M32
    h ^= h >> 16; h = (h * 0x85EBCA6B) & M32; h ^= h >> 13; h = (h * 0xC2B2AE35) & M32; h ^= h >> 16
    return h


def draw(seed: int, key: int, d: int) -> int:
    """Draw d of utterance `key` under `seed`: the construction of include/mfa_hip.h "Equal alignment"."""
    h = fmix((seed ^ 0x9E3779B9) & M32)
    h = fmix((h + key * 0x85EBCA6B + 0x165667B1) & M32)
    return fmix(h ^ ((d * 0xC2B2AE35 + 0x27D4EB2F) & M32))


def prune_weight(w: np.float32, theta: float, seed: int, key: int, d: int) -> np.float32:
    theta = np.float32(theta)
    w = np.float32(w)
    if not theta > 0 or w == 0 or not abs(w) < theta:
        return w
    r = np.float32(abs(w)) / theta
    u = np.float32(draw(seed, key, d) >> 8) * np.float32(2.0 ** -24)
    return np.float32(np.copysign(theta, w)) if u < r else np.float32(0.0)


@dataclass
class Case:
    """One batch as the statistics calls take it (host arrays)."""
    mfcc: np.ndarray            # float32 [ΣT, dim]
    frame_off: np.ndarray       # int64 [n_utt + 1]
    utt2spk: Optional[np.ndarray]
    cmvn: Optional[np.ndarray]  # float64 [n_spk, 2, dim + 1]
    ali: np.ndarray             # int32 [ΣT]
    tid2class: np.ndarray       # int32 [n_tids]
    tid_weight: np.ndarray      # float32 [n_tids]
    n_classes: int
    ctx: int

    @property
    def S(self) -> int:
        return (2 * self.ctx + 1) * int(self.mfcc.shape[1])

    @property
    def tables(self):
        return (self.tid2class, self.tid_weight)


def spliced(case: Case) -> np.ndarray:
    """float32 [ΣT, S]: per utterance the oracle's CMVN application and splice."""
    out = np.zeros((case.mfcc.shape[0], case.S), np.float32)
    for u in range(len(case.frame_off) - 1):
        a, b = int(case.frame_off[u]), int(case.frame_off[u + 1])
        if b == a:
            continue
        x = case.mfcc[a:b]
        if case.cmvn is not None:
            x = O.cmvn_apply(case.cmvn[case.utt2spk[u]], x)
        out[a:b] = O.splice(x, case.ctx, case.ctx)
    return out


def frame_tables(case: Case, rand_prune: float = 0.0, utt_keys=None, seed: int = 0):
    """(class int32 [ΣT] with −1 for frames that take no part, weight float32 [ΣT] after the prune)."""
    ali = case.ali.astype(np.int64)
    n_tids = len(case.tid2class)
    ok = (ali > 0) & (ali < n_tids)
    safe = np.where(ok, ali, 0)
    cls = np.where(ok, case.tid2class[safe], -1).astype(np.int64)
    w = np.where(ok, case.tid_weight[safe], np.float32(0)).astype(np.float32)
    ok &= (w != 0) & (cls >= 0) & (cls < case.n_classes)
    if rand_prune > 0:
        for u in range(len(case.frame_off) - 1):
            a, b = int(case.frame_off[u]), int(case.frame_off[u + 1])
            for t in range(a, b):
                if ok[t]:
                    w[t] = prune_weight(w[t], rand_prune, seed, int(utt_keys[u]), t - a)
        ok &= w != 0
    return np.where(ok, cls, -1).astype(np.int32), np.where(ok, w, np.float32(0)).astype(np.float32)


def statistics(case: Case, rand_prune: float = 0.0, utt_keys=None, seed: int = 0, want_abs: bool = False):
    """The sums in float64 by matrix products (another order than either implementation).  With ``want_abs`` also
    (Σ|w·x_i·x_j| [S, S], Σ|w·x_i| [C, S], frames that take part): what the summation bounds are made of."""
    cls, w = frame_tables(case, rand_prune, utt_keys, seed)
    x = spliced(case).astype(np.float64)
    wd = w.astype(np.float64)
    take = cls >= 0
    st = LdaStats.zeros(case.n_classes, case.S)
    np.add.at(st.zero, cls[take], wd[take])
    wx = x * wd[:, None]
    np.add.at(st.first, cls[take], wx[take])
    st.second = wx[take].T @ x[take]
    st.second = np.tril(st.second) + np.tril(st.second, -1).T
    if not want_abs:
        return st
    abs2 = np.abs(wx[take]).T @ np.abs(x[take])
    abs1 = np.zeros_like(st.first)
    np.add.at(abs1, cls[take], np.abs(wx[take]))
    return st, abs2, abs1, int(take.sum())


def bound(n_frames: int, abs_sum: np.ndarray) -> np.ndarray:
    """Two summation orders of T terms, one rounding per term (and per partial sum): (2T + 2)·2⁻⁵³·Σ|terms|."""
    return (2 * n_frames + 2) * U64 * abs_sum


def integer_case(rng, dim: int, ctx: int, lengths, n_classes: int, class_of_frame=None, n_spk: int = 0) -> Case:
    """Integer-valued features in [−8, 8] and weights from {0, ½, 1, 2}: every product and partial sum is exact in double,
    so any summation order gives the same bits.  One transition-id per (class, weight) pair."""
    lengths = np.asarray(lengths, dtype=np.int64)
    fo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    T = int(fo[-1])
    mfcc = rng.integers(-8, 9, size=(T, dim)).astype(np.float32)
    tid2class = np.concatenate([[0], np.repeat(np.arange(n_classes), len(WEIGHT_SET))]).astype(np.int32)
    tid_weight = np.concatenate([[0], np.tile(WEIGHT_SET, n_classes)]).astype(np.float32)
    cls = rng.integers(0, n_classes, size=T) if class_of_frame is None else np.asarray(class_of_frame)
    ali = (1 + cls * len(WEIGHT_SET) + rng.integers(0, len(WEIGHT_SET), size=T)).astype(np.int32)
    return Case(mfcc, fo, None, None, ali, tid2class, tid_weight, n_classes, ctx)


def real_case(rng, dim: int, ctx: int, lengths, n_classes: int, n_spk: int = 2) -> Case:
    """MFCC-like real features (per-column scale and a per-speaker offset) with per-speaker CMVN statistics of those rows."""
    lengths = np.asarray(lengths, dtype=np.int64)
    fo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    T, n_utt = int(fo[-1]), len(lengths)
    utt2spk = (np.arange(n_utt) % n_spk).astype(np.int32)
    scale = np.linspace(12.0, 1.5, dim)
    shift = rng.normal(0, 5.0, size=(n_spk, dim))
    mfcc = np.zeros((T, dim), np.float32)
    for u in range(n_utt):
        a, b = int(fo[u]), int(fo[u + 1])
        mfcc[a:b] = (rng.normal(size=(b - a, dim)) * scale + shift[utt2spk[u]]).astype(np.float32)
    cmvn = np.zeros((n_spk, 2, dim + 1))
    for s in range(n_spk):
        rows = [mfcc[int(fo[u]): int(fo[u + 1])] for u in range(n_utt) if utt2spk[u] == s and fo[u + 1] > fo[u]]
        if rows:
            cmvn[s] = O.cmvn_stats(rows)
        else:
            cmvn[s, 0, dim] = 1.0
    n_tids = 2 * n_classes + 1
    tid2class = np.concatenate([[0], np.repeat(np.arange(n_classes), 2)]).astype(np.int32)
    tid_weight = np.concatenate([[0], rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 1.5], np.float32), size=n_tids - 1)]).astype(np.float32)
    ali = rng.integers(0, n_tids, size=T).astype(np.int32)
    return Case(mfcc, fo, utt2spk, cmvn, ali, tid2class, tid_weight, n_classes, ctx)


# ---- the estimate, brute force ------------------------------------------------------------------------------------------------
def scatter(stats: LdaStats):
    """(N, m, within, between) straight from the definitions: a loop over the classes."""
    N = stats.zero.sum()
    m = stats.first.sum(axis=0) / N
    total = stats.second / N - np.outer(m, m)
    between = -np.outer(m, m)
    for c in range(len(stats.zero)):
        if stats.zero[c] != 0:
            between = between + np.outer(stats.first[c], stats.first[c]) / stats.zero[c] / N
    return N, m, total - between, between


def estimate(stats: LdaStats, remove_offset: bool = False):
    """(full float64 [S, S(+1)], s descending): whitening by the within-class eigendecomposition (not Cholesky), then the
    eigenvectors of the whitened between-class matrix; row signs fixed as the contract says."""
    _N, m, within, between = scatter(stats)
    ev, V = np.linalg.eigh(0.5 * (within + within.T))
    Wh = (V / np.sqrt(ev)).T                       # Wh·within·Whᵀ = I
    s, Q = np.linalg.eigh(Wh @ (0.5 * (between + between.T)) @ Wh.T)
    order = np.argsort(-s, kind="stable")
    s, Q = s[order], Q[:, order]
    full = Q.T @ Wh
    big = np.abs(full).argmax(axis=1)
    full = full * np.where(full[np.arange(len(full)), big] < 0, -1.0, 1.0)[:, None]
    if remove_offset:
        full = np.concatenate([full, -(full @ m)[:, None]], axis=1)
    return full, s


def identity_residuals(full: np.ndarray, within: np.ndarray, between: np.ndarray):
    """(max |full·within·fullᵀ − I|, max |off-diagonal of full·between·fullᵀ| / largest diagonal entry, the diagonal)."""
    S = within.shape[0]
    F = np.asarray(full, dtype=np.float64)[:, :S]
    a = F @ within @ F.T
    b = F @ between @ F.T
    d = np.diag(b).copy()
    off = b - np.diag(d)
    return float(np.abs(a - np.eye(len(F))).max()), float(np.abs(off).max() / np.abs(d).max()), d
