"""GMM statistics from two feature matrices (mfa_gmm_acc_twofeats_batch in csrc/gmm_acc.hip, its host twin in
csrc/gmm_acc_host.cpp): tests/gmm_acc_ref.py's float64 restatement and bound, restated for two matrices, and the cases
tests/test_gmm_acc_twofeats_cpu.py (host twin) and tests/test_gpu_gmm_acc_twofeats.py (device) share.

The bound is the one derived in tests/gmm_acc_ref.py, term for term.  Everything up to the posterior — the log-likelihood
chain, the softmax and its float32 steps, so δ(t, g) and the absolute w·2⁻¹²⁵ — and the totals see the rows of ``feats_post``
only.  The posterior's error |Δγ_tg| ≤ γ_tg·δ(t, g) + w·2⁻¹²⁵ enters occ as it is, and mean / var weighted by |y_k| and y_k²,
y the row of ``feats_sum``: the terms of those sums are γ·y and γ·y², so S = Σ γ|term| is taken over ``feats_sum`` too, and
the double summation adds its 2·T_p·2⁻⁵³·S.  Nothing here is measured on the code under test."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import gmm_acc_ref as R
from tests.gmm_acc_ref import EPS32, U32, U64, frame_tables, tid_counts   # noqa: F401  (shared with the one-feature tests)


def gmm_acc2(feats_post, feats_sum, pdf, weight, am):
    """``gmm_acc_ref.gmm_acc`` for two matrices: the same dict, posteriors / tot / B_tot / S_tot from ``feats_post``, mean /
    var / S_mean and their bounds with the terms of ``feats_sum``."""
    x_all, y_all = np.asarray(feats_post, np.float64), np.asarray(feats_sum, np.float64)
    assert x_all.shape == y_all.shape
    T, D = x_all.shape
    pdf = np.asarray(pdf, np.int64)
    w_all = np.asarray(weight, np.float64)
    gc, mi, iv = (np.asarray(v, np.float64) for v in (am.gconsts, am.means_invvars, am.inv_vars))
    G = gc.shape[0]
    out = dict(occ=np.zeros(G), mean=np.zeros((G, D)), var=np.zeros((G, D)), S_mean=np.zeros((G, D)), B_occ=np.zeros(G),
               B_mean=np.zeros((G, D)), B_var=np.zeros((G, D)), n_frames=np.zeros(G, np.int64),
               post=np.zeros((T, int(np.diff(am.pdf_offsets).max()))))
    tot, b_tot, s_tot = np.zeros(2), 0.0, 0.0
    live = (w_all != 0) & (pdf >= 0)
    for p in np.unique(pdf[live]):
        rows = np.nonzero(live & (pdf == p))[0]
        g0, g1 = int(am.pdf_offsets[p]), int(am.pdf_offsets[p + 1])
        n, Tp = g1 - g0, len(rows)
        x, y, w = x_all[rows], y_all[rows], w_all[rows]
        x2, y2 = x * x, y * y
        ll = gc[None, g0:g1] + x @ mi[g0:g1].T - 0.5 * x2 @ iv[g0:g1].T
        mag = np.abs(gc)[None, g0:g1] + np.abs(x) @ np.abs(mi[g0:g1]).T + 0.5 * x2 @ np.abs(iv[g0:g1]).T
        e = (2 * D + 1) * U32 * mag.max(axis=1)
        mx = ll.max(axis=1)
        d = ll - mx[:, None]
        ex = np.exp(d)
        s = ex.sum(axis=1)
        sm = ex / s[:, None]
        post = sm * w[:, None]
        dbar = (sm * np.abs(d)).sum(axis=1)
        delta = np.expm1(2 * e)[:, None] + U32 * (np.abs(d) + dbar[:, None] + n + 12)
        dpost = post * delta + w[:, None] * 2.0 ** -125
        out["post"][rows, :n] = post
        out["n_frames"][g0:g1] = Tp
        out["occ"][g0:g1] = post.sum(axis=0)
        out["mean"][g0:g1] = post.T @ y
        out["var"][g0:g1] = post.T @ y2
        out["S_mean"][g0:g1] = post.T @ np.abs(y)
        out["B_occ"][g0:g1] = dpost.sum(axis=0) + 2 * Tp * U64 * out["occ"][g0:g1]
        out["B_mean"][g0:g1] = dpost.T @ np.abs(y) + 2 * Tp * U64 * out["S_mean"][g0:g1]
        out["B_var"][g0:g1] = dpost.T @ y2 + 2 * Tp * U64 * out["var"][g0:g1]
        LL = mx + np.log(s)
        tot += [(w * LL).sum(), w.sum()]
        b_tot += float((w * (e + U32 * (2 * np.abs(LL) + dbar + n + 17))).sum())
        s_tot += float((w * np.abs(LL)).sum())
    out["tot"] = tot
    out["S_tot"] = s_tot
    out["B_tot"] = b_tot + 2 * int(live.sum()) * U64 * s_tot
    return out


@dataclass
class AccCase2:
    name: str
    am: object
    tm: object
    feats: np.ndarray       # [T, dim] float32: the posteriors' rows (gmm_acc_ref.skewed_case's)
    feats_sum: np.ndarray   # [T, dim] float32: the sums' rows
    ali: np.ndarray
    weights: np.ndarray


@lru_cache(maxsize=None)
def skewed_case2(dim) -> AccCase2:
    """``gmm_acc_ref.skewed_case(dim)`` with ``feats_sum`` = a_t·feats + b_tk: every frame its own scale a_t in [0.5, 1.5] and
    every element its own offset in ±1 (at least ¼ in magnitude, so the two matrices differ in every element)."""
    c = R.skewed_case(dim)
    rng = np.random.default_rng(8300 + dim)
    T = c.feats.shape[0]
    a = rng.uniform(0.5, 1.5, size=(T, 1))
    b = rng.uniform(0.25, 1.0, size=(T, dim)) * rng.choice([-1.0, 1.0], size=(T, dim))
    feats_sum = (a * c.feats.astype(np.float64) + b).astype(np.float32)
    return AccCase2(f"two features, {c.name}", c.am, c.tm, c.feats, feats_sum, c.ali, c.weights)
