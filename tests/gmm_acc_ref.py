"""GMM statistics (csrc/gmm_acc.hip, its host twin csrc/gmm_acc_host.cpp): the float64 restatement of the contract of
include/mfa_hip.h, a derived bound on what a float32 softmax may put between it and an implementation of the contract, and
the cases tests/test_gmm_acc_cpu.py (host twin) and tests/test_gpu_gmm_acc.py (device) share.

The bound.  u = 2⁻²⁴ is float32's unit roundoff.  For a frame t of pdf p with n Gaussians and weight w:

  log-likelihood   the contract's chain is 2·dim fmaf (one rounding each of a partial sum of magnitude at most M) and dim
                   float32 squares (one rounding of a term); with M(t, g) = |gconst_g| + Σ_k |w_gk · x̃_tk| in float64, as in
                   tests/gmm_ref.py, |ll̂_g − ll_g| ≤ (2·dim + 1)·u·M(t, g) =: e(t, g); e_t = max_g e(t, g).
  softmax          γ_g = w·exp(ll_g) / Σ_h exp(ll_h) is moved by a factor within exp(±2 e_t) when every ll moves by at most
                   e_t: a relative expm1(2 e_t).
  float32 steps    d_g = ll_g − m rounds once: u·|d_g| on the exponent, so relative u·|d_g| on e_g; the exponential itself: libm
                   is below 1 ulp, the device's is held to 2.5 ulp (tests/test_gpu_fmllr_stats.py): 5u; the sum s carries
                   its terms' errors weighted by their share, Σ_h softmax_h·(u·|d_h| + 5u) =: u·(D̄_t + 5), and n − 1 additions
                   of positive terms in any order: (n − 1)·u; 1/s, ·inv, ·w: 3u.  Together
                       δ(t, g) = expm1(2 e_t) + u·(|d_g| + D̄_t + n + 12)
                   and an absolute w·2⁻¹²⁵ for an e_g under float32's normal range (flushed or rounded as a denormal).
  sums             |Δγ_tg| ≤ γ_tg·δ(t, g) + w·2⁻¹²⁵ enters occ as it is and mean / var weighted by |x_k|, x_k²; the double
                   sums themselves, T_p addends in two different orders: 2·T_p·2⁻⁵³·S, S the sum of the absolute terms.
  totals           log-sum-exp is 1-Lipschitz in the max norm: e_t; m + logf(s) rounds its result and logf (1 ulp of at most
                   ln 128 < 5) and carries s's relative error: u·(2·|LL| + 10 + D̄_t + 5 + n − 1 + 3) ≤ u·(2·|LL| + D̄_t + n + 17);
                   weighted by w and summed, plus the double summation.  tot[1] = Σ w has no float32 step at all.
Nothing here is measured on the code under test."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import gmm_ref, helpers

U32 = 2.0 ** -24
U64 = 2.0 ** -53
EPS32 = 2.0 ** -23


def frame_tables(tm, ali, weights=None):
    """Per-frame (pdf, weight) of the contract: pdf −1 and weight 0 for a frame that takes no part."""
    id2pdf = np.maximum(tm.id2pdf, 0).astype(np.int32)
    w = np.ones(len(id2pdf), np.float32) if weights is None else np.asarray(weights, np.float32).copy()
    w[0] = 0
    ali = np.asarray(ali, np.int64)
    ok = (ali > 0) & (ali < len(id2pdf))
    safe = np.where(ok, ali, 0)
    fw = np.where(ok, w[safe], 0).astype(np.float32)
    pdf = np.where(ok & (fw != 0), id2pdf[safe], -1).astype(np.int32)
    return pdf, fw


def gmm_acc(feats, pdf, weight, am):
    """The statistics in float64, grouped by pdf, and the bound of the module docstring on each of them.  Returns a dict:
    occ [G], mean / var [G, dim], tot [2]; S_mean = Σ γ|x| (occ and var are their own absolute sums); B_occ, B_mean, B_var,
    B_tot: the bounds; S_tot = Σ w|LL|; n_frames [G]: frames of the Gaussian's pdf; post [T, largest pdf]: the float64 posteriors."""
    x_all = np.asarray(feats, np.float64)
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
        x, w = x_all[rows], w_all[rows]
        x2 = x * x
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
        out["mean"][g0:g1] = post.T @ x
        out["var"][g0:g1] = post.T @ x2
        out["S_mean"][g0:g1] = post.T @ np.abs(x)
        out["B_occ"][g0:g1] = dpost.sum(axis=0) + 2 * Tp * U64 * out["occ"][g0:g1]
        out["B_mean"][g0:g1] = dpost.T @ np.abs(x) + 2 * Tp * U64 * out["S_mean"][g0:g1]
        out["B_var"][g0:g1] = dpost.T @ x2 + 2 * Tp * U64 * out["var"][g0:g1]
        LL = mx + np.log(s)
        tot += [(w * LL).sum(), w.sum()]
        b_tot += float((w * (e + U32 * (2 * np.abs(LL) + dbar + n + 17))).sum())
        s_tot += float((w * np.abs(LL)).sum())
    out["tot"] = tot
    out["S_tot"] = s_tot
    out["B_tot"] = b_tot + 2 * int(live.sum()) * U64 * s_tot
    return out


def tid_counts(ali, pdf, n_tids):
    """tid_count of the contract: one per frame that takes part."""
    ali = np.asarray(ali, np.int64)
    return np.bincount(ali[np.asarray(pdf) >= 0], minlength=n_tids).astype(np.int64)


# ---- the soft cases: tests/gmm_ref.py's skewed model, frames from its own Gaussians ----------------------------------------
@dataclass
class AccCase:
    name: str
    am: object
    tm: object
    feats: np.ndarray     # [T, dim] float32
    ali: np.ndarray       # [T] int32 transition-ids: some 0, some outside the table, some of weight 0
    weights: np.ndarray   # [n_tids] float32


@lru_cache(maxsize=None)
def skewed_case(dim) -> AccCase:
    """gmm_ref.skewed_gmm over SIZES_SKEWED (1 … 128 Gaussians) with sample_frames; transition-ids 2p + 1 / 2p + 2 of pdf p
    (helpers.fmllr_tm).  The 128- and the 17-Gaussian pdf get 700 and 600 frames (more than one chunk of the device kernel,
    both rounds of its posterior phase), the rest is uniform; frames are shuffled.  Weights: 1, 0.5, 0.3 and, for one
    transition-id, 0; 40 frames carry id 0 and 40 an id outside the table."""
    rng = np.random.default_rng(8100 + dim)
    sizes = gmm_ref.SIZES_SKEWED
    sk = gmm_ref.skewed_gmm(rng, dim, sizes)
    P = len(sizes)
    T = 2500
    pdfs = np.concatenate([np.full(700, sizes.index(128)), np.full(600, sizes.index(17)), rng.integers(0, P, size=T - 1300)])
    pdfs = rng.permutation(pdfs)
    tm = helpers.fmllr_tm(P)
    n_tids = 2 * P + 1
    weights = rng.choice(np.array([1.0, 0.5, 0.3], np.float32), size=n_tids).astype(np.float32)
    weights[4] = 0.0                          # the second transition-id of pdf 1: its frames take no part
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=T)).astype(np.int32)
    odd = rng.permutation(T)[:80]
    ali[odd[:40]] = 0
    ali[odd[40:60]] = n_tids + rng.integers(0, 5, size=20)
    ali[odd[60:]] = -1 - rng.integers(0, 5, size=20)
    return AccCase(f"skewed dim {dim}", sk.am, tm, gmm_ref.sample_frames(rng, sk, T), ali, weights)
