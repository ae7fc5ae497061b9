"""The diagonal-UBM stage (csrc/ubm.hip, its host twins csrc/ubm_host.cpp): the float64 restatement of both contracts of
include/mfa_hip.h ("Diagonal UBM"), the bound of tests/gmm_acc_ref.py re-derived for a softmax over a frame's n selected
Gaussians, and the cases tests/test_ubm_cpu.py (host twins) and tests/test_gpu_ubm.py (device) share.

The bound.  u = 2⁻²⁴ is float32's unit roundoff.  For a frame t with weight w whose list holds n valid Gaussians (n = G on
the dense path):

  log-likelihood   as tests/gmm_acc_ref.py: |ll̂_g − ll_g| ≤ (2·dim + 1)·u·M(t, g) =: e(t, g), M(t, g) = |gconst_g| +
                   Σ_k |w_gk·x̃_tk| in float64; e_t = max over ALL Gaussians of the model (the selection compares them all).
  selection        two Gaussians whose float64 log-likelihoods are more than 2·e_t apart cannot change places in float32.  A
                   frame is boundary-ambiguous when the gap between its n-th and (n + 1)-th float64 log-likelihood is ≤ 2·e_t;
                   on every other frame the float32 set is the float64 set, and along any float32 list the float64
                   log-likelihoods are non-increasing up to 2·e_t.
  softmax          over the n listed Gaussians, exactly as gmm_acc_ref derives it over a pdf's:
                       δ(t, g) = expm1(2 e_t) + u·(|d_g| + D̄_t + n + 12),   |Δγ_tg| ≤ γ_tg·δ(t, g) + w·2⁻¹²⁵.
  sums             Δγ enters occ as it is and mean / var weighted by |x_k|, x_k²; the double sums themselves: a Gaussian's
                   addends are at most the T frames of the batch plus, on the device, one partial per slab — two orders of at
                   most T + T/slab + 1 ≤ 2T + 1 addends: 2·(2T + 1)·2⁻⁵³·S, S the sum of the absolute terms.  (A frame that does
                   not list the Gaussian adds an exact zero on the device and nothing on the host.)
  frame loglike    log-sum-exp is 1-Lipschitz in the max norm: e_t; m + logf(s) rounds its result, logf is held to 2 ulp of at
                   most ln 2048 < 8, and s carries u·(D̄_t + 5 + n − 1 + 3): u·(2·|LL| + 16 + D̄_t + n + 7) =
                   u·(2·|LL| + D̄_t + n + 23).  Weighted by w and summed for tot[0], plus the double summation; tot[1] = Σ w
                   has no float32 step at all.
Nothing here is measured on the code under test."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from montreal_forced_aligner_amd.ubm import DiagUbm

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def random_ubm(rng, G, dim) -> DiagUbm:
    """Means N(0, 2²), variances U(0.3, 2), Dirichlet(1) weights."""
    w = rng.dirichlet(np.ones(G)) if G > 1 else np.ones(1)
    w = np.maximum(w, 1e-6)
    return DiagUbm.from_parameters(w / w.sum(), rng.normal(0.0, 2.0, (G, dim)), rng.uniform(0.3, 2.0, (G, dim)))


def sample_frames(rng, ubm: DiagUbm, T, spread=1.3) -> np.ndarray:
    """T frames drawn from the mixture with ``spread`` times its standard deviations, float32."""
    g = rng.choice(ubm.num_gauss, size=T, p=ubm.weights.astype(np.float64) / ubm.weights.astype(np.float64).sum())
    return (ubm.means[g] + spread * np.sqrt(ubm.variances[g]) * rng.standard_normal((T, ubm.dim))).astype(np.float32)


@lru_cache(maxsize=None)
def case(G, dim, T, seed=0):
    """(model, frames) shared by the tests; treat both as read-only."""
    rng = np.random.default_rng(9000 + 7 * G + dim + seed)
    ubm = random_ubm(rng, G, dim)
    return ubm, sample_frames(rng, ubm, T)


def loglikes(feats, ubm: DiagUbm):
    """float64 ll [T, G] of the float32 model and frames, and e_t [T]."""
    x = np.asarray(feats, np.float64)
    gc, mi, iv = (np.asarray(a, np.float64) for a in (ubm.gconsts, ubm.means_invvars, ubm.inv_vars))
    x2 = x * x
    ll = gc[None] + x @ mi.T - 0.5 * x2 @ iv.T
    mag = np.abs(gc)[None] + np.abs(x) @ np.abs(mi).T + 0.5 * x2 @ np.abs(iv).T
    return ll, (2 * x.shape[1] + 1) * U32 * mag.max(axis=1)


def select(ll, n):
    """The contract's order in float64: (ll, index) pairs descending, the first n.  int32 [T, min(n, G)]."""
    T, G = ll.shape
    idx = np.broadcast_to(np.arange(G), (T, G))
    order = np.lexsort((-idx, -ll), axis=1)      # by ll descending, at equal ll by index descending
    return order[:, :min(n, G)].astype(np.int32)


def ambiguous(ll, e, n):
    """Frames whose n-th and (n + 1)-th float64 log-likelihoods are within 2·e_t (none when n >= G)."""
    if n >= ll.shape[1]:
        return np.zeros(ll.shape[0], dtype=bool)
    s = -np.sort(-ll, axis=1)
    return s[:, n - 1] - s[:, n] <= 2 * e


def frame_loglike(ll, e, gselect):
    """float64 log-sum-exp over each frame's list and the bound on a float32 evaluation of it."""
    sel = np.take_along_axis(ll, gselect.astype(np.int64), axis=1)
    mx = sel.max(axis=1)
    d = sel - mx[:, None]
    ex = np.exp(d)
    s = ex.sum(axis=1)
    LL = mx + np.log(s)
    dbar = (ex / s[:, None] * np.abs(d)).sum(axis=1)
    return LL, e + U32 * (2 * np.abs(LL) + dbar + gselect.shape[1] + 23)


def ubm_acc(feats, ubm: DiagUbm, gselect=None, weight=None):
    """The statistics in float64 and the module docstring's bound on each of them.  Returns a dict: occ [G], mean / var
    [G, dim], tot [2], post [T, n] (the list's order; dense: [T, G]), the bounds B_occ, B_mean, B_var, B_tot, B_post."""
    x = np.asarray(feats, np.float64)
    T, D = x.shape
    G = ubm.num_gauss
    ll, e = loglikes(feats, ubm)
    w = np.ones(T) if weight is None else np.asarray(weight, np.float64)
    sel = np.broadcast_to(np.arange(G), (T, G)) if gselect is None else np.asarray(gselect, np.int64)
    n = sel.shape[1]
    valid = (sel >= 0) & (sel < G)
    safe = np.where(valid, sel, 0)
    lls = np.where(valid, np.take_along_axis(ll, safe, axis=1), -np.inf)
    live = valid.any(axis=1) & (w != 0)
    mx = np.where(live, lls.max(axis=1), 0.0)
    d = np.where(valid, lls - mx[:, None], -np.inf)
    ex = np.where(live[:, None], np.exp(d), 0.0)
    s = np.where(live, ex.sum(axis=1), 1.0)
    sm = ex / s[:, None]
    post = sm * (w * live)[:, None]
    absd = np.where(valid & live[:, None], np.abs(d), 0.0)
    dbar = (sm * absd).sum(axis=1)
    nv = valid.sum(axis=1)
    delta = np.expm1(2 * e)[:, None] + U32 * (absd + dbar[:, None] + nv[:, None] + 12)
    dpost = np.where(valid & live[:, None], post * delta + np.abs(w)[:, None] * 2.0 ** -125, 0.0)
    x2 = x * x
    out = dict(post=post, B_post=dpost, occ=np.zeros(G), mean=np.zeros((G, D)), var=np.zeros((G, D)), B_occ=np.zeros(G),
               B_mean=np.zeros((G, D)), B_var=np.zeros((G, D)))
    S_mean = np.zeros((G, D))
    if gselect is None:                     # every list is 0 … G − 1: plain products
        ax = np.abs(x)
        out.update(occ=post.sum(axis=0), mean=post.T @ x, var=post.T @ x2, B_occ=dpost.sum(axis=0), B_mean=dpost.T @ ax,
                   B_var=dpost.T @ x2)
        S_mean = np.abs(post).T @ ax
    for j in range(0 if gselect is None else n):          # scatter column by column: a list's indices are distinct
        g, p, dp = safe[:, j], post[:, j], dpost[:, j]
        np.add.at(out["occ"], g, p)
        np.add.at(out["mean"], g, p[:, None] * x)
        np.add.at(out["var"], g, p[:, None] * x2)
        np.add.at(S_mean, g, np.abs(p)[:, None] * np.abs(x))
        np.add.at(out["B_occ"], g, dp)
        np.add.at(out["B_mean"], g, dp[:, None] * np.abs(x))
        np.add.at(out["B_var"], g, dp[:, None] * x2)
    order = 2 * (2 * T + 1) * U64
    out["B_occ"] += order * np.abs(out["occ"])
    out["B_mean"] += order * S_mean
    out["B_var"] += order * np.abs(out["var"])
    LL = np.where(live, mx + np.log(s), 0.0)
    wl = w * live
    out["tot"] = np.array([(wl * LL).sum(), wl.sum()])
    out["B_tot"] = float((np.abs(wl) * (e + U32 * (2 * np.abs(LL) + dbar + nv + 23))).sum()) + order * float((np.abs(wl) * np.abs(LL)).sum())
    out["live"] = live
    return out


def check_stats(st, ref, what):
    """``st`` (a GmmStats of the twin or the device) against ``ubm_acc``'s result under its bound; prints the worst ratios."""
    worst = {}
    for name, got, want, bound in (("occ", st.occ, ref["occ"], ref["B_occ"]), ("mean", st.mean_acc, ref["mean"], ref["B_mean"]),
                                   ("var", st.var_acc, ref["var"], ref["B_var"])):
        assert np.isfinite(got).all(), (what, name)
        err = np.abs(got - want)
        worst[name] = float(np.max(err / np.where(bound > 0, bound, 1.0)))
    worst["tot"] = abs(st.tot_like - ref["tot"][0]) / ref["B_tot"] if ref["B_tot"] > 0 else abs(st.tot_like - ref["tot"][0])
    print(f"{what}: |got - float64| / bound: " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    for name, got, want, bound in (("occ", st.occ, ref["occ"], ref["B_occ"]), ("mean", st.mean_acc, ref["mean"], ref["B_mean"]),
                                   ("var", st.var_acc, ref["var"], ref["B_var"])):
        assert (np.abs(got - want) <= bound).all(), (what, name, worst[name])
    assert abs(st.tot_like - ref["tot"][0]) <= ref["B_tot"], (what, worst)
    assert st.tot_count == ref["tot"][1], what            # Σ w of the cases' weights (1, ½, 0, ¼) is exact


def bits(st):
    return b"".join(np.asarray(a, dtype=np.float64).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count]))


# ---- the trainer's two corpora ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def mixture8():
    """20 000 frames of dim 13 from a known, well separated 8-Gaussian mixture, as (key, matrix) utterances of 500 frames."""
    rng = np.random.default_rng(808)
    ubm = DiagUbm.from_parameters(np.full(8, 0.125), rng.normal(0.0, 4.0, (8, 13)), rng.uniform(0.5, 1.5, (8, 13)))
    x = sample_frames(rng, ubm, 20000, spread=1.0)
    return ubm, [(f"utt{i:02d}", x[500 * i: 500 * (i + 1)]) for i in range(40)]


@lru_cache(maxsize=None)
def wav_features():
    """The reference fixture's recording as the UBM stage reads it, made on the host: MFCC with energy → the energy VAD on
    them → sliding-window CMVN (window 300, centred) → the voiced frames → every fifth.  One utterance per 4 s of audio."""
    from montreal_forced_aligner_amd import frontend as F
    from oracle import oracle as O
    from tests import helpers

    pcm = helpers.Fixtures().pcm
    out = []
    for i in range(0, len(pcm) - 16000, 64000):
        mf = O.mfcc(pcm[i: i + 64000].astype(np.float32), O.default_mfcc_opts(use_energy=1, raw_energy=0))
        fo = np.array([0, mf.shape[0]], dtype=np.int64)
        vad = F.vad_host(mf, fo)[0]
        x = F.sliding_cmvn_host(mf, fo, cmn_window=300, center=1, norm_vars=0)
        x, _ = F.select_frames_host(x, fo, vad, 5)
        if x.shape[0]:
            out.append((f"wav-{i // 64000}", np.ascontiguousarray(x, dtype=np.float32)))
    return out
