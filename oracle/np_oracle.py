"""Second, independent restatement of the path in numpy/float64 (TEST INFRASTRUCTURE ONLY).

Used to cross-check oracle/mfa_oracle.cpp — the reference holds no golden vectors at the kalpy boundary
(SURVEY.md §8c), so two independently written implementations agreeing is the available evidence.
Written from the formulas in SURVEY.md Appendix A, vectorised, float64 throughout (so it approximates the
float32 oracle from the "exact arithmetic" side).  PARITY STATUS: parity unpinned.
"""
from __future__ import annotations

import numpy as np


def mfcc(wave, samp_freq=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph=0.97, low_freq=20.0,
         high_freq=7800.0, num_mel_bins=23, num_ceps=13, cepstral_lifter=22.0, snip_edges=False, remove_dc_offset=True,
         use_energy=False, raw_energy=True, energy_floor=0.0):
    """SURVEY Appendix A.1 (Kaldi compute-mfcc-feats with MFA's options, dither 0; use_energy: C0 is the frame's log
    energy, before pre-emphasis and window with raw_energy, after them without)."""
    wave = np.asarray(wave, dtype=np.float64)
    n = wave.shape[0]
    win = int(samp_freq * 0.001 * frame_length_ms)
    shift = int(samp_freq * 0.001 * frame_shift_ms)
    nfft = 1
    while nfft < win:
        nfft *= 2
    if snip_edges:
        T = 0 if n < win else 1 + (n - win) // shift
        starts = np.arange(T) * shift
    else:
        T = (n + shift // 2) // shift
        starts = np.arange(T) * shift + shift // 2 - win // 2
    idx = starts[:, None] + np.arange(win)[None, :]
    for _ in range(4):  # reflect (repeatedly for pathological short inputs)
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    fr = wave[idx]
    if remove_dc_offset:
        fr = fr - fr.mean(axis=1, keepdims=True)
    eps = np.finfo(np.float32).eps
    log_energy = np.log(np.maximum((fr * fr).sum(axis=1), eps))
    pre = fr.copy()
    pre[:, 1:] = fr[:, 1:] - preemph * fr[:, :-1]
    pre[:, 0] = fr[:, 0] - preemph * fr[:, 0]
    window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / (win - 1))) ** 0.85
    if not raw_energy:
        log_energy = np.log(np.maximum(((pre * window) ** 2).sum(axis=1), eps))
    spec = np.fft.rfft(pre * window, nfft, axis=1)
    power = spec.real ** 2 + spec.imag ** 2  # [T, nfft/2+1]

    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)

    nyq = 0.5 * samp_freq
    hf = high_freq if high_freq > 0 else nyq + high_freq
    ml, mh = mel(low_freq), mel(hf)
    delta = (mh - ml) / (num_mel_bins + 1)
    binf = mel(samp_freq / nfft * np.arange(nfft // 2))
    W = np.zeros((num_mel_bins, nfft // 2))
    for b in range(num_mel_bins):
        left, center, right = ml + b * delta, ml + (b + 1) * delta, ml + (b + 2) * delta
        up = (binf - left) / (center - left)
        down = (right - binf) / (right - center)
        w = np.where(binf <= center, up, down)
        W[b] = np.where((binf > left) & (binf < right), w, 0.0)
    melE = power[:, : nfft // 2] @ W.T
    melE = np.log(np.maximum(melE, eps))
    k = np.arange(num_ceps)[:, None]
    nn = np.arange(num_mel_bins)[None, :]
    dct = np.sqrt(2.0 / num_mel_bins) * np.cos(np.pi / num_mel_bins * (nn + 0.5) * k)
    dct[0, :] = np.sqrt(1.0 / num_mel_bins)
    c = melE @ dct.T
    if cepstral_lifter != 0:
        c = c * (1.0 + 0.5 * cepstral_lifter * np.sin(np.pi * np.arange(num_ceps) / cepstral_lifter))
    if use_energy:
        c[:, 0] = np.maximum(log_energy, np.log(energy_floor)) if energy_floor > 0 else log_energy
    return c


def cmvn(feats):
    return feats - feats.mean(axis=0, keepdims=True)


def deltas(feats):
    """Appendix A.3: Δ = [-2,-1,0,1,2]/10, ΔΔ = Δ∗Δ, edge frames clamped."""
    feats = np.asarray(feats, np.float64)
    T = feats.shape[0]
    d1 = np.array([-2, -1, 0, 1, 2], dtype=np.float64) / 10.0
    d2 = np.convolve(d1, d1)

    def conv(k):
        h = (len(k) - 1) // 2
        out = np.zeros_like(feats)
        for j in range(-h, h + 1):
            out += k[j + h] * feats[np.clip(np.arange(T) + j, 0, T - 1)]
        return out

    return np.concatenate([feats, conv(d1), conv(d2)], axis=1)


def splice(feats, left=3, right=3):
    T = feats.shape[0]
    return np.concatenate([feats[np.clip(np.arange(T) + j, 0, T - 1)] for j in range(-left, right + 1)], axis=1)


def affine(feats, M):
    d = feats.shape[1]
    y = feats @ M[:, :d].T
    if M.shape[1] == d + 1:
        y = y + M[:, d]
    return y


def gmm_loglikes(feats, gconsts, means_invvars, inv_vars, pdf_offsets, pdf_list):
    """Appendix A.6, float64, plain log-sum-exp (no cutoff: it only drops terms < eps relative)."""
    x = np.asarray(feats, np.float64)
    ll = gconsts[None, :].astype(np.float64) + x @ means_invvars.T.astype(np.float64) - 0.5 * (x * x) @ inv_vars.T.astype(np.float64)
    out = np.zeros((x.shape[0], len(pdf_list)))
    for j, p in enumerate(pdf_list):
        a, b = pdf_offsets[p], pdf_offsets[p + 1]
        m = ll[:, a:b].max(axis=1)
        out[:, j] = m + np.log(np.exp(ll[:, a:b] - m[:, None]).sum(axis=1))
    return out


def viterbi_exact(num_states, start, arc_offsets, arcs, final, neg_scaled_loglikes, tid2col):
    """Unpruned Viterbi over an epsilon-free graph: returns (best total cost, alignment).  Cost = Σ arc weight +
    Σ acoustic cost + final weight; used to check that the beam decoder with a wide beam finds the optimum."""
    T = neg_scaled_loglikes.shape[0]
    INF = np.inf
    cost = np.full(num_states, INF)
    cost[start] = 0.0
    src = np.repeat(np.arange(num_states), np.diff(arc_offsets))
    il = arcs["ilabel"]
    if np.any(il == 0):
        raise ValueError("viterbi_exact expects an epsilon-free graph")
    w = arcs["weight"].astype(np.float64)
    dst = arcs["nextstate"]
    cols = tid2col[il]
    back = np.zeros((T, num_states), dtype=np.int64)
    for t in range(T):
        cand = cost[src] + w + neg_scaled_loglikes[t, cols].astype(np.float64)
        new = np.full(num_states, INF)
        order = np.argsort(cand, kind="stable")
        # first occurrence per dst in cost order wins
        d_sorted = dst[order]
        first = np.unique(d_sorted, return_index=True)[1]
        win = order[first]
        new[dst[win]] = cand[win]
        back[t, dst[win]] = win
        cost = new
    tot = cost + np.where(np.isinf(final), INF, final.astype(np.float64))
    s = int(np.argmin(tot))
    best = tot[s]
    ali = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        a = back[t, s]
        ali[t] = il[a]
        s = src[a]
    return best, ali


# ---- fMLLR: statistics and the row-by-row solve, float64 ------------------------------------------------------
def fmllr_acc(feats, ali_pdf, weight, gconsts, means_invvars, inv_vars, pdf_offsets, stat_means_invvars=None,
              stat_inv_vars=None, chunk=4096):
    """fMLLR statistics of one speaker's frames, everything in float64 (log-likelihoods, posteriors, a, b and the sums):
    β = Σ_t Σ_g γ_tg,  K = Σ_t a_t ξ_tᵀ,  G_d = Σ_t b_t[d] ξ_t ξ_tᵀ  with ξ = [x; 1], γ_t = w_t · softmax over the aligned pdf,
    a_t = Σ_g γ_tg mi_g, b_t = Σ_g γ_tg iv_g.  With ``stat_*`` the posteriors come from (gconsts, means_invvars, inv_vars) and
    mi, iv from the stat_* arrays (the two-model form).  Frames of weight 0 or pdf < 0 contribute nothing.

    Returns dict(beta, K, G) and the absolute-sum scales of the same sums, the unit a float32 pipeline's error is measured in:
    S_beta = Σ_t w_t,  SK[d,e] = Σ_t (Σ_g γ_tg |mi_g[d]|) |ξ_t[e]|,  SG[d,e,f] = Σ_t (Σ_g γ_tg iv_g[d]) |ξ_t[e] ξ_t[f]|."""
    x_all = np.asarray(feats, np.float64)
    T, D = x_all.shape
    D1 = D + 1
    ali_pdf = np.asarray(ali_pdf, np.int64)
    w_all = np.asarray(weight, np.float64)
    gc, mi, iv = (np.asarray(v, np.float64) for v in (gconsts, means_invvars, inv_vars))
    smi = mi if stat_means_invvars is None else np.asarray(stat_means_invvars, np.float64)
    siv = iv if stat_inv_vars is None else np.asarray(stat_inv_vars, np.float64)
    a, b, aa = np.zeros((T, D)), np.zeros((T, D)), np.zeros((T, D))
    beta = 0.0
    live = (w_all != 0) & (ali_pdf >= 0)
    for p in np.unique(ali_pdf[live]):
        rows = np.nonzero(live & (ali_pdf == p))[0]
        g0, g1 = int(pdf_offsets[p]), int(pdf_offsets[p + 1])
        x = x_all[rows]
        ll = gc[None, g0:g1] + x @ mi[g0:g1].T - 0.5 * (x * x) @ iv[g0:g1].T
        post = np.exp(ll - ll.max(axis=1, keepdims=True))
        post *= (w_all[rows] / post.sum(axis=1))[:, None]
        beta += float(post.sum())
        a[rows], b[rows], aa[rows] = post @ smi[g0:g1], post @ siv[g0:g1], post @ np.abs(smi[g0:g1])
    xi = np.concatenate([x_all, np.ones((T, 1))], axis=1)
    xi[~live] = 0.0
    K, SK = a.T @ xi, aa.T @ np.abs(xi)
    G, SG = np.zeros((D, D1 * D1)), np.zeros((D, D1 * D1))
    for t0 in range(0, T, chunk):
        xc = xi[t0:t0 + chunk]
        ef = (xc[:, :, None] * xc[:, None, :]).reshape(xc.shape[0], D1 * D1)
        G += b[t0:t0 + chunk].T @ ef
        SG += b[t0:t0 + chunk].T @ np.abs(ef)
    return dict(beta=beta, K=K, G=G.reshape(D, D1, D1), S_beta=float(w_all[live].sum()), SK=SK, SG=SG.reshape(D, D1, D1))


def fmllr_aux(W, beta, K, G):
    """β log|det A| + Σ_d w_d·k_d − ½ Σ_d w_d G_d w_dᵀ  (W = [A b])."""
    D = W.shape[0]
    quad = sum(float(W[d] @ G[d] @ W[d]) for d in range(D))
    return beta * np.linalg.slogdet(W[:, :D])[1] + float(np.sum(W * K)) - 0.5 * quad


def fmllr_solve(beta, K, G, num_iters=40, min_count=500.0, init=None, trace=None):
    """The row update of Kaldi's ComputeFmllrMatrixDiagGmmFull, from its description: for ``num_iters`` sweeps and each row
    d, with c = [row d of (A⁻¹)ᵀ; 0] (the cofactor row up to det A): e1 = cᵀ G_d⁻¹ c, e2 = cᵀ G_d⁻¹ k_d, α = the root of
    e1 α² + e2 α − β = 0 that maximises β log|α e1 + e2| − ½ α² e1, and w_d = G_d⁻¹ (α c + k_d).  Linear systems with
    np.linalg.solve (no explicit inverse of G).  The estimate is dropped for the starting transform when β < min_count or the
    auxiliary function fell by more than rounding.  Returns (W [D, D+1] float64, improvement); ``trace`` (a list) receives the
    auxiliary function before the first and after every sweep."""
    K, G = np.asarray(K, np.float64), np.asarray(G, np.float64)
    D = K.shape[0]
    W0 = np.eye(D, D + 1) if init is None else np.array(init, dtype=np.float64)
    if beta < min_count:
        return W0, 0.0
    W = W0.copy()
    old = fmllr_aux(W0, beta, K, G)
    if trace is not None:
        trace.append(old)
    for _ in range(num_iters):
        for d in range(D):
            e_d = np.zeros(D)
            e_d[d] = 1.0
            c = np.append(np.linalg.solve(W[:, :D], e_d), 0.0)      # A⁻¹ e_d = column d of A⁻¹ = row d of (A⁻¹)ᵀ
            gc_, gk = np.linalg.solve(G[d], np.stack([c, K[d]], axis=1)).T
            e1, e2 = float(c @ gc_), float(c @ gk)
            root = np.sqrt(e2 * e2 + 4.0 * e1 * beta)
            a1, a2 = (-e2 + root) / (2.0 * e1), (-e2 - root) / (2.0 * e1)
            f1, f2 = (beta * np.log(abs(al * e1 + e2)) - 0.5 * al * al * e1 for al in (a1, a2))
            W[d] = (a1 if f1 > f2 else a2) * gc_ + gk
        if trace is not None:
            trace.append(fmllr_aux(W, beta, K, G))
    new = fmllr_aux(W, beta, K, G)
    if new < old and abs(new - old) > 0.001 * (abs(new) + abs(old)):
        return W0, 0.0
    return W, new - old
