"""Numpy restatement of the pitch tracker (include/mfa_hip.h, "Pitch and voicing"): Kaldi's ComputeKaldiPitch
(offline, whole utterance) followed by ProcessPitch, written from the algorithm's description — Kaldi's source is not among
this project's references, so nothing here is pinned against Kaldi's arithmetic.  tests/test_pitch_cpu.py pins this file by
what a pitch tracker has to do (tones, noise, a chirp); tests/test_gpu_pitch.py checks the kernels against it.

Two modes.  float64 (``chain=False``): every table and every sum in double.  ``chain=True``: the tables rounded once to
float32 and the device's float32 operation order for the stages whose arithmetic the interface fixes — down-sampling, NCCF,
up-sampling, the Viterbi recursion, the raw output — so that the result is bit-identical to the kernels'.

Decisions where the description leaves room (device and restatement agree on all of them):
  * frames: with n resampled samples, window N and shift: 0 when n < N; with snip_edges (n - N) // shift + 1, without
    int(n / shift + 0.5).  The window of frame t starts at t * shift with snip_edges, else at t * shift + shift // 2 - N // 2;
    samples outside the utterance are zero (before the mean is subtracted).
  * the mean square feeding the ballast is sum(x^2) / n over the resampled signal (no mean removed), summed in double as
    256 interleaved partial sums (sample k to partial k mod 256) added in ascending order.
  * ties in the Viterbi recursion take the smallest predecessor; the final state is the smallest argmin.
  * frame 0 is treated like every other frame with fwd_{-1} = 0.
  * the normalisation window of ProcessPitch is +-normalization_context frames clipped to the utterance, its sums in
    ascending frame order.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace  # noqa: F401

import numpy as np

f32, f64 = np.float32, np.float64


@dataclass(frozen=True)
class Opts:
    sample_frequency: float = 16000.0
    frame_length: float = 25.0
    frame_shift: float = 10.0
    min_f0: float = 50.0
    max_f0: float = 800.0
    soft_min_f0: float = 10.0
    penalty_factor: float = 0.1
    lowpass_cutoff: float = 1000.0
    resample_frequency: float = 4000.0
    delta_pitch: float = 0.005
    nccf_ballast: float = 7000.0
    lowpass_filter_width: int = 1
    upsample_filter_width: int = 5
    snip_edges: bool = True
    pov_scale: float = 2.0
    pov_offset: float = 0.0
    pitch_scale: float = 2.0
    normalization_context: int = 75
    add_pov_feature: bool = True
    add_normalized_log_pitch: bool = True
    add_raw_log_pitch: bool = False


def fmaf32(a, b, c):
    """Correctly rounded float32 fma of float32 arrays: the product is exact in double, the sum is rounded to odd there
    (its exact error comes from TwoSum), and a value rounded to odd at 53 bits rounds to 24 bits as the exact one does."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    nudge = (e != 0.0) & ((bits & 1) == 0)
    grow = (e > 0.0) == (s > 0.0)          # the exact sum lies further from zero than s
    bits = np.where(nudge, np.where(grow, bits + 1, bits - 1), bits)
    return bits.view(f64).astype(f32)


def _filter(d, fc, zeros):
    """Hann-windowed sinc of cutoff fc with ``zeros`` zero crossings a side, at offsets d (seconds)."""
    ww = zeros / (2.0 * fc)
    win = np.where(np.abs(d) < ww, 0.5 * (1.0 + np.cos(2.0 * math.pi * fc / zeros * d)), 0.0)
    safe = np.where(d != 0.0, d, 1.0)
    return np.where(d != 0.0, np.sin(2.0 * math.pi * fc * d) / (math.pi * safe), 2.0 * fc) * win


class LinearPlan:
    """Kaldi's LinearResample(fin, fout, cutoff, zeros): phases O, in_per_unit I, first[i], taps[i], w[i] (float64)."""

    def __init__(self, fin: int, fout: int, fc: float, zeros: int):
        g = math.gcd(fin, fout)
        self.fin, self.fout, self.phases, self.in_per_unit = fin, fout, fout // g, fin // g
        ww = float(zeros) / (2.0 * fc)
        self.first, self.taps, self.w = [], [], []
        for i in range(self.phases):
            t = float(i) / float(fout)
            lo, hi = math.ceil((t - ww) * float(fin)), math.floor((t + ww) * float(fin))
            d = (lo + np.arange(hi - lo + 1, dtype=f64)) / float(fin) - t
            self.first.append(lo); self.taps.append(hi - lo + 1); self.w.append(_filter(d, fc, float(zeros)) / float(fin))
        self.max_taps = max(self.taps)

    def num_out(self, n: int) -> int:
        if n <= 0:
            return 0
        length = n * self.phases
        last = length // self.in_per_unit
        if last * self.in_per_unit == length:
            last -= 1
        return last + 1


class Tables:
    def __init__(self, o: Opts):
        self.o = o
        # the interface carries every option as a float32 (mfa_pitch_opts): 0.005 and 0.1 are their float32 neighbours
        o = replace(o, **{k: float(f32(getattr(o, k))) for k in ("min_f0", "max_f0", "soft_min_f0", "penalty_factor", "delta_pitch",
                                                                   "lowpass_cutoff", "frame_length", "frame_shift")})
        fs = float(o.resample_frequency)
        self.N, self.shift = int(fs * o.frame_length / 1000.0), int(fs * o.frame_shift / 1000.0)
        min_lag, max_lag = 1.0 / o.max_f0, 1.0 / o.min_f0
        w = o.upsample_filter_width / (2.0 * fs)
        self.first, self.last = math.ceil(fs * (min_lag - w)), math.floor(fs * (max_lag + w))
        self.L = self.last - self.first + 1
        lags, lag = [], min_lag
        while lag <= max_lag:
            lags.append(lag)
            lag *= 1.0 + o.delta_pitch
        self.lags = np.array(lags, dtype=f64)
        self.S = len(lags)
        self.sml = o.soft_min_f0 * self.lags
        self.c = o.delta_pitch * o.delta_pitch * o.penalty_factor
        # ArbitraryResample(L inputs at fs, cutoff fs / 2, sample points lag_i - first / fs, upsample_filter_width zeros)
        fc, zeros = 0.5 * fs, float(o.upsample_filter_width)
        fw = zeros / (2.0 * fc)
        t = self.lags - self.first / fs
        lo = np.maximum(np.ceil(fs * (t - fw)).astype(np.int64), 0)
        hi = np.minimum(np.floor(fs * (t + fw)).astype(np.int64), self.L - 1)
        self.up_first, self.up_taps = lo, hi - lo + 1
        self.up_max_taps = int(self.up_taps.max())
        self.up_w = np.zeros((self.S, self.up_max_taps), dtype=f64)
        for i in range(self.S):
            d = t[i] - (lo[i] + np.arange(self.up_taps[i], dtype=f64)) / fs
            self.up_w[i, : self.up_taps[i]] = _filter(d, fc, zeros) / fs
        self.rs = LinearPlan(int(o.sample_frequency), int(o.resample_frequency), float(o.lowpass_cutoff), int(o.lowpass_filter_width))
        # what the device holds
        self.lags32, self.sml32, self.up_w32 = self.lags.astype(f32), self.sml.astype(f32), self.up_w.astype(f32)
        d = np.arange(self.S, dtype=np.int64)
        self.pen32 = f32(self.c) * (d * d).astype(f32)          # one float32 product per entry
        self.pen64 = self.c * (d * d).astype(f64)


_TABLES = {}


def tables(o: Opts) -> Tables:
    if o not in _TABLES:
        _TABLES[o] = Tables(o)
    return _TABLES[o]


def num_frames(n_samples: int, o: Opts) -> int:
    tb = tables(o)
    n = tb.rs.num_out(n_samples)
    if n < tb.N:
        return 0
    return (n - tb.N) // tb.shift + 1 if o.snip_edges else int(n / tb.shift + 0.5)


def resample(x, o: Opts, chain: bool):
    """The down-sampled signal: float64, or (chain) the float32 fmaf chain over ascending taps, taps outside skipped."""
    p = tables(o).rs
    x = np.asarray(x)
    n, count = x.shape[0], p.num_out(x.shape[0])
    y = np.zeros(count, dtype=f32 if chain else f64)
    if count == 0:
        return y
    pad = p.max_taps + p.in_per_unit + 8
    xp = np.concatenate([np.zeros(pad), x.astype(f64), np.zeros(pad)])
    for i in range(min(p.phases, count)):
        u = np.arange((count - i + p.phases - 1) // p.phases, dtype=np.int64)
        start = p.first[i] + u * p.in_per_unit + pad
        win = xp[start[:, None] + np.arange(p.taps[i])[None, :]]
        if chain:
            w, acc = p.w[i].astype(f32), np.zeros(u.shape[0], dtype=f32)
            for j in range(p.taps[i]):                     # (a zero outside the utterance leaves acc as a skipped tap does)
                acc = fmaf32(w[j], win[:, j].astype(f32), acc)
            y[i::p.phases] = acc
        else:
            y[i::p.phases] = win @ p.w[i]
    return y


def ballast(xr, o: Opts, chain: bool):
    tb = tables(o)
    x2 = np.asarray(xr, dtype=f64) ** 2
    if chain:
        x2 = np.concatenate([x2, np.zeros(-x2.shape[0] % 256)]).reshape(-1, 256)
        part = np.zeros(256)
        for row in x2:
            part = part + row
        total = 0.0
        for v in part:
            total = total + float(v)
    else:
        total = math.fsum(x2)
    b = total / float(len(xr)) * float(tb.N)
    b = b * b * float(f32(o.nccf_ballast))
    return f32(b) if chain else b


def windows(xr, T: int, o: Opts):
    """[T][N + last] windows of the resampled signal, zeros outside, before the mean is subtracted."""
    tb = tables(o)
    start = np.arange(T, dtype=np.int64) * tb.shift + (0 if o.snip_edges else tb.shift // 2 - tb.N // 2)
    idx = start[:, None] + np.arange(tb.N + tb.last)[None, :]
    xp = np.concatenate([np.asarray(xr), np.zeros(1, dtype=xr.dtype)])         # index len(xr): the zero outside
    return xp[np.where((idx >= 0) & (idx < len(xr)), idx, len(xr))]


def nccf(xr, T: int, o: Opts, chain: bool):
    """(pitch NCCF, POV NCCF) at the measured lags, [T][L] each."""
    tb = tables(o)
    N, L = tb.N, tb.L
    dt = f32 if chain else f64
    if T == 0:
        return np.zeros((0, L), dt), np.zeros((0, L), dt)
    w = windows(np.asarray(xr, dtype=dt), T, o)
    bal = ballast(xr, o, chain)
    lag_idx = tb.first + np.arange(L)
    if chain:
        s = np.zeros(T, dtype=f32)
        for k in range(N):
            s = s + w[:, k]
        w = w - (s / f32(N))[:, None]
        e0 = np.zeros(T, dtype=f32)
        inner, en = np.zeros((T, L), dtype=f32), np.zeros((T, L), dtype=f32)
        for k in range(N):
            e0 = fmaf32(w[:, k], w[:, k], e0)
            b = w[:, k + lag_idx]
            inner = fmaf32(w[:, k][:, None], b, inner)
            en = fmaf32(b, b, en)
        norm = e0[:, None] * en
    else:
        w = w - w[:, :N].mean(axis=1)[:, None]
        e0 = (w[:, :N] ** 2).sum(axis=1)
        inner, en = np.zeros((T, L)), np.zeros((T, L))
        for q, l in enumerate(lag_idx):
            inner[:, q] = (w[:, :N] * w[:, l: l + N]).sum(axis=1)
            en[:, q] = (w[:, l: l + N] ** 2).sum(axis=1)
        norm = e0[:, None] * en
    with np.errstate(divide="ignore", invalid="ignore"):
        dp, dv = np.sqrt(norm + dt(bal)), np.sqrt(norm)
        n_p = np.where(dp != 0, inner / np.where(dp != 0, dp, 1), 0).astype(dt)
        n_v = np.where(dv != 0, inner / np.where(dv != 0, dv, 1), 0).astype(dt)
    return n_p, n_v


def upsample(meas, o: Opts, chain: bool):
    """[T][L] at the measured lags -> [T][S] at the state lags."""
    tb = tables(o)
    T = meas.shape[0]
    cols = np.minimum(tb.up_first[:, None] + np.arange(tb.up_max_taps)[None, :], tb.L - 1)    # padded taps carry zero weights
    if chain:
        acc = np.zeros((T, tb.S), dtype=f32)
        for j in range(tb.up_max_taps):
            live = tb.up_taps > j                                                              # the device stops at the row's taps
            acc[:, live] = fmaf32(tb.up_w32[live, j][None, :], meas[:, cols[live, j]], acc[:, live])
        return acc
    return np.einsum("sj,tsj->ts", tb.up_w, np.asarray(meas, f64)[:, cols])


def viterbi(nccf_up, o: Opts, chain: bool, want_margin: bool = False):
    """State per frame [T] (and, asked for, the float64 margin between the best and the second-best predecessor of the
    chosen state per frame — frame 0 has no predecessor worth the name: its margin is inf)."""
    tb = tables(o)
    T, S = nccf_up.shape
    dt = f32 if chain else f64
    n = np.asarray(nccf_up, dtype=dt)
    if chain:
        local = fmaf32(tb.sml32[None, :], n, f32(1.0) - n)
        pen = tb.pen32
    else:
        local = 1.0 - n + tb.sml[None, :] * n
        pen = tb.pen64
    d = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :])
    P = pen[d]                                                   # [i][j]
    prev = np.zeros(S, dtype=dt)
    bp = np.zeros((T, S), dtype=np.int64)
    second = np.zeros((T, S))
    for t in range(T):
        cand = prev[None, :] + P                                 # float32 adds in chain mode
        arg = cand.argmin(axis=1)                                # first minimum: smallest j
        best = cand[np.arange(S), arg]
        if want_margin:
            c2 = cand.astype(f64).copy()
            c2[np.arange(S), arg] = np.inf
            second[t] = c2.min(axis=1) - best
        cur = best + local[t]
        prev = cur - cur.min()
        bp[t] = arg
    path = np.zeros(T, dtype=np.int64)
    if T:
        path[T - 1] = int(prev.argmin())
        for t in range(T - 1, 0, -1):
            path[t - 1] = bp[t, path[t]]
    if want_margin:
        m = second[np.arange(T), path] if T else np.zeros(0)
        if T:
            m[0] = np.inf
        return path, m
    return path


def raw_output(pov_up, path, o: Opts, chain: bool):
    """[T][2] = (POV NCCF at the state, 1 / lag_state)."""
    tb = tables(o)
    T = len(path)
    out = np.zeros((T, 2), dtype=f32 if chain else f64)
    out[:, 0] = pov_up[np.arange(T), path]
    out[:, 1] = (f32(1.0) / tb.lags32[path]) if chain else 1.0 / tb.lags[path]
    return out


def pov_weight(nccf, dt=f64):
    a = np.minimum(np.abs(nccf.astype(dt)), dt(1.0))
    r = dt(-5.2) + dt(5.4) * np.exp(dt(7.5) * (a - dt(1.0))) + dt(4.8) * a - dt(2.0) * np.exp(dt(-10.0) * a) \
        + dt(4.2) * np.exp(dt(20.0) * (a - dt(1.0)))
    return dt(1.0) / (dt(1.0) + np.exp(-r))


def process(raw, o: Opts, dt=f64):
    """ProcessPitch on the raw output [T][2] -> [T][columns]: POV feature, normalised log-pitch, raw log-pitch, each if its
    add_* flag is set.  ``dt``: the precision every operation is carried out in (float64: the restatement; float32: what a
    single-precision evaluation of the same formulas gives — the yardstick of the device's tolerance)."""
    raw = np.asarray(raw)
    T = raw.shape[0]
    n, logf = raw[:, 0].astype(dt), np.log(raw[:, 1].astype(dt))
    cols = []
    if o.add_pov_feature:
        c = np.clip(n, dt(-1.0), dt(1.0))
        cols.append(dt(o.pov_scale) * (np.power(dt(1.0001) - c, dt(0.15)) - dt(1.0)) + dt(o.pov_offset))
    if o.add_normalized_log_pitch:
        p = pov_weight(n, dt)
        mean = np.zeros(T, dtype=dt)
        for t in range(T):
            lo, hi = max(0, t - o.normalization_context), min(T - 1, t + o.normalization_context)
            num, den = dt(0.0), dt(0.0)
            for s in range(lo, hi + 1):
                num = num + p[s] * logf[s]
                den = den + p[s]
            mean[t] = num / den
        cols.append(dt(o.pitch_scale) * (logf - mean))
    if o.add_raw_log_pitch:
        cols.append(logf)
    return np.stack(cols, axis=1).astype(dt) if T else np.zeros((0, len(cols)), dtype=dt)


def compute(x, o: Opts, chain: bool = False, T: int | None = None):
    """Everything for one utterance x (int16 or float samples at sample_frequency): dict with resampled, nccf_pitch /
    nccf_pov [T][S] (up-sampled), path [T], raw [T][2]."""
    x = np.asarray(x)
    T = num_frames(len(x), o) if T is None else T
    xr = resample(x, o, chain)
    mp, mv = nccf(xr, T, o, chain)
    up_p, up_v = upsample(mp, o, chain), upsample(mv, o, chain)
    path = viterbi(up_p, o, chain)
    return {"resampled": xr, "nccf_pitch": up_p, "nccf_pov": up_v, "path": path, "raw": raw_output(up_v, path, o, chain)}
