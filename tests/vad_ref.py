"""Plain restatement of the speech-activity stage in Python floats (float64), one frame at a time from the definitions of
include/mfa_hip.h ("Speech activity") and of Kaldi's ComputeVadEnergy / SlidingWindowCmn / select-voiced-frames /
subsample-feats.  Nothing here knows csrc/vad_math.hpp: sums are plain left-to-right float64 sums, window counts are
counted frame by frame, windows are summed from scratch for every frame."""
import math

import numpy as np


def vad_threshold(energy, energy_threshold=5.0, energy_mean_scale=0.5):
    e = [float(v) for v in energy]
    if energy_mean_scale == 0.0 or not e:
        return float(np.float32(energy_threshold))
    return float(np.float32(float(np.float32(energy_threshold)) + float(np.float32(energy_mean_scale)) * (math.fsum(e) / len(e))))


def vad(energy, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
    """(0/1 decisions float32 [T], threshold).  The decision is Kaldi's `num >= den * proportion_threshold` in float32."""
    thr = vad_threshold(energy, energy_threshold, energy_mean_scale)
    T = len(energy)
    out = np.zeros(T, dtype=np.float32)
    pt = np.float32(proportion_threshold)
    for t in range(T):
        num = den = 0
        for t2 in range(t - frames_context, t + frames_context + 1):
            if 0 <= t2 < T:
                den += 1
                if float(energy[t2]) > thr:
                    num += 1
        if np.float32(num) >= np.float32(den) * pt:
            out[t] = 1.0
    return out, thr


def cmn_window(t, T, cmn_window=600, min_window=100, center=False):
    if center:
        start = t - cmn_window // 2
        end = start + cmn_window
    else:
        start = t - cmn_window
        end = t + 1
    if start < 0:
        end -= start
        start = 0
    if not center and end > t:
        end = max(t + 1, min_window)
    if end > T:
        start -= end - T
        end = T
        if start < 0:
            start = 0
    return start, end


def sliding_cmvn(x, cmn_window_=600, min_window=100, center=False, norm_vars=False, dim=None):
    """float64 [T, D]: every window summed from scratch with math.fsum (the exactly rounded sum)."""
    x = np.asarray(x, dtype=np.float64)
    T, D = x.shape
    dim = D if dim is None else dim
    out = x.copy()
    for t in range(T):
        s, e = cmn_window(t, T, cmn_window_, min_window, center)
        n = e - s
        for c in range(dim):
            col = x[s:e, c].tolist()
            mean = math.fsum(col) / n
            v = x[t, c] - mean
            if norm_vars and n > 1:
                var = math.fsum(a * a for a in col) / n - mean * mean
                v *= 1.0 / math.sqrt(max(var, 1e-10))
            out[t, c] = v
    return out


def select_frames(x, vad_=None, n=1):
    rows = [t for t in range(len(x)) if vad_ is None or vad_[t] != 0]
    return np.asarray(x)[rows[::n]] if rows else np.asarray(x)[:0]


def select_batch(x, frame_off, vad_=None, n=1):
    outs = [select_frames(x[a:b], None if vad_ is None else vad_[a:b], n) for a, b in zip(frame_off[:-1], frame_off[1:])]
    return (np.concatenate(outs) if outs else np.asarray(x)[:0]), np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64)


def runs(vad_):
    """[(first frame, last frame + 1)] of every maximal run of non-zero entries."""
    out, start = [], None
    for t, v in enumerate(list(vad_) + [0]):
        if v != 0 and start is None:
            start = t
        elif v == 0 and start is not None:
            out.append((start, t))
            start = None
    return out


def scan(values, frame_off):
    """(exclusive scan restarted at every utterance, utterance sums)."""
    out, totals = np.zeros(len(values), dtype=np.int64), []
    for a, b in zip(frame_off[:-1], frame_off[1:]):
        acc = 0
        for f in range(a, b):
            out[f] = acc
            acc += int(values[f])
        totals.append(acc)
    return out, np.asarray(totals, dtype=np.int64)
