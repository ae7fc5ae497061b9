"""Tree statistics time per call on resident inputs, at the benchmark's batch shape: 8 192 utterances × 10 s (about 1 000
frames each), dim 40, 70 three-state phones and two silence phones with long states that are context-independent.  Alignments
are phone sequences (every phone has 24 possible successors: some 10⁵ windows; 1 024 distinct utterances, repeated) in the order of the project's graphs (a state's forward arc, then its self-loops), states of 1 – 6
frames, silence on some 15 % of the frames: a handful of events with a large share of all frames, tens of thousands of a
few tens of frames.  Reported: the median over ``--rounds`` calls of mfa_tree_acc_batch per stage, by the library's event
pairs (mfa_kernel_timing, slots 21 – 23: keys, ordering, sums); the download of the event rows' bytes, into pinned memory
and into a newly allocated pageable array (what ``tree_statistics`` itself does, four arrays); the MFCC launch on the same
batch (slot 0); the streaming floor — the features read once, at 8 TB/s —; and the host twin (mfa_debug_tree_acc_host, one
thread) on the first ``--host-utts`` utterances of the same data, with its rate carried to the whole batch.  GPU.
  python tools/tree_acc_rate.py [--utts 8192] [--seconds 10] [--rounds 10] [--host-utts 200] [--commit ID]
                                [--out profiles/tree_acc_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd.engine import AlignmentEngine, tree_statistics, tree_statistics_host
from montreal_forced_aligner_amd.model import TransitionModel

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--phones", type=int, default=72)
ap.add_argument("--dim", type=int, default=40)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-utts", type=int, default=200)
ap.add_argument("--commit", default="", help="recorded in the report; default: git rev-parse --short HEAD")
ap.add_argument("--out", default="profiles/tree_acc_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

rng = np.random.default_rng(1)
NP_, D = args.phones, args.dim
SIL = (1, 2)
bakis = [K.HmmState(i, i, [(i, 0.75), (i + 1, 0.25)]) for i in range(3)] + [K.HmmState(-1, -1, [])]
topo = K.HmmTopology(np.arange(1, NP_ + 1, dtype=np.int32), np.concatenate([[-1], np.zeros(NP_, np.int32)]).astype(np.int32), [bakis])
tm = TransitionModel(mle.init_mono(topo, 2)[0])
state_of = {(int(r[0]), int(r[1])): ts + 1 for ts, r in enumerate(tm.tuples)}
fwd = np.zeros((NP_ + 1, 3), np.int32)
loop = np.zeros((NP_ + 1, 3), np.int32)
for p in range(1, NP_ + 1):
    for hs in range(3):
        ts = state_of[(p, hs)]
        loop[p, hs], fwd[p, hs] = tm.transition_id(ts, 0), tm.transition_id(ts, 1)

eng = AlignmentEngine(0)
eng.configure_mfcc(snip_edges=1)
rate = eng.model_rate()
n_in = int(args.seconds * rate)
gen = torch.Generator(device=eng.device).manual_seed(1)
pcm = (1500.0 * torch.randn((args.utts, n_in), device=eng.device, generator=gen)).to(torch.int16).reshape(-1)   # (an input, not the product)
so = np.arange(args.utts + 1, dtype=np.int64) * n_in
mfcc, fo = eng.mfcc(pcm, so)
fo = np.asarray(fo, dtype=np.int64)
T = int(fo[-1])
del mfcc


succ = rng.integers(3, NP_ + 1, size=(NP_ + 1, 24))


def utterance(n):
    """``n`` >= 3 frames of whole phones: the last one takes what is left."""
    out = np.empty(n, np.int32)
    t, p = 0, SIL[0]
    while t < n:
        p = int(rng.choice(SIL)) if rng.random() < 0.05 else int(succ[p, rng.integers(24)])
        d = rng.integers(1, 7, size=3) * (4 if p in SIL else 1)
        if n - t - int(d.sum()) < 3:
            d = np.array([1, 1, n - t - 2])
        for hs in range(3):
            out[t] = fwd[p, hs]
            out[t + 1: t + d[hs]] = loop[p, hs]
            t += int(d[hs])
    return out


base = [utterance(int(fo[1] - fo[0])) for _ in range(min(1024, args.utts))]
ali_host = np.concatenate([base[u % len(base)] if fo[u + 1] - fo[u] == len(base[0]) else utterance(int(fo[u + 1] - fo[u]))
                           for u in range(args.utts)]).astype(np.int32)
feats = torch.randn((T, D), dtype=torch.float32, device=eng.device, generator=gen) * 5.0
ali = torch.from_numpy(ali_host).to(eng.device)

for _ in range(args.warmup):
    st, _fe, skipped = tree_statistics(eng, feats, fo, ali, tm, SIL)
    eng.mfcc(pcm, so)
torch.cuda.synchronize()
cap = st.num_events

eng.kernel_timing(True)
stage = {"keys": [], "order": [], "sums": []}
t_mfcc, t_wall, t_down, t_page = [], [], [], []
first = None
rows = torch.zeros((cap, 2 * D + 2), dtype=torch.float64, device=eng.device)      # the event rows' size: key, count, sums
pinned = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
pinned.copy_(rows)
for _ in range(args.rounds):
    eng.reset_kernel_times()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, _fe, _sk = tree_statistics(eng, feats, fo, ali, tm, SIL, cap=cap)
    torch.cuda.synchronize()
    t_wall.append((time.perf_counter() - t0) * 1e3)
    for k, name in enumerate(stage):
        stage[name].append(eng._kernel_time(21 + k)["ms"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pinned.copy_(rows)
    torch.cuda.synchronize()
    t_down.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    rows.cpu()
    t_page.append((time.perf_counter() - t0) * 1e3)
    eng.mfcc(pcm, so)
    torch.cuda.synchronize()
    t_mfcc.append(eng.kernel_times()["mfcc"]["ms"])
    bits = got.keys.tobytes() + got.sum.tobytes() + got.sumsq.tobytes()
    first = bits if first is None else first
    reproducible = first == bits
eng.kernel_timing(False)

n_host = min(args.utts, args.host_utts)
f_host = int(fo[n_host])
x_host = feats[:f_host].cpu().numpy()
t0 = time.perf_counter()
twin, _tfe, tskipped = tree_statistics_host(x_host, fo[: n_host + 1], ali_host[:f_host], tm, SIL)
t_host = (time.perf_counter() - t0) * 1e3
part, _pfe, pskipped = tree_statistics(eng, feats[:f_host], fo[: n_host + 1], ali[:f_host], tm, SIL)
keys_equal = bool(np.array_equal(part.keys, twin.keys) and np.array_equal(part.count, twin.count) and pskipped == tskipped)

med = lambda v: float(np.median(v))
floor_ms = T * D * 4 / 8e12 * 1e3
total = sum(med(v) for v in stage.values())
big = int((got.count > int(eng.lib.mfa_tree_acc_chunk_frames())).sum())
rep = {"commit": commit, "utterances": args.utts, "seconds_per_utterance": args.seconds, "frames": T, "dim": D, "phones": NP_,
       "events": int(got.num_events), "events_longer_than_a_chunk": big, "largest_event_frames": int(got.count.max()),
       "median_event_frames": float(np.median(got.count)), "skipped": int(skipped),
       "chunk_frames": int(eng.lib.mfa_tree_acc_chunk_frames()), "rounds": args.rounds,
       "keys_ms": round(med(stage["keys"]), 4), "order_ms": round(med(stage["order"]), 4), "sums_ms": round(med(stage["sums"]), 4),
       "stages_total_ms": round(total, 4),
       "stages_total_ms_min": round(float(np.min(np.sum([stage[k] for k in stage], axis=0))), 4),
       "call_wall_ms_with_host_copies": round(med(t_wall), 2), "event_row_bytes": int(rows.numel() * 8),
       "event_download_pinned_ms": round(med(t_down), 3), "event_download_new_pageable_array_ms": round(med(t_page), 3),
       "mfcc_ms": round(med(t_mfcc), 4), "feature_bytes": T * D * 4, "streaming_floor_ms_at_8TBps": round(floor_ms, 4),
       "host_twin_utterances": n_host, "host_twin_frames": f_host, "host_twin_ms": round(t_host, 1),
       "host_twin_ms_whole_batch_at_that_rate": round(t_host * T / max(f_host, 1), 0),
       "device_keys_and_counts_equal_host_twin": keys_equal, "two_rounds_same_bits": bool(reproducible)}
print(f"{T} frames x {D}, {rep['events']} events ({big} longer than a chunk): keys {rep['keys_ms']:.3f} + order {rep['order_ms']:.3f} + sums "
      f"{rep['sums_ms']:.3f} = {total:.3f} ms; event download {rep['event_download_pinned_ms']:.3f} ms pinned / {rep['event_download_new_pageable_array_ms']:.3f} ms pageable; call {rep['call_wall_ms_with_host_copies']:.2f} ms; MFCC {rep['mfcc_ms']:.3f} ms; floor "
      f"{floor_ms:.3f} ms; host twin {t_host:.0f} ms on {f_host} frames", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
