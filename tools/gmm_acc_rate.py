"""GMM statistics time per call on resident inputs, at the benchmark's shape: 8 192 utterances × 10 s (about 1 000 frames
each) and a model of BASELINE configs[2]'s shape (5 000 pdfs × 32 Gaussians, dim 40; seeded random parameters — the work
does not depend on their values).  Alignments are runs of 3 – 12 frames per pdf with one "silence" pdf on 15 % of the frames.
Reported: the median over ``--rounds`` calls of mfa_gmm_acc_batch per stage, by the library's event pairs (mfa_kernel_timing,
slots 8 – 11: lookup, ordering, sums, reduction); the MFCC launch on the same batch (slot 0); the streaming floor — features
read once and accumulators read and written once, at 8 TB/s —; and the host twin (mfa_debug_gmm_acc_host, one thread) on the
first ``--host-frames`` frames of the same data, with its rate carried to the whole batch.  Beside the one-feature stages
the same four slots of mfa_gmm_acc_twofeats_batch on the same batch (``two_feats``: the second matrix is an affine image of
the first, resident as well), when the library has it (an older build under MFA_HIP_SO has not).  GPU.
  python tools/gmm_acc_rate.py [--utts 8192] [--seconds 10] [--rounds 10] [--host-frames 200000] [--commit ID]
                               [--out profiles/gmm_acc_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.engine import AlignmentEngine, GmmStats, gmm_statistics, gmm_statistics_host, gmm_statistics_twofeats

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--pdfs", type=int, default=5000)
ap.add_argument("--gauss", type=int, default=32)
ap.add_argument("--dim", type=int, default=40)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-frames", type=int, default=200000)
ap.add_argument("--commit", default="", help="recorded in the report; default: git rev-parse --short HEAD")
ap.add_argument("--out", default="profiles/gmm_acc_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

rng = np.random.default_rng(1)
P, NG, D = args.pdfs, args.gauss, args.dim
G = P * NG
mean = rng.normal(0, 3, size=(G, D))
var = rng.uniform(0.5, 4.0, size=(G, D))
w = rng.dirichlet(np.ones(NG), size=P).reshape(G)
gc = np.log(w) - 0.5 * (D * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
am = M.DiagGmmModel(D, gc.astype(np.float32), (mean / var).astype(np.float32), (1.0 / var).astype(np.float32),
                    (np.arange(P + 1) * NG).astype(np.int32))
tm = SimpleNamespace(id2pdf=np.concatenate([[-1], np.repeat(np.arange(P), 2)]).astype(np.int32), num_transition_ids=2 * P)

eng = AlignmentEngine(0)
eng.configure_mfcc(snip_edges=1)
rate = eng.model_rate()
n_in = int(args.seconds * rate)
gen = torch.Generator(device=eng.device).manual_seed(1)
pcm = (1500.0 * torch.randn((args.utts, n_in), device=eng.device, generator=gen)).to(torch.int16).reshape(-1)   # (an input, not the product)
so = np.arange(args.utts + 1, dtype=np.int64) * n_in
mfcc, fo = eng.mfcc(pcm, so)
T = int(fo[-1])
del mfcc

# alignments: runs of 3 – 12 frames; pdf 0 ("silence") takes 15 % of the runs
runs = rng.integers(3, 13, size=T // 3 + 1)
runs = runs[: int(np.searchsorted(np.cumsum(runs), T)) + 1]
run_pdf = np.where(rng.random(len(runs)) < 0.15, 0, rng.integers(0, P, size=len(runs)))
pdf_of_frame = np.repeat(run_pdf, runs)[:T]
ali_host = (2 * pdf_of_frame + 1).astype(np.int32)
# features near the aligned pdf's first Gaussian (float32 on the host in slices: 1.3 GB at the default shape)
feats = torch.empty((T, D), dtype=torch.float32, device=eng.device)
for a in range(0, T, 1 << 20):
    b = min(T, a + (1 << 20))
    g = pdf_of_frame[a:b] * NG
    feats[a:b] = torch.from_numpy((mean[g] + np.sqrt(var[g]) * rng.normal(size=(b - a, D))).astype(np.float32)).to(eng.device)
ali = torch.from_numpy(ali_host).to(eng.device)

eng.load_gmm(am)
st = GmmStats.zeros(G, D, 2 * P + 1)
for _ in range(args.warmup):
    gmm_statistics(eng, feats, ali, tm, into=st)
    eng.mfcc(pcm, so)
torch.cuda.synchronize()

eng.kernel_timing(True)
stage = {"lookup": [], "order": [], "sums": [], "reduce": []}
t_mfcc, t_wall = [], []
first = None
for _ in range(args.rounds):
    eng.reset_kernel_times()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = gmm_statistics(eng, feats, ali, tm)
    torch.cuda.synchronize()
    t_wall.append((time.perf_counter() - t0) * 1e3)
    for k, name in enumerate(stage):
        stage[name].append(eng._kernel_time(8 + k)["ms"])
    eng.mfcc(pcm, so)
    torch.cuda.synchronize()
    t_mfcc.append(eng.kernel_times()["mfcc"]["ms"])
    bits = got.occ.tobytes() + got.mean_acc.tobytes() + got.var_acc.tobytes()
    first = bits if first is None else first
    reproducible = first == bits

# the two-feature path: the same batch, the sums from a second resident matrix
two = None
if hasattr(eng.lib, "mfa_gmm_acc_twofeats_batch"):
    feats_sum = feats * 0.9 + 0.25
    for _ in range(args.warmup):
        gmm_statistics_twofeats(eng, feats, feats_sum, ali, tm, into=st)
    torch.cuda.synchronize()
    two = {"lookup": [], "order": [], "sums": [], "reduce": []}
    for _ in range(args.rounds):
        eng.reset_kernel_times()
        torch.cuda.synchronize()
        got2 = gmm_statistics_twofeats(eng, feats, feats_sum, ali, tm)
        torch.cuda.synchronize()
        for k, name in enumerate(two):
            two[name].append(eng._kernel_time(8 + k)["ms"])
    two_follows_post = bool(got2.occ.tobytes() == got.occ.tobytes() and got2.tot_like == got.tot_like
                            and got2.mean_acc.tobytes() != got.mean_acc.tobytes())
    del feats_sum
eng.kernel_timing(False)

n_host = min(T, args.host_frames)
x_host = feats[:n_host].cpu().numpy()
t0 = time.perf_counter()
twin = gmm_statistics_host(am, x_host, ali_host[:n_host], tm)
t_host = (time.perf_counter() - t0) * 1e3
part = gmm_statistics(eng, feats[:n_host], ali[:n_host], tm)
counts_equal = bool(np.array_equal(part.tid_count, twin.tid_count) and part.tot_count == twin.tot_count)

med = lambda v: float(np.median(v))
acc_bytes = G * (2 * D + 1) * 8
floor_ms = (T * D * 4 + 2 * acc_bytes) / 8e12 * 1e3
total = sum(med(v) for v in stage.values())
rep = {"commit": commit, "utterances": args.utts, "seconds_per_utterance": args.seconds, "frames": T, "dim": D, "pdfs": P,
       "gaussians_per_pdf": NG, "chunk_frames": int(eng.lib.mfa_gmm_acc_chunk_frames()), "rounds": args.rounds,
       "lookup_ms": round(med(stage["lookup"]), 4), "order_ms": round(med(stage["order"]), 4), "sums_ms": round(med(stage["sums"]), 4),
       "reduce_ms": round(med(stage["reduce"]), 4), "stages_total_ms": round(total, 4),
       "stages_total_ms_min": round(float(np.min(np.sum([stage[k] for k in stage], axis=0))), 4),
       "call_wall_ms_with_host_copies": round(med(t_wall), 2), "mfcc_ms": round(med(t_mfcc), 4),
       "feature_bytes": T * D * 4, "accumulator_bytes": acc_bytes, "streaming_floor_ms_at_8TBps": round(floor_ms, 4),
       "host_twin_frames": n_host, "host_twin_ms": round(t_host, 1), "host_twin_ms_whole_batch_at_that_rate": round(t_host * T / n_host, 0),
       "device_counts_equal_host_twin": counts_equal, "two_rounds_same_bits": bool(reproducible)}
if two is not None:
    rep["two_feats"] = {"lookup_ms": round(med(two["lookup"]), 4), "order_ms": round(med(two["order"]), 4),
                        "sums_ms": round(med(two["sums"]), 4), "reduce_ms": round(med(two["reduce"]), 4),
                        "stages_total_ms": round(sum(med(v) for v in two.values()), 4),
                        "sums_ms_all_rounds": [round(v, 4) for v in two["sums"]],
                        "occ_and_loglike_equal_one_feature": two_follows_post}
rep["sums_ms_all_rounds"] = [round(v, 4) for v in stage["sums"]]
print(f"{T} frames x {D}, {P} pdfs x {NG}: lookup {rep['lookup_ms']:.3f} + order {rep['order_ms']:.3f} + sums {rep['sums_ms']:.3f} + reduce "
      f"{rep['reduce_ms']:.3f} = {total:.3f} ms; MFCC {rep['mfcc_ms']:.3f} ms; floor {floor_ms:.3f} ms; host twin {t_host:.0f} ms on {n_host} frames",
      flush=True)
if two is not None:
    t2 = rep["two_feats"]
    print(f"two features: lookup {t2['lookup_ms']:.3f} + order {t2['order_ms']:.3f} + sums {t2['sums_ms']:.3f} + reduce {t2['reduce_ms']:.3f} "
          f"= {t2['stages_total_ms']:.3f} ms", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
