"""LDA statistics: time per call on a resident batch of bench.py's shape — 8 192 utterances × 1 000 frames of 13 cepstra, 64
speakers, ±3 splice (S = 91), 2 500 classes, alignments in runs of a few frames, an eighth of the frames silence (weight 0).
  lda          mfa_lda_acc_batch, split by stage with the library's event pairs (mfa_kernel_timing):
               lda_lookup (lookup + CMVN offsets), lda_second (the f64 matrix-pipe kernel), lda_class (sort + class sums),
               lda_reduce (both reductions), and the whole call on the wall clock
  lda_pruned   the same with rand_prune = 4 (the reference's setting): three quarters of the frames take no part
  mfcc         the MFCC launch that makes such a batch from PCM (the front end's heaviest stage, for scale)
  read         a streaming read of the base features (torch sum over the matrix): what a bandwidth-bound pass would cost
  host twin    mfa_debug_lda_acc_host on the first ``--twin-utts`` utterances, wall clock, one thread
Every variant is warmed up, then the variants are launched in turn, ``--rounds`` times; a figure is the median over a
variant's launches (wall clock between two device synchronisations for a whole call, the library's event pairs for a stage
and for the MFCC launch).  The second-moment stage's double-precision rate follows from the frames that take part: frames × tiles ×
16·16 fused multiply-adds (padded tiles included: what the matrix pipe executes).  GPU.
  python tools/lda_rate.py [--rounds 10] [--out profiles/lda_rate.json | --out '']"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import lda_statistics, lda_statistics_host

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--speakers", type=int, default=64)
ap.add_argument("--classes", type=int, default=2500)
ap.add_argument("--context", type=int, default=3)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--twin-utts", type=int, default=16)
ap.add_argument("--out", default="profiles/lda_rate.json", help="report file; '' writes none")
args = ap.parse_args()

eng = AlignmentEngine(0)
dev = eng.device
dim, ctx, C = 13, args.context, args.classes
T = args.utts * args.frames
torch.manual_seed(1)
mfcc = 10.0 * torch.randn((T, dim), device=dev)
fo = np.arange(args.utts + 1, dtype=np.int64) * args.frames
u2s = (np.arange(args.utts) % args.speakers).astype(np.int32)
cmvn = eng.cmvn_stats(mfcc, fo, u2s, args.speakers)
rng = np.random.default_rng(2)
runs = rng.integers(3, 12, size=T // 3 + 1)
ali_host = np.repeat(rng.integers(1, C + 1, size=runs.shape[0]), runs)[:T].astype(np.int32)
ali = torch.from_numpy(ali_host).to(dev)
tid2class = np.concatenate([[0], np.arange(C)]).astype(np.int32)
tid_weight = np.ones(C + 1, np.float32)
tid_weight[0] = 0.0
tid_weight[1: C // 8 + 1] = 0.0                      # "silence": an eighth of the classes weigh 0
tables = (tid2class, tid_weight)
keys = np.arange(args.utts, dtype=np.uint32)
S = (2 * ctx + 1) * dim
nb = (S + 15) // 16
tiles = nb * (nb + 1) // 2
taking = int((tid_weight[ali_host] != 0).sum())

# PCM of the same batch for the MFCC launch: 10 ms shift, 25 ms window, snip_edges off → frames × 160 samples
eng.configure_mfcc()
samples = args.frames * 160
pcm = torch.randint(-3000, 3000, (args.utts * samples,), dtype=torch.int16, device=dev)
so = np.arange(args.utts + 1, dtype=np.int64) * samples
STAGES = ("lda_lookup", "lda_second", "lda_class", "lda_reduce")


def run(name):
    if name == "lda":
        return lda_statistics(eng, mfcc, fo, u2s, cmvn, ali, tables, ctx, num_classes=C)
    if name == "lda_pruned":
        return lda_statistics(eng, mfcc, fo, u2s, cmvn, ali, tables, ctx, num_classes=C, rand_prune=4.0, utt_keys=keys, seed=1)
    if name == "mfcc":
        return eng.mfcc(pcm, so)
    return mfcc.sum()


variants = ["lda", "lda_pruned", "mfcc", "read"]
for v in variants:
    for _ in range(args.warmup):
        run(v)
torch.cuda.synchronize()
eng.kernel_timing(True)
times = {v: [] for v in variants}
stage_ms = {v: {s: [] for s in STAGES} for v in ("lda", "lda_pruned")}
for _ in range(args.rounds):
    for v in variants:
        eng.reset_kernel_times()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(v)
        torch.cuda.synchronize()
        times[v].append((time.perf_counter() - t0) * 1e3)
        if v in stage_ms:
            for s in STAGES:
                stage_ms[v][s].append(eng.kernel_time(s)["ms"])
        if v == "mfcc":
            times[v][-1] = eng.kernel_time("mfcc")["ms"]
        del out
eng.kernel_timing(False)


def med(a):
    a = np.asarray(a)
    return {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4)}


rep = {"utterances": args.utts, "frames_per_utterance": args.frames, "speakers": args.speakers, "classes": C, "spliced_dim": S,
       "tiles": tiles, "frames_taking_part": taking, "launches_per_variant": args.rounds, "ms": {}}
for v in variants:
    rep["ms"][v] = med(times[v])
    print(f"{v:12s} median {rep['ms'][v]['median']:9.4f} ms  (min {rep['ms'][v]['min']:.4f}, max {rep['ms'][v]['max']:.4f})", flush=True)
    if v in stage_ms:
        rep["ms"][v]["stages"] = {s: med(stage_ms[v][s]) for s in STAGES}
        for s in STAGES:
            print(f"    {s:12s} median {rep['ms'][v]['stages'][s]['median']:9.4f} ms", flush=True)
rep["ms"]["lda"]["note"] = "whole call: host-side uploads and downloads of the accumulators included; stages: device time"
sec = rep["ms"]["lda"]["stages"]["lda_second"]["median"]
rep["second_moment_f64_tflops_executed"] = round(2.0 * T * tiles * 256 / (sec * 1e-3) / 1e12, 2)       # every staged frame is issued
rep["second_moment_f64_tflops_useful"] = round(2.0 * taking * S * (S + 1) / 2 / (sec * 1e-3) / 1e12, 2)
rep["read_GBps"] = round(T * dim * 4 / (rep["ms"]["read"]["median"] * 1e-3) / 1e9, 1)
print(f"second moment: {rep['second_moment_f64_tflops_executed']} TFLOP/s f64 executed on the matrix pipe, "
      f"{rep['second_moment_f64_tflops_useful']} useful; streaming read {rep['read_GBps']} GB/s", flush=True)

n = min(args.twin_utts, args.utts)
fe = int(fo[n])
h_mfcc, h_cmvn = mfcc[:fe].cpu().numpy(), cmvn.cpu().numpy()
t0 = time.perf_counter()
lda_statistics_host(h_mfcc, fo[: n + 1], u2s[:n], h_cmvn, ali_host[:fe], tables, ctx, num_classes=C)
dt = time.perf_counter() - t0
rep["host_twin"] = {"utterances": n, "frames": fe, "seconds": round(dt, 3), "Mframes_per_s": round(fe / dt / 1e6, 4)}
print(f"host twin: {fe} frames in {dt:.3f} s = {fe / dt / 1e6:.4f} Mframes/s (one thread)", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
