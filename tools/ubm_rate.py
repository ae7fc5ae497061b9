"""Diagonal-UBM time per call on resident inputs, at the benchmark's batch: 8 192 utterances × 10 s, every fifth frame (the
stage's subsample), dim 40, lists of 30, for mixtures of 256 and of 2 048 Gaussians (seeded random parameters; frames drawn
near the Gaussians, so that a frame's best list is a real one).  Reported per mixture: the median over ``--rounds`` calls of
mfa_ubm_gselect_batch (slot 25) and of mfa_ubm_acc_batch over the selection (slots 26 – 28: posteriors, sums, reductions) by
the library's event pairs, and the dense statistics (no selection: the init phase) on ``--init-frames`` frames; beside them
the MFCC launch on the same batch (slot 0), a streaming copy of the features (torch), the arithmetic floors — scoring: G·2·dim
FMAs per frame over the FP32 vector peak (157.3 TFLOP/s); sums: the f64 matrix instructions the dense-tile form issues over
the FP64 matrix peak (78.6 TFLOP/s) — and the host twins on 16 threads over the first ``--host-frames`` frames, their rate
carried to the whole batch.  GPU.
  python tools/ubm_rate.py [--utts 8192] [--seconds 10] [--rounds 10] [--host-frames 64000] [--out profiles/ubm_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import gaussian_selection, gaussian_selection_host, ubm_statistics, ubm_statistics_host
from montreal_forced_aligner_amd.ubm import DiagUbm

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--subsample", type=int, default=5)
ap.add_argument("--dim", type=int, default=40)
ap.add_argument("--gselect", type=int, default=30)
ap.add_argument("--gauss", type=int, nargs="+", default=[256, 2048])
ap.add_argument("--init-frames", type=int, default=500000)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-frames", type=int, default=64000)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/ubm_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

rng = np.random.default_rng(1)
D, N = args.dim, args.gselect
eng = AlignmentEngine(0)
eng.configure_mfcc(snip_edges=1)
rate = eng.model_rate()
n_in = int(args.seconds * rate)
gen = torch.Generator(device=eng.device).manual_seed(1)
pcm = (1500.0 * torch.randn((args.utts, n_in), device=eng.device, generator=gen)).to(torch.int16).reshape(-1)   # (an input, not the product)
so = np.arange(args.utts + 1, dtype=np.int64) * n_in
mfcc, fo = eng.mfcc(pcm, so)
T = int(np.sum((np.diff(fo) + args.subsample - 1) // args.subsample))
del mfcc
med = lambda v: float(np.median(v))


def timed(fn, slots):
    """Median per slot of ``slots`` over the rounds of ``fn``, by the library's event pairs."""
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = {s: [] for s in slots}
    for _ in range(args.rounds):
        eng.reset_kernel_times()
        fn()
        torch.cuda.synchronize()
        for s in slots:
            ms[s].append(eng.kernel_time(s)["ms"])
    return {s: round(med(v), 4) for s, v in ms.items()}


eng.kernel_timing(True)
rep = {"commit": commit, "utterances": args.utts, "seconds_per_utterance": args.seconds, "subsample": args.subsample, "frames": T,
       "dim": D, "num_gselect": N, "rounds": args.rounds, "slab_frames": int(eng.lib.mfa_ubm_acc_slab_frames()), "mixtures": {}}
rep["mfcc_ms"] = timed(lambda: eng.mfcc(pcm, so), ["mfcc"])["mfcc"]

for G in args.gauss:
    mean = rng.normal(0, 2, size=(G, D))
    var = rng.uniform(0.3, 2.0, size=(G, D))
    ubm = DiagUbm.from_parameters(rng.dirichlet(np.ones(G)), mean, var)
    feats = torch.empty((T, D), dtype=torch.float32, device=eng.device)
    for a in range(0, T, 1 << 20):
        b = min(T, a + (1 << 20))
        g = rng.integers(0, G, size=b - a)
        feats[a:b] = torch.from_numpy((mean[g] + 1.3 * np.sqrt(var[g]) * rng.normal(size=(b - a, D))).astype(np.float32)).to(eng.device)
    r = {}
    r.update(timed(lambda: gaussian_selection(eng, feats, ubm, N), ["ubm_select"]))
    gs, _ = gaussian_selection(eng, feats, ubm, N)
    r.update(timed(lambda: ubm_statistics(eng, feats, ubm, gs), ["ubm_post", "ubm_sums", "ubm_reduce"]))
    n_init = min(T, args.init_frames)
    dense = timed(lambda: ubm_statistics(eng, feats[:n_init], ubm), ["ubm_post", "ubm_sums", "ubm_reduce"])
    r["dense_init"] = dict(frames=n_init, **dense)
    a = ubm_statistics(eng, feats, ubm, gs)
    b = ubm_statistics(eng, feats, ubm, gs)
    r["two_calls_same_bits"] = bool(a.occ.tobytes() + a.mean_acc.tobytes() + a.var_acc.tobytes() == b.occ.tobytes() + b.mean_acc.tobytes() + b.var_acc.tobytes())
    # a streaming copy of the features, by torch's events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copies = []
    for _ in range(args.rounds):
        ev[0].record(); feats.clone(); ev[1].record(); torch.cuda.synchronize()
        copies.append(ev[0].elapsed_time(ev[1]))
    r["feature_copy_ms"] = round(med(copies), 4)
    # floors
    r["scoring_floor_ms"] = round(T * G * 2 * D / (157.3e12 / 2) * 1e3, 4)
    ncb = (2 * D + 1 + 15) // 16
    r["sums_mfma_floor_ms"] = round((T / 4) * (-(-G // 16)) * ncb * 2048 / 78.6e12 * 1e3, 4)
    # the host twins on ``threads`` threads (the library call releases the interpreter lock), on the first frames
    n_host = min(T, args.host_frames)
    x = feats[:n_host].cpu().numpy()
    g_host = gs[:n_host].cpu().numpy()
    cuts = np.linspace(0, n_host, args.threads + 1).astype(int)
    with ThreadPoolExecutor(args.threads) as pool:
        t0 = time.perf_counter()
        sel = list(pool.map(lambda i: gaussian_selection_host(x[cuts[i]: cuts[i + 1]], ubm, N)[0], range(args.threads)))
        t_sel = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        list(pool.map(lambda i: ubm_statistics_host(x[cuts[i]: cuts[i + 1]], ubm, g_host[cuts[i]: cuts[i + 1]]), range(args.threads)))
        t_acc = (time.perf_counter() - t0) * 1e3
    r["host_twin"] = dict(frames=n_host, threads=args.threads, select_ms=round(t_sel, 1), statistics_ms=round(t_acc, 1),
                          select_ms_whole_batch_at_that_rate=round(t_sel * T / n_host, 0),
                          statistics_ms_whole_batch_at_that_rate=round(t_acc * T / n_host, 0),
                          selection_equals_device=bool(np.array_equal(np.concatenate(sel), g_host)))
    rep["mixtures"][str(G)] = r
    print(f"G {G}: {T} frames x {D}, n {N}: select {r['ubm_select']:.3f} ms (floor {r['scoring_floor_ms']:.3f}); statistics post "
          f"{r['ubm_post']:.3f} + sums {r['ubm_sums']:.3f} (floor {r['sums_mfma_floor_ms']:.3f}) + reduce {r['ubm_reduce']:.3f} ms; dense on "
          f"{n_init} frames {sum(dense.values()):.3f} ms; copy {r['feature_copy_ms']:.3f} ms; MFCC {rep['mfcc_ms']:.3f} ms; twins x{args.threads} on "
          f"{n_host} frames {t_sel:.0f} + {t_acc:.0f} ms", flush=True)
    del feats, gs
eng.kernel_timing(False)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
