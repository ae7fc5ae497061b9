"""I-vector extractor time per launch group on resident inputs, at the reference's defaults: 256 Gaussians, dim 40, i-vector
dimension 192, lists of 20, ``--utts`` utterances of about ``--frames`` frames (seeded random features, distinct random lists,
posteriors pruned at 0.025).  Reported: the median over ``--rounds`` calls, by the library's event pairs, of the pruning (slot
29), the utterance statistics γ and X (30) and the global S (31), and of one training E-step: the products Q and lin (32), the
per-utterance solve (33), the accumulating products (34); beside them the extraction E-step (no accumulators), the f64 matrix
floors computed from the shapes over the FP64 matrix peak (78.6 TFLOP/s; 2 048 flop per 16×16×4 instruction, the tiles the
kernels issue for the statistics, 2·M·N·K for the products), and the host twins on ``--threads`` threads over the first
``--host-utts`` utterances, their rate carried to the whole batch.  GPU.
  python tools/ivector_rate.py [--utts 8192] [--frames 200] [--rounds 5] [--host-utts 64] [--out profiles/ivector_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import ivector as IV
from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import (ivector_estep, ivector_estep_host, ivector_utterance_statistics,
                                               ivector_utterance_statistics_host, prune_posteriors, prune_posteriors_host)

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--gauss", type=int, default=256)
ap.add_argument("--dim", type=int, default=40)
ap.add_argument("--ivector-dim", type=int, default=192)
ap.add_argument("--gselect", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--host-utts", type=int, default=64)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/ivector_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

rng = np.random.default_rng(1)
G, D, R, N, U = args.gauss, args.dim, args.ivector_dim, args.gselect, args.utts
P, PD = R * (R + 1) // 2, D * (D + 1) // 2
eng = AlignmentEngine(0)
dev = eng.device
lengths = rng.integers(args.frames - args.frames // 4, args.frames + args.frames // 4 + 1, size=U)
off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
T = int(off[-1])
gen = torch.Generator(device=dev).manual_seed(1)
feats = 2.0 * torch.randn((T, D), device=dev, generator=gen)
gs = torch.empty((T, N), dtype=torch.int32, device=dev)
raw = torch.empty((T, N), dtype=torch.float32, device=dev)
for a in range(0, T, 1 << 18):                                           # distinct lists: the N largest of G random keys
    b = min(T, a + (1 << 18))
    gs[a:b] = torch.rand((b - a, G), device=dev, generator=gen).topk(N, dim=1).indices.to(torch.int32)
    e = torch.rand((b - a, N), device=dev, generator=gen) ** 6
    raw[a:b] = e / e.sum(dim=1, keepdim=True)
M = rng.normal(size=(G, D, R)) * 0.3
A = rng.normal(size=(G, D, D)) * 0.1 + np.eye(D)
model = IV.IvectorExtractorModel(np.full(G, 1.0 / G), M, A @ A.transpose(0, 2, 1), 100.0)
med = lambda v: float(np.median(v))


def timed(fn, slots):
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
rep = {"commit": commit, "utterances": U, "frames": T, "gauss": G, "dim": D, "ivector_dim": R, "num_gselect": N, "rounds": args.rounds,
       "scatter_slab_frames": int(eng.lib.mfa_ivector_scatter_slab_frames())}
rep.update(timed(lambda: prune_posteriors(eng, raw, 0.025, 5.0), ["ivec_prune"]))
post = prune_posteriors(eng, raw, 0.025, 5.0)
rep.update(timed(lambda: ivector_utterance_statistics(eng, feats, off, gs, post, G), ["ivec_utt"]))
rep.update(timed(lambda: ivector_utterance_statistics(eng, feats, off, gs, post, G, want_S=True), ["ivec_scatter"]))
gamma, X, S = ivector_utterance_statistics(eng, feats, off, gs, post, G, want_S=True)


def train_estep():
    st = IV.IvectorStats.zeros(G, D, R)
    ivector_estep(eng, model, gamma, X, into=st)
    return st


rep["train_estep"] = timed(train_estep, ["ivec_products", "ivec_solve", "ivec_acc"])
rep["extract_estep"] = timed(lambda: ivector_estep(eng, model, gamma, X), ["ivec_products", "ivec_solve"])
a, b = train_estep(), train_estep()
rep["two_calls_same_bits"] = bool(all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("gamma", "Y", "Rq", "isum", "iscat")))

peak = 78.6e12
tiles = float(np.sum((lengths + 3) // 4))
rep["floors_ms"] = {
    "ivec_utt": round(tiles * (-(-G // 16)) * (-(-(D + 1) // 16)) * 2048 / peak * 1e3, 4),
    "ivec_scatter": round((T / 4) * (-(-G // 16)) * (-(-PD // 64) * 4) * 2048 / peak * 1e3, 4),
    "ivec_products": round((2.0 * U * G * P + 2.0 * U * G * D * R) / peak * 1e3, 4),
    "ivec_acc": round((2.0 * U * G * P + 2.0 * U * G * D * R) / peak * 1e3, 4),
}
rep["solve_fma_per_utterance"] = int(R ** 3 // 6 + R ** 3 // 6 + R ** 3 // 6 + R * R)   # Cholesky, inverse, Var, the two solves

# the host twins on ``threads`` threads (the library call releases the interpreter lock), on the first utterances
n_host = min(U, args.host_utts)
cuts = np.linspace(0, n_host, args.threads + 1).astype(int)
xh, gh, ph, rh = (t[: off[n_host]].cpu().numpy() for t in (feats, gs, post, raw))
gam_h, X_h = gamma[:n_host].cpu().numpy(), X[:n_host].cpu().numpy()
model.derived()
with ThreadPoolExecutor(args.threads) as pool:
    part = lambda i: slice(int(off[cuts[i]]), int(off[cuts[i + 1]]))
    t0 = time.perf_counter()
    list(pool.map(lambda i: prune_posteriors_host(rh[part(i)], 0.025, 5.0), range(args.threads)))
    t_prune = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    list(pool.map(lambda i: ivector_utterance_statistics_host(xh[part(i)], off[cuts[i]: cuts[i + 1] + 1] - off[cuts[i]], gh[part(i)],
                                                              ph[part(i)], G, want_S=True), range(args.threads)))
    t_stats = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    list(pool.map(lambda i: ivector_estep_host(model, gam_h[cuts[i]: cuts[i + 1]], X_h[cuts[i]: cuts[i + 1]],
                                               into=IV.IvectorStats.zeros(G, D, R)), range(args.threads)))
    t_estep = (time.perf_counter() - t0) * 1e3
rep["host_twin"] = dict(utterances=n_host, threads=args.threads, prune_ms=round(t_prune, 1), statistics_ms=round(t_stats, 1),
                        estep_ms=round(t_estep, 1), statistics_ms_whole_batch_at_that_rate=round(t_stats * U / n_host, 0),
                        estep_ms_whole_batch_at_that_rate=round(t_estep * U / n_host, 0))
eng.kernel_timing(False)
tr, fl = rep["train_estep"], rep["floors_ms"]
print(f"G {G} D {D} R {R}: {U} utterances, {T} frames, n {N}: prune {rep['ivec_prune']:.3f} ms; γ, X {rep['ivec_utt']:.3f} (floor "
      f"{fl['ivec_utt']:.3f}); S {rep['ivec_scatter']:.3f} (floor {fl['ivec_scatter']:.3f}); E-step products {tr['ivec_products']:.3f} "
      f"(floor {fl['ivec_products']:.3f}) + solve {tr['ivec_solve']:.3f} + accumulate {tr['ivec_acc']:.3f} (floor {fl['ivec_acc']:.3f}) ms; "
      f"twins x{args.threads} on {n_host} utterances: statistics {t_stats:.0f} ms, E-step {t_estep:.0f} ms", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
