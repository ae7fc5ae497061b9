"""Silhouette time on resident inputs, on the corpus of tools/cluster_rate.py: N generated utterance vectors (speakers of ``--utts``
utterances, D = 50), ordered by speaker as ``cluster.silhouette_samples`` orders them → the pair form's prepare and pack (timing
slot 36), the offset check (43) and the silhouette sweep (44), for the plda, euclidean and dot metrics, the median over ``--rounds``
calls by the library's event pairs.  Beside them, at the same N, one neighbour-bits sweep (36, 37) — the sweep DBSCAN pays — and
the ratio of the two sweeps, and a streaming pass over the vectors (a torch reduction, by HIP events) as the floor of anything
that reads them.  ``--layouts`` adds cluster sizes other than the speakers' (one sweep each, euclidean): where the boundary work
goes.  No number here gates anything.  GPU.
  python tools/silhouette_rate.py [--sizes 4096,32768] [--dim 50] [--rounds 5] [--layouts 1,4,64,1024] [--out profiles/silhouette_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import metric_sweep, plda_scores, score_threshold, silhouette

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,32768")
ap.add_argument("--dim", type=int, default=50)
ap.add_argument("--utts", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layouts", default="1,4,64,1024", help="other cluster sizes to time the euclidean sweep at; '' for none")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/silhouette_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

D = args.dim
rng = np.random.default_rng(1)
model = P.PldaModel(np.zeros(D), np.eye(D), np.full(D, 16.0))     # between-speaker variance 16, within 1, in the model's space
eng = AlignmentEngine(0)
dev = eng.device
med = lambda v: float(np.median(v))


def slot_times(fn, slots):
    fn()
    torch.cuda.synchronize()
    ms = {s: [] for s in slots}
    extra = None
    for _ in range(args.rounds):
        eng.reset_kernel_times()
        extra = fn()
        torch.cuda.synchronize()
        for s in slots:
            ms[s].append(eng.kernel_time(s)["ms"])
    return {s: round(med(v), 4) for s, v in ms.items()}, extra


def equal_offsets(n, size):
    return np.unique(np.concatenate([np.arange(0, n, size), [n]])).astype(np.int32)


SIL_SLOTS = ["plda_prepare", "silhouette_offsets", "silhouette_sweep"]
eng.kernel_timing(True)
rep = {"commit": commit, "dim": D, "utts_per_speaker": args.utts, "rounds": args.rounds, "sizes": {}}
for N in (int(s) for s in args.sizes.split(",")):
    speakers = np.arange(N) // args.utts
    means = rng.standard_normal((speakers.max() + 1, D)) * 4.0
    x = torch.from_numpy(means[speakers] + rng.standard_normal((N, D))).to(dev)          # ordered by speaker
    offsets = equal_offsets(N, args.utts)
    m = min(N, 1024)
    sample = -plda_scores(eng, model, x[:m], x[:m])
    same = speakers[:m, None] == speakers[None, :m]
    thr = score_threshold("plda", 0.5 * (np.max(sample[same]) + np.min(sample[~same])))
    cur = {"clusters": int(offsets.shape[0] - 1), "score_matrix_bytes": N * N * 8}
    cur["neighbor_bits_sweep"], _ = slot_times(lambda: metric_sweep(eng, "plda", x, x, thr, model)[3], ["plda_prepare", "plda_sweep"])
    for metric in ("plda", "euclidean", "dot"):
        t, res = slot_times(lambda: silhouette(eng, metric, x, offsets, model), SIL_SLOTS)
        t["score"] = round(float(res["sil"].mean()), 6)
        t["sweep_over_neighbor_sweep"] = round(t["silhouette_sweep"] / cur["neighbor_bits_sweep"]["plda_sweep"], 3)
        cur[metric] = t
    cur["euclidean_by_cluster_size"] = {}
    for size in (int(s) for s in args.layouts.split(",") if s):
        if 2 <= (N + size - 1) // size <= N and size < N:
            off = equal_offsets(N, size)
            t, _ = slot_times(lambda: silhouette(eng, "euclidean", x, off), SIL_SLOTS)
            cur["euclidean_by_cluster_size"][str(size)] = t["silhouette_sweep"]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = []
    for _ in range(args.rounds + 1):
        a.record()
        x.sum()
        b.record()
        torch.cuda.synchronize()
        stream.append(a.elapsed_time(b))
    cur["stream_vectors_ms"] = round(med(stream[1:]), 4)
    rep["sizes"][str(N)] = cur
    print(f"N {N}: {json.dumps(cur)}", flush=True)
    del x
eng.kernel_timing(False)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
