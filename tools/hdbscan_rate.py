"""HDBSCAN time on resident inputs: N generated utterance vectors (speakers of ``--utts`` utterances, D = 50, the plda metric) →
the pair form (timing slot 36) → the core sweep (37, 38) → the Borůvka rounds of the spanning tree (their sweeps 37, merges 38,
component work 41, with the round count; per round: the slot's total over the rounds of a call) → the cluster tree on the host
(wall clock), the median over ``--rounds`` calls by the library's event pairs.  Beside them one neighbour sweep of the same N
(what tools/cluster_rate.py times): the floor of a round.  No number here gates anything.  GPU.
  python tools/hdbscan_rate.py [--sizes 4096,32768] [--dim 50] [--rounds 5] [--out profiles/hdbscan_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import hdbscan as H
from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import core_scores, metric_sweep, mreach_mst, score_to_distance

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,32768")
ap.add_argument("--dim", type=int, default=50)
ap.add_argument("--utts", type=int, default=16)
ap.add_argument("--min-cluster-size", type=int, default=15)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/hdbscan_rate.json", help="report file; '' writes none")
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
min_samples = max(5, args.min_cluster_size // 4)
SLOTS = ["plda_prepare", "plda_sweep", "plda_merge", "cluster_rounds"]


def slot_times(fn):
    fn()
    torch.cuda.synchronize()
    ms = {s: [] for s in SLOTS}
    wall, extra = [], None
    for _ in range(args.rounds):
        eng.reset_kernel_times()
        t0 = time.perf_counter()
        extra = fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        for s in SLOTS:
            ms[s].append(eng.kernel_time(s)["ms"])
    return {s: round(med(v), 4) for s, v in ms.items()}, round(med(wall), 3), extra


eng.kernel_timing(True)
rep = {"commit": commit, "dim": D, "utts_per_speaker": args.utts, "min_cluster_size": args.min_cluster_size, "min_samples": min_samples,
       "rounds": args.rounds, "sizes": {}}
for N in (int(s) for s in args.sizes.split(",")):
    speakers = np.arange(N) // args.utts
    order = rng.permutation(N)
    means = rng.standard_normal((speakers.max() + 1, D)) * 4.0
    x = torch.from_numpy((means[speakers] + rng.standard_normal((N, D)))[order]).to(dev)
    speakers = speakers[order]
    cur = {}
    t, wall, _ = slot_times(lambda: metric_sweep(eng, "plda", x, x, 0.0, model)[3])
    cur["neighbour_sweep"] = {"prepare_ms": t["plda_prepare"], "sweep_ms": t["plda_sweep"]}
    t, wall, pf = slot_times(lambda: core_scores(eng, "plda", x, min_samples - 1, model))
    cur["core"] = {"prepare_ms": t["plda_prepare"], "sweep_ms": t["plda_sweep"], "merge_ms": t["plda_merge"], "wall_ms": wall}
    t, wall, tree = slot_times(lambda: mreach_mst(eng, "plda", pf["y"], pf["q"], pf["core"]))
    r = max(tree["rounds"], 1)
    cur["tree"] = {"rounds": tree["rounds"], "edges_found": tree["found"], "pack_ms": t["plda_prepare"], "sweeps_ms": t["plda_sweep"],
                   "sweep_per_round_ms": round(t["plda_sweep"] / r, 4), "merges_ms": t["plda_merge"], "components_ms": t["cluster_rounds"],
                   "components_per_round_ms": round(t["cluster_rounds"] / r, 4), "wall_ms_with_download_and_sort": wall}
    dist = score_to_distance("plda", tree["score"])
    dist = dist - dist[np.isfinite(dist)].min()
    t0 = time.perf_counter()
    labels = H.cluster_tree_labels(N, tree["lo"], tree["hi"], dist, args.min_cluster_size, 0.0)
    cur["host_tree_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    pairs = set(zip(labels.tolist(), speakers.tolist()))
    cur["clusters"] = int(labels.max()) + 1
    cur["noise"] = int((labels < 0).sum())
    cur["clusters_are_speakers"] = bool(cur["noise"] == 0 and len(pairs) == cur["clusters"] == int(speakers.max()) + 1)
    rep["sizes"][str(N)] = cur
    print(f"N {N}: {json.dumps(cur)}", flush=True)
    del x, pf
eng.kernel_timing(False)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
