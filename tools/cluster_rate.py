"""Speaker clustering time on resident inputs: N generated utterance vectors (speakers of ``--utts`` utterances, D = 50, the plda
metric) → the neighbour sweep (timing slots 36, 37) → DBSCAN on the bits: symmetrise (39), degree (40), the rounds (41, with their
count) and the labels (42), the median over ``--rounds`` calls by the library's event pairs.  Beside them, at the same N, the
route that existed before the bit matrix — ``plda_scores`` to a stored matrix on the host, then DBSCAN restated in numpy on
it (wall clock, once) — and a streaming pass over the bit matrix (a torch reduction over its words, by HIP events) as the floor
of anything that reads it.  No number here gates anything.  GPU.
  python tools/cluster_rate.py [--sizes 4096,32768] [--dim 50] [--rounds 5] [--out profiles/cluster_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import dbscan_from_bits, metric_sweep, plda_scores, score_threshold

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096,32768")
ap.add_argument("--dim", type=int, default=50)
ap.add_argument("--utts", type=int, default=16)
ap.add_argument("--min-samples", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-route-max", type=int, default=32768, help="largest N at which the stored-matrix route is run")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/cluster_rate.json", help="report file; '' writes none")
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


def numpy_dbscan(adj, min_samples):
    """The rules of the device path on a boolean matrix, components by frontier expansion."""
    adj |= adj.T
    np.fill_diagonal(adj, True)
    core = adj.sum(axis=1) >= min_samples
    labels = np.full(adj.shape[0], -1, dtype=np.int32)
    nxt = 0
    for s in np.flatnonzero(core):
        if labels[s] >= 0:
            continue
        front = np.array([s])
        labels[s] = nxt
        while front.size:
            reach = adj[front].any(axis=0) & core & (labels < 0)
            labels[reach] = nxt
            front = np.flatnonzero(reach)
        nxt += 1
    for i in np.flatnonzero(~core):
        near = labels[adj[i] & core]
        if near.size:
            labels[i] = near.min()
    return labels


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


eng.kernel_timing(True)
rep = {"commit": commit, "dim": D, "utts_per_speaker": args.utts, "min_samples": args.min_samples, "rounds": args.rounds, "sizes": {}}
for N in (int(s) for s in args.sizes.split(",")):
    speakers = np.arange(N) // args.utts
    order = rng.permutation(N)
    means = rng.standard_normal((speakers.max() + 1, D)) * 4.0
    x = torch.from_numpy((means[speakers] + rng.standard_normal((N, D)))[order]).to(dev)
    speakers = speakers[order]
    # ε from a sample: between the largest within-speaker and the smallest between-speaker distance there
    m = min(N, 1024)
    sample = -plda_scores(eng, model, x[:m], x[:m])
    same = speakers[:m, None] == speakers[None, :m]
    eps = 0.5 * (np.max(sample[same]) + np.min(sample[~same]))
    thr = score_threshold("plda", eps)
    cur = {"eps": round(float(eps), 4), "bit_matrix_bytes": N * ((N + 63) // 64) * 8, "score_matrix_bytes": N * N * 8}
    t, bits = slot_times(lambda: metric_sweep(eng, "plda", x, x, thr, model)[3], ["plda_prepare", "plda_sweep"])
    cur["sweep"] = t
    pristine = bits.clone()
    work = torch.empty_like(bits)

    def cluster():
        work.copy_(pristine)
        return dbscan_from_bits(eng, work, args.min_samples)

    t, res = slot_times(cluster, ["cluster_symmetrise", "cluster_degree", "cluster_rounds", "cluster_labels"])
    cur["dbscan"] = dict(t, rounds=res["rounds"], n_clusters=res["n_clusters"], noise=int((res["labels"] < 0).sum()))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = []
    for _ in range(args.rounds + 1):
        a.record()
        pristine.sum()
        b.record()
        torch.cuda.synchronize()
        stream.append(a.elapsed_time(b))
    cur["stream_bits_ms"] = round(med(stream[1:]), 4)
    cur["device_total_ms"] = round(sum(cur["sweep"].values()) + sum(v for k, v in t.items()), 4)
    if N <= args.host_route_max:
        t0 = time.perf_counter()
        scores = plda_scores(eng, model, x, x, max_bytes=1 << 40)
        t1 = time.perf_counter()
        labels = numpy_dbscan(scores >= thr, args.min_samples)
        t2 = time.perf_counter()
        cur["stored_matrix_route"] = {"plda_scores_to_host_ms": round((t1 - t0) * 1e3, 1), "numpy_dbscan_ms": round((t2 - t1) * 1e3, 1),
                                      "labels_equal_device": bool(np.array_equal(labels, res["labels"].cpu().numpy()))}
        del scores
    rep["sizes"][str(N)] = cur
    print(f"N {N}: {json.dumps(cur)}", flush=True)
    del x, bits, pristine, work
eng.kernel_timing(False)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
