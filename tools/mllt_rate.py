"""MLLT statistics time per call on resident inputs, at the benchmark's shape: 8 192 utterances × 10 s (about 1 000 frames
each) and a model of 4 960 pdfs × 32 Gaussians, dim 40 (seeded random parameters — the work does not depend on their
values).  Alignments are runs of 3 – 12 frames per pdf with one "silence" pdf on 15 % of the frames — at weight 0, as the
MLLT pass of the training stage has it, unless ``--silence-weight 1``.
Reported: the median over ``--rounds`` calls of mfa_mllt_acc_batch per stage, by the library's event pairs (mfa_kernel_timing,
slots 17 – 20: lookup, ordering, sums, reductions); beside it mfa_gmm_acc_batch (slots 8 – 11) and the MFCC launch (slot 0) on
the same batch; the workspace the call lays over the context's shared buffer and the accumulators' size; the f64 matrix
work of the moment phase (tile-padded) and what rate that is; the host twin (mfa_debug_mllt_acc_host, one thread) on the first
``--host-frames`` frames, with its rate carried to the whole batch; and the host time of ``mllt.mllt_accs`` +
``mllt.estimate_mllt`` on the statistics of the whole batch.  GPU.
  python tools/mllt_rate.py [--utts 8192] [--seconds 10] [--rounds 5] [--host-frames 20000] [--commit ID]
                            [--out profiles/mllt_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import mllt
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.engine import AlignmentEngine, gmm_statistics, mllt_statistics, mllt_statistics_host

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--pdfs", type=int, default=4960)
ap.add_argument("--gauss", type=int, default=32)
ap.add_argument("--dim", type=int, default=40)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--silence-weight", type=float, default=0.0)
ap.add_argument("--host-frames", type=int, default=20000)
ap.add_argument("--sweeps", type=int, default=200)
ap.add_argument("--commit", default="", help="recorded in the report; default: git rev-parse --short HEAD")
ap.add_argument("--out", default="profiles/mllt_rate.json", help="report file; '' writes none")
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
weights = np.ones(2 * P + 1, np.float32)
weights[1:3] = args.silence_weight                      # pdf 0 is the "silence" pdf

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
feats = torch.empty((T, D), dtype=torch.float32, device=eng.device)
for a in range(0, T, 1 << 20):
    b = min(T, a + (1 << 20))
    g = pdf_of_frame[a:b] * NG
    feats[a:b] = torch.from_numpy((mean[g] + np.sqrt(var[g]) * rng.normal(size=(b - a, D))).astype(np.float32)).to(eng.device)
ali = torch.from_numpy(ali_host).to(eng.device)
taking_part = int((weights[ali_host] != 0).sum())

eng.load_gmm(am)
for _ in range(args.warmup):
    mllt_statistics(eng, feats, ali, tm, weights)
    gmm_statistics(eng, feats, ali, tm, weights)
    eng.mfcc(pcm, so)
torch.cuda.synchronize()

eng.kernel_timing(True)
names = ("lookup", "order", "sums", "reduce")
mllt_ms, gmm_ms = {k: [] for k in names}, {k: [] for k in names}
t_mfcc = []
first, reproducible, st = None, True, None
for _ in range(args.rounds):
    eng.reset_kernel_times()
    st = mllt_statistics(eng, feats, ali, tm, weights)
    torch.cuda.synchronize()
    for k, name in enumerate(names):
        mllt_ms[name].append(eng._kernel_time(17 + k)["ms"])
    gmm_statistics(eng, feats, ali, tm, weights)
    torch.cuda.synchronize()
    for k, name in enumerate(names):
        gmm_ms[name].append(eng._kernel_time(8 + k)["ms"])
    eng.mfcc(pcm, so)
    torch.cuda.synchronize()
    t_mfcc.append(eng.kernel_times()["mfcc"]["ms"])
    dev = st._dev                                       # compared on the device: the accumulators are 2 GB at this shape
    if first is None:
        first = tuple(t.clone() for t in dev)
    else:
        reproducible = reproducible and all(torch.equal(a, b) for a, b in zip(first, dev))
eng.kernel_timing(False)
del first

n_host = min(T, args.host_frames)
x_host = feats[:n_host].cpu().numpy()
t0 = time.perf_counter()
twin = mllt_statistics_host(am, x_host, ali_host[:n_host], tm, weights)
t_host = (time.perf_counter() - t0) * 1e3
part = mllt_statistics(eng, feats[:n_host], ali[:n_host], tm, weights)
rel = float(np.abs(part.full - twin.full).max() / np.abs(twin.full).max())

# the host half on the whole batch's statistics
t0 = time.perf_counter()
full = st.full                                          # the one download of the pass
t_down = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
beta, Gj = mllt.mllt_accs(st, am)
t_accs = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
try:
    mat, impr, count, _trace = mllt.estimate_mllt(beta, Gj, num_sweeps=args.sweeps)
    estimate = {"objf_impr_per_frame": round(impr / count, 6), "logdet": round(float(np.linalg.slogdet(mat.astype(np.float64))[1]), 6)}
except ValueError as e:                                  # (a batch too small for the dimension)
    estimate = {"error": str(e)}
t_est = (time.perf_counter() - t0) * 1e3

med = lambda v: float(np.median(v))
LT = D * (D + 1) // 2
chunk, sub = int(eng.lib.mfa_mllt_acc_chunk_frames()), int(eng.lib.mfa_gmm_acc_chunk_frames())
rows_max = (T // chunk + 1) * NG + G
srows_max = (T // sub + 1) * NG + G
ws_bytes = 5 * T * 4 + rows_max * LT * 8 + srows_max * 8 + (T // sub + P) * 16      # keys, values, weights; partials; occ; totals
nb = (D + 15) // 16
flop = taking_part * NG * (nb * (nb + 1) // 2) * 16 * 16 * 2          # tile-padded multiply-adds of the moment phase, as flop
m_total = sum(med(v) for v in mllt_ms.values())
g_total = sum(med(v) for v in gmm_ms.values())
rep = {"commit": commit, "utterances": args.utts, "seconds_per_utterance": args.seconds, "frames": T, "frames_taking_part": taking_part,
       "dim": D, "pdfs": P, "gaussians_per_pdf": NG, "chunk_frames": chunk, "rounds": args.rounds,
       "mllt_lookup_ms": round(med(mllt_ms["lookup"]), 4), "mllt_order_ms": round(med(mllt_ms["order"]), 4),
       "mllt_sums_ms": round(med(mllt_ms["sums"]), 4), "mllt_reduce_ms": round(med(mllt_ms["reduce"]), 4),
       "mllt_stages_total_ms": round(m_total, 4),
       "gmm_lookup_ms": round(med(gmm_ms["lookup"]), 4), "gmm_order_ms": round(med(gmm_ms["order"]), 4),
       "gmm_sums_ms": round(med(gmm_ms["sums"]), 4), "gmm_reduce_ms": round(med(gmm_ms["reduce"]), 4),
       "gmm_stages_total_ms": round(g_total, 4), "mllt_over_gmm": round(m_total / g_total, 2), "mfcc_ms": round(med(t_mfcc), 4),
       "moment_phase_f64_tflop_tile_padded": round(flop / 1e12, 4),
       "moment_phase_f64_tflops": round(flop / 1e12 / (med(mllt_ms["sums"]) / 1e3), 2),
       "accumulator_bytes": G * (D * D + 1) * 8, "workspace_bytes": int(ws_bytes),
       "host_twin_frames": n_host, "host_twin_ms": round(t_host, 1), "host_twin_ms_whole_batch_at_that_rate": round(t_host * T / n_host, 0),
       "device_vs_host_twin_max_relative": rel, "two_rounds_same_bits": bool(reproducible),
       "download_ms": round(t_down, 1), "host_mllt_accs_ms": round(t_accs, 1), "host_estimate_mllt_ms": round(t_est, 1),
       "estimate_sweeps": args.sweeps, "estimate": estimate}
print(f"{T} frames x {D} ({taking_part} take part), {P} pdfs x {NG}: MLLT lookup {rep['mllt_lookup_ms']:.3f} + order {rep['mllt_order_ms']:.3f} + "
      f"sums {rep['mllt_sums_ms']:.3f} + reduce {rep['mllt_reduce_ms']:.3f} = {m_total:.3f} ms ({rep['mllt_over_gmm']} x the GMM statistics' "
      f"{g_total:.3f} ms); MFCC {rep['mfcc_ms']:.3f} ms; workspace {ws_bytes / 1e9:.2f} GB; host twin {t_host:.0f} ms on {n_host} frames; "
      f"mllt_accs {t_accs:.0f} ms + estimate_mllt {t_est:.0f} ms on the host", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
