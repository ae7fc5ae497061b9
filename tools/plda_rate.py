"""PLDA scoring time per call on resident inputs: N test vectors against the same N as train vectors (the diagonal excluded),
D = 192, for each output mode — the stored matrix (row blocks within ``--matrix-bytes``; reported per block and carried to
the whole matrix), the best column, the k nearest — and the transform.  Reported: the median over ``--rounds`` calls, by the
library's event pairs, of the prepare (slot 36), sweep (37) and merge (38) launches, beside two floors computed here from the
shapes: the f64 matrix pipe's time for the instructions the kernel issues (two per 16 × 16 × 4 tile step, 2 048 flop each,
on padded tiles: 4·Nt·Ns·D flop — a product with K = 2·D at two flop per multiply-add; a count of 8·Nt·Ns·D would be twice
what the pipe has to do) over the FP64 matrix peak of 78.6 TFLOP/s, and the time to stream the bytes the call
writes (``--hbm-gbs``, default 4 000 GB/s: an achievable rate, not the data-sheet's).  One warm-up call per mode, inputs
generated once and kept on the device, nothing else running on it.  GPU.
  python tools/plda_rate.py [--sizes 8192,65536] [--dim 192] [--k 10] [--rounds 5] [--out profiles/plda_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd import plda as P
from montreal_forced_aligner_amd.engine import AlignmentEngine
from montreal_forced_aligner_amd.stats import _plda_score_call, plda_transform

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="8192,65536")
ap.add_argument("--dim", type=int, default=192)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--matrix-bytes", type=int, default=1 << 30, help="device bytes of one stored row block")
ap.add_argument("--hbm-gbs", type=float, default=4000.0)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="profiles/plda_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

D, K = args.dim, args.k
rng = np.random.default_rng(1)
psi = np.sort(np.exp(rng.uniform(np.log(0.05), np.log(8.0), D)))[::-1].copy()
model = P.PldaModel(rng.standard_normal(D), rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D), psi)
eng = AlignmentEngine(0)
dev = eng.device
SLOTS = ["plda_prepare", "plda_sweep", "plda_merge"]
PEAK = 78.6e12
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


def mfma_floor_ms(nt, ns):
    """Two matrix instructions per (16 rows × 16 columns × 4 of K) tile step, on the padded shapes."""
    steps = -(-nt // 16) * -(-ns // 16) * -(-D // 4)
    return 2.0 * steps * 2048 / PEAK * 1e3


eng.kernel_timing(True)
rep = {"commit": commit, "dim": D, "k": K, "rounds": args.rounds, "fp64_matrix_peak_tflops": PEAK / 1e12, "hbm_gbs": args.hbm_gbs, "sizes": {}}
for N in (int(s) for s in args.sizes.split(",")):
    gen = torch.Generator(device=dev).manual_seed(N)
    raw = torch.randn((N, D), device=dev, dtype=torch.float64, generator=gen)
    cur = {"transform": timed(lambda: plda_transform(eng, model, raw), ["plda_transform"])["plda_transform"]}
    x = plda_transform(eng, model, raw)
    n = torch.ones(N, dtype=torch.int32, device=dev)
    rows = max(64, min(N, args.matrix_bytes // (N * 8) // 64 * 64))
    blocks = -(-N // rows)
    modes = {
        "matrix_block": (lambda: _plda_score_call(eng, model, x[:rows], x, n, False, 1, True, False, False), rows, rows * N * 8),
        "best": (lambda: _plda_score_call(eng, model, x, x, n, True, 1, False, True, False), N, N * 12),
        "knn": (lambda: _plda_score_call(eng, model, x, x, n, True, K, False, False, True), N, N * K * 12),
    }
    for name, (fn, nt, written) in modes.items():
        t = timed(fn, SLOTS)
        t["total_ms"] = round(sum(t[s] for s in SLOTS), 4)
        t["mfma_floor_ms"] = round(mfma_floor_ms(nt, N), 4)
        t["write_floor_ms"] = round(written / (args.hbm_gbs * 1e9) * 1e3, 4)
        t["rows"] = nt
        if name == "matrix_block":
            t["blocks_of_the_whole_matrix"] = blocks
            t["whole_matrix_ms_at_that_rate"] = round(t["total_ms"] * N / nt, 2)
        cur[name] = t
        print(f"N {N} D {D} {name}: {t['total_ms']:.3f} ms ({nt} rows; prepare {t['plda_prepare']:.3f}, sweep {t['plda_sweep']:.3f}, merge "
              f"{t['plda_merge']:.3f}); floors: matrix pipe {t['mfma_floor_ms']:.3f}, written bytes {t['write_floor_ms']:.3f} ms", flush=True)
    a = _plda_score_call(eng, model, x, x, n, True, K, False, True, True)
    b = _plda_score_call(eng, model, x, x, n, True, K, False, True, True)
    cur["two_calls_same_bits"] = bool(all(torch.equal(p, q) for s, t in zip(a[1:], b[1:]) for p, q in zip(s, t)))
    rep["sizes"][str(N)] = cur
    del raw, x, a, b
eng.kernel_timing(False)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
