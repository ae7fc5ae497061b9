"""MFCC time per launch on resident inputs: 8 192 utterances × 10 s of 16 kHz PCM (1 000 frames each), default options.
  specialised   the tail with compile-time trip counts and [lane][entry] tables (what the default options take)
  generic       the generic tail, the bit reference (MFA_MFCC_GENERIC=1)
Both are warmed up, then launched in turn, ``--rounds`` times; the figure is the median of a variant's launches, timed by the
library's event pair (mfa_kernel_timing / mfa_kernel_time_ms, which = 0).  GPU.
  python tools/mfcc_rate.py [--rounds 20] [--out profiles/mfcc_rate.json | --out '']
With MFA_HIP_SO=<another build> the same script times that build (A/B against an older library): a build without the switch
runs its one kernel under both names, and the report says so (`paths`)."""
import argparse
import json
import os
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="profiles/mfcc_rate.json", help="report file; '' writes none")
args = ap.parse_args()

eng = AlignmentEngine(0)
eng.configure_mfcc()
n_in = int(args.seconds * 16000)
gen = torch.Generator(device=eng.device).manual_seed(1)
# one utterance's worth of noise around a tone, repeated with a per-utterance shift: the kernel's work does not depend on the signal
t = torch.arange(n_in + args.utts, device=eng.device, dtype=torch.float32) / 16000.0
base = (4000.0 * torch.sin(2 * np.pi * 130.0 * t) + 1500.0 * torch.randn(n_in + args.utts, device=eng.device, generator=gen)).to(torch.int16)
pcm = base.unfold(0, n_in, 1)[: args.utts].contiguous().reshape(-1)
del base, t
so = np.arange(args.utts + 1, dtype=np.int64) * n_in
variants = ["specialised", "generic"]


def run(name):
    os.environ.pop("MFA_MFCC_GENERIC", None)
    if name == "generic":
        os.environ["MFA_MFCC_GENERIC"] = "1"
    try:
        path = eng.mfcc_path() if hasattr(eng.lib, "mfa_mfcc_path") else "the build's only kernel"
        return eng.mfcc(pcm, so), path
    finally:
        os.environ.pop("MFA_MFCC_GENERIC", None)


paths, bits = {}, {}
for v in variants:
    for _ in range(args.warmup):
        (m, fo), paths[v] = run(v)
    bits[v] = m
torch.cuda.synchronize()
same = bool(torch.equal(bits["specialised"].view(torch.int32), bits["generic"].view(torch.int32)))
frames = int(fo[-1])
del bits, m
eng.kernel_timing(True)
times = {v: [] for v in variants}
for _ in range(args.rounds):
    for v in variants:
        eng.reset_kernel_times()
        out = run(v)
        torch.cuda.synchronize()
        k = eng.kernel_times()["mfcc"]
        assert k["launches"] == 1
        times[v].append(k["ms"])
        del out
eng.kernel_timing(False)
rep = {"library": os.environ.get("MFA_HIP_SO") or "default", "utterances": args.utts, "frames": frames, "launches_per_variant": args.rounds,
       "paths": paths, "outputs_bit_identical": same, "ms_per_launch": {}}
for v in variants:
    a = np.asarray(times[v])
    rep["ms_per_launch"][v] = {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4),
                               "max": round(float(a.max()), 4), "Mframes_per_s": round(frames / np.median(a) / 1e3, 1)}
    print(f"{v:12s} ({paths[v]}) median {np.median(a):8.4f} ms  (min {a.min():.4f}, max {a.max():.4f})  {frames / np.median(a) / 1e3:9.1f} Mframes/s",
          flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
assert same, "the two paths disagree"
