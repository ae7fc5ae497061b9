"""Feature-kernel time per launch on resident inputs: 8 192 utterances × 1 000 frames of 13 cepstra, 64 speakers.
  delta             CMVN → Δ+ΔΔ                                   (the floor: no transform)
  delta_fmllr       CMVN → Δ+ΔΔ → fMLLR, in feats_kernel
  lda_fmllr_gen     CMVN → splice ±3 → LDA → fMLLR, generic kernel (MFA_FEATS_GENERIC=1)
  lda_fmllr_reg     CMVN → splice ±3 → LDA → fMLLR, frame-per-lane kernel (the yardstick)
Every variant is warmed up, then the variants are launched in turn, ``--rounds`` times; the figure is the median of a
variant's launches, timed by the library's event pair (mfa_kernel_timing / mfa_kernel_time_ms, which = 2).  GPU.
  python tools/feats_rate.py [--rounds 20] [--only delta] [--out profiles/feats_rate.json | --out '']
``--only delta`` with MFA_HIP_SO=<another build> times the floor of that build (A/B against an older library)."""
import argparse
import json
import os
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

import synth_workload as synth
from montreal_forced_aligner_amd.engine import AlignmentEngine

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--speakers", type=int, default=64)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default="")
ap.add_argument("--out", default="profiles/feats_rate.json", help="report file; '' writes none")
args = ap.parse_args()

eng = AlignmentEngine(0)
dev = eng.device
dim = 13
gen = torch.Generator(device="cpu").manual_seed(1)
mfcc = (10.0 * torch.randn((args.utts * args.frames, dim), generator=gen)).to(dev)
fo = (np.arange(args.utts + 1, dtype=np.int64) * args.frames)
u2s = (np.arange(args.utts) % args.speakers).astype(np.int32)
cmvn = eng.cmvn_stats(mfcc, fo, u2s, args.speakers)
rng = np.random.default_rng(2)
w39 = np.eye(39, 40)[None] + 0.05 * rng.normal(size=(args.speakers, 39, 40))
d_w39 = torch.from_numpy(w39.astype(np.float32)).to(dev)
d_lda = torch.from_numpy(synth.seeded_lda()).to(dev)
d_w40 = torch.from_numpy(synth.seeded_fmllr(args.speakers)).to(dev)


def run(name):
    os.environ.pop("MFA_FEATS_GENERIC", None)
    if name == "delta":
        return eng.features(mfcc, fo, u2s, cmvn)
    if name == "delta_fmllr":
        return eng.features(mfcc, fo, u2s, cmvn, fmllr=d_w39)
    if name == "lda_fmllr_gen":
        os.environ["MFA_FEATS_GENERIC"] = "1"
        try:
            return eng.features(mfcc, fo, u2s, cmvn, lda=d_lda, fmllr=d_w40)
        finally:
            os.environ.pop("MFA_FEATS_GENERIC", None)
    return eng.features(mfcc, fo, u2s, cmvn, lda=d_lda, fmllr=d_w40)


variants = ["delta", "delta_fmllr", "lda_fmllr_gen", "lda_fmllr_reg"]
if args.only:
    variants = [v for v in variants if v in args.only.split(",")]
for v in variants:
    for _ in range(args.warmup):
        run(v)
torch.cuda.synchronize()
eng.kernel_timing(True)
times = {v: [] for v in variants}
for _ in range(args.rounds):
    for v in variants:
        eng.reset_kernel_times()
        out = run(v)
        torch.cuda.synchronize()
        t = eng.kernel_times()["feats"]
        assert t["launches"] == 1
        times[v].append(t["ms"])
        del out
eng.kernel_timing(False)
frames = args.utts * args.frames
rep = {"library": os.environ.get("MFA_HIP_SO") or "default", "utterances": args.utts, "frames_per_utterance": args.frames,
       "speakers": args.speakers, "launches_per_variant": args.rounds, "ms_per_launch": {}}
for v in variants:
    a = np.asarray(times[v])
    rep["ms_per_launch"][v] = {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4),
                               "max": round(float(a.max()), 4), "Mframes_per_s": round(frames / np.median(a) / 1e3, 1)}
    print(f"{v:16s} median {np.median(a):8.4f} ms  (min {a.min():.4f}, max {a.max():.4f})  {frames / np.median(a) / 1e3:9.1f} Mframes/s",
          flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
