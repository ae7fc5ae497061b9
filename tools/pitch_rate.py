"""Pitch time per call on resident inputs, beside the MFCC launch on the same batch: 1 024 utterances × 10 s at the model's
rate.  The tracker (mfa_pitch_batch: down-sampling + the per-utterance NCCF / Viterbi workgroups, in as many sub-launches as
the workspace budget asks for) and ProcessPitch (mfa_pitch_process_batch) are timed together by the library's event pairs
(mfa_kernel_timing, slot 6), the MFCC by slot 0.  Each is warmed up, then run ``--rounds`` times; the figure is the median.
The input is band-limited noise around a tone: the tracker's work does not depend on the signal.  GPU.
  python tools/pitch_rate.py [--utts 1024] [--seconds 10] [--rounds 5] [--out profiles/pitch_rate.json | --out '']"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=1024)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--max-f0", type=float, default=800.0)
ap.add_argument("--out", default="profiles/pitch_rate.json", help="report file; '' writes none")
args = ap.parse_args()

eng = AlignmentEngine(0)
eng.configure_mfcc(snip_edges=1)
eng.configure_pitch(max_f0=args.max_f0)
rate = eng.model_rate()
n_in = int(args.seconds * rate)
gen = torch.Generator(device=eng.device).manual_seed(1)
t = torch.arange(n_in, device=eng.device, dtype=torch.float32) / rate
tone = 4000.0 * torch.sin(2 * np.pi * 130.0 * t)
pcm = (tone[None, :] + 1500.0 * torch.randn((args.utts, n_in), device=eng.device, generator=gen)).to(torch.int16).reshape(-1)   # (an input, not the product)
so = np.arange(args.utts + 1, dtype=np.int64) * n_in
fo = eng.pitch_frame_offsets(so)
for _ in range(args.warmup):
    eng.pitch(pcm, so, fo)
    eng.mfcc(pcm, so)
torch.cuda.synchronize()
eng.kernel_timing(True)
t_pitch, t_mfcc, launches = [], [], 0
for _ in range(args.rounds):
    eng.reset_kernel_times()
    out = eng.pitch(pcm, so, fo)
    mf, _fo = eng.mfcc(pcm, so)
    torch.cuda.synchronize()
    a, b = eng.pitch_time(), eng.kernel_times()["mfcc"]
    t_pitch.append(a["ms"]); t_mfcc.append(b["ms"]); launches = a["launches"]
    del mf
eng.kernel_timing(False)
rep = {"utterances": args.utts, "seconds_per_utterance": args.seconds, "frames": int(fo[-1]), "states": int(eng.lib.mfa_pitch_num_states(eng.ctx)),
       "rounds": args.rounds, "timed_launch_groups_per_call": launches, "workspace_bytes": eng.pitch_workspace_bytes(so, fo),
       "pitch_ms": round(float(np.median(t_pitch)), 3), "pitch_ms_min": round(float(np.min(t_pitch)), 3),
       "mfcc_ms": round(float(np.median(t_mfcc)), 4),
       "audio_seconds_per_s": round(args.utts * args.seconds / np.median(t_pitch) * 1e3, 0)}
print(f"{args.utts} x {args.seconds:g} s, {rep['states']} states: pitch {rep['pitch_ms']:.3f} ms per call (min {rep['pitch_ms_min']:.3f}), "
      f"MFCC of the same batch {rep['mfcc_ms']:.4f} ms", flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
