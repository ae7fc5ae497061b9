"""Speech-activity time per call on resident inputs, at the two shapes the stage meets: many short utterances (the
benchmark's batch of 10 s utterances: feature archives) and a handful of long recordings (four of one hour: segmenting).  Per
round and shape, in this order: the energy VAD, sliding-window CMVN (cmn_window 300, centred), voiced-frame selection with
subsampling 2 (count + gather), the voiced runs, the MFCC launch on the same batch, and a device-to-device copy of the MFCC
matrix (the same bytes streamed once in and once out: the floor to judge the four against — the VAD and the runs read one
column and write a vector, the CMVN and the selection read and write the matrix).  The four stages and the MFCC are timed by
the library's event pairs (mfa_kernel_timing, slots 24 and 0; a stage's launches are summed), the copy by an event pair of its
own; every variant is warmed up and the figures are medians over ``--rounds``.  The input is a tone under noise whose level
steps up and down, so that the VAD has runs to find.  GPU.
  python tools/vad_rate.py [--utts 1024] [--seconds 10] [--long 4] [--long-seconds 3600] [--rounds 7] [--commit ID]
                           [--out profiles/vad_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=1024)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--long", type=int, default=4)
ap.add_argument("--long-seconds", type=float, default=3600.0)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--commit", default="", help="recorded in the report; default: git rev-parse --short HEAD")
ap.add_argument("--out", default="profiles/vad_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

eng = AlignmentEngine(0)
eng.configure_mfcc(use_energy=1, raw_energy=0)
rate = eng.model_rate()
med = lambda v: float(np.median(v))      # noqa: E731


def signal(n_utt, n_in):
    """int16 [n_utt · n_in]: a tone under noise, loud and quiet in turns of 0.7 s (an input, not the product)."""
    gen = torch.Generator(device=eng.device).manual_seed(1)
    out = torch.empty(n_utt * n_in, dtype=torch.int16, device=eng.device)
    t = torch.arange(n_in, device=eng.device, dtype=torch.float32) / rate
    level = 0.02 + 0.98 * (torch.floor(t / 0.7) % 2)
    tone = 4000.0 * torch.sin(2 * np.pi * 130.0 * t)
    for k in range(n_utt):
        out[k * n_in: (k + 1) * n_in] = (level * (tone + 1500.0 * torch.randn(n_in, device=eng.device, generator=gen))).to(torch.int16)
    return out


def measure(name, n_utt, seconds):
    n_in = int(seconds * rate)
    pcm = signal(n_utt, n_in)
    so = np.arange(n_utt + 1, dtype=np.int64) * n_in
    mfcc, fo = eng.mfcc(pcm, so)
    vad = eng.vad(mfcc, fo, energy_threshold=0.0, energy_mean_scale=1.0)[0]
    copy_dst = torch.empty_like(mfcc)
    stages = {"vad": lambda: eng.vad(mfcc, fo, energy_threshold=0.0, energy_mean_scale=1.0),
              "sliding_cmvn": lambda: eng.sliding_cmvn(mfcc, fo, cmn_window=300, center=1),
              "select_frames": lambda: eng.select_frames(mfcc, fo, vad, 2),
              "vad_runs": lambda: eng.vad_runs(vad, fo)}
    for _ in range(args.warmup):
        for f in stages.values():
            f()
        eng.mfcc(pcm, so, fo)
        copy_dst.copy_(mfcc)
    torch.cuda.synchronize()
    eng.kernel_timing(True)
    times = {k: [] for k in list(stages) + ["mfcc", "copy_in_out"]}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for k, f in stages.items():
            eng.reset_kernel_times()
            f()
            torch.cuda.synchronize()
            times[k].append(eng.kernel_time("vad")["ms"])
        eng.reset_kernel_times()
        eng.mfcc(pcm, so, fo)
        e0.record(torch.cuda.current_stream(eng.device))
        copy_dst.copy_(mfcc)
        e1.record(torch.cuda.current_stream(eng.device))
        torch.cuda.synchronize()
        times["mfcc"].append(eng.kernel_times()["mfcc"]["ms"])
        times["copy_in_out"].append(e0.elapsed_time(e1))
    eng.kernel_timing(False)
    _b, _e, run_off = eng.vad_runs(vad, fo)
    rep = {"shape": name, "utterances": n_utt, "seconds_per_utterance": seconds, "frames": int(fo[-1]), "columns": int(mfcc.shape[1]),
           "matrix_bytes": int(mfcc.numel() * 4), "voiced_share": round(float(vad.mean()), 4), "runs": int(run_off[-1])}
    rep.update({k + "_ms": round(med(v), 4) for k, v in times.items()})
    print(f"{name}: {n_utt} x {seconds:g} s, {rep['frames']} x {rep['columns']}: " +
          ", ".join(f"{k} {rep[k + '_ms']:.4f} ms" for k in times), flush=True)
    del pcm, mfcc, vad, copy_dst
    torch.cuda.empty_cache()
    return rep


report = {"commit": commit, "rounds": args.rounds,
          "shapes": [measure("short utterances", args.utts, args.seconds), measure("long recordings", args.long, args.long_seconds)]}
print(json.dumps(report))
if args.out:
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
eng.close()
