"""Resampler time per launch on resident inputs, beside the MFCC launch it feeds: 8 192 utterances × 10 s at 44.1 kHz and at
8 kHz → the model's rate, then the MFCC of the converted batch in the same run.  Each is warmed up, then launched
``--rounds`` times; the figure is the median, timed by the library's event pair (mfa_kernel_timing).  The streaming floor
is (input bytes + output bytes) ÷ ``--hbm-tbs`` (HBM bandwidth, TB/s).  GPU.
  python tools/resample_rate.py [--utts 8192] [--seconds 10] [--rounds 10] [--out profiles/resample_rate.json | --out '']"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from montreal_forced_aligner_amd.engine import AlignmentEngine

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--rates", default="44100,8000")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--hbm-tbs", type=float, default=8.0)
ap.add_argument("--out", default="profiles/resample_rate.json", help="report file; '' writes none")
args = ap.parse_args()

eng = AlignmentEngine(0)
eng.configure_mfcc()
target = eng.model_rate()
rep = {"utterances": args.utts, "seconds_per_utterance": args.seconds, "model_rate_hz": target, "launches": args.rounds,
       "hbm_tbs": args.hbm_tbs, "rates": {}}
for rate in [int(r) for r in args.rates.split(",")]:
    n_in = int(args.seconds * rate)
    gen = torch.Generator(device=eng.device).manual_seed(rate)
    pcm = torch.randint(-8000, 8000, (args.utts * n_in,), dtype=torch.int16, device=eng.device, generator=gen)   # (an input, not the product)
    so = np.arange(args.utts + 1, dtype=np.int64) * n_in
    rates = [rate] * args.utts
    for _ in range(args.warmup):
        out, oo = eng.resample(pcm, so, rates)
        eng.mfcc(out, oo)
    torch.cuda.synchronize()
    eng.kernel_timing(True)
    t_rs, t_mfcc = [], []
    for _ in range(args.rounds):
        eng.reset_kernel_times()
        out, oo = eng.resample(pcm, so, rates)
        mf, _fo = eng.mfcc(out, oo)
        torch.cuda.synchronize()
        a, b = eng.resample_time(), eng.kernel_times()["mfcc"]
        assert a["launches"] == 1 and b["launches"] == 1
        t_rs.append(a["ms"]); t_mfcc.append(b["ms"])
        del mf
    eng.kernel_timing(False)
    moved = 2 * (int(so[-1]) + int(oo[-1]))
    floor_ms = moved / (args.hbm_tbs * 1e12) * 1e3
    r = {"resample_ms": round(float(np.median(t_rs)), 4), "resample_ms_min": round(float(np.min(t_rs)), 4),
         "mfcc_ms": round(float(np.median(t_mfcc)), 4), "streaming_floor_ms": round(floor_ms, 4), "bytes_moved": moved,
         "audio_seconds_per_s": round(args.utts * args.seconds / np.median(t_rs) * 1e3, 0)}
    rep["rates"][str(rate)] = r
    print(f"{rate:6d} Hz -> {target} Hz: resample {r['resample_ms']:.4f} ms (min {r['resample_ms_min']:.4f}), MFCC of the result "
          f"{r['mfcc_ms']:.4f} ms, streaming floor {floor_ms:.4f} ms", flush=True)
    del pcm, out
    torch.cuda.empty_cache()
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
