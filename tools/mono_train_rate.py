"""Flat-start monophone training time per iteration at the benchmark's batch shape: 8 192 synthetic utterances × 10 s in one
device batch (``--pool`` distinct utterances, each a speaker of its own, tiled over the batch with keys of their own).
``MonophoneTrainer`` runs ``--iterations`` iterations on its device backend; reported per iteration: the wall time of the
three backend calls (equal alignment, alignment, statistics — features, graph compilation, packing and copies included)
and of the host update (transition update, mle_update, mix-up), and beside them the library's event pairs
(mfa_kernel_timing): the equal-alignment kernel (slot 12), scoring + decoder (slots 3, 4: the alignment step the benchmark
measures), the GMM statistics (slots 8 – 11).  GPU.
  python tools/mono_train_rate.py [--utts 8192] [--seconds 10] [--pool 64] [--iterations 4] [--max-gaussians 1000]
                                  [--commit ID] [--out profiles/mono_train_rate.json | --out '']"""
import argparse
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

import synth_workload as S
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusUtterance
from montreal_forced_aligner_amd.engine import KERNEL_SLOTS, AlignmentEngine
from montreal_forced_aligner_amd.train import MonophoneTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=8192)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--pool", type=int, default=64, help="distinct synthetic utterances, tiled over the batch")
ap.add_argument("--iterations", type=int, default=4)
ap.add_argument("--max-gaussians", type=int, default=1000)
ap.add_argument("--commit", default="", help="recorded in the report; default: git rev-parse --short HEAD")
ap.add_argument("--out", default="profiles/mono_train_rate.json", help="report file; '' writes none")
args = ap.parse_args()

commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"

world = S.SynthWorld.build()
samples = int(args.seconds * S.SR)
pool = [world.utterance(3_000_000 + i, n_words=max(1, int(3 * args.seconds)), samples=samples) for i in range(min(args.pool, args.utts))]
utts = [CorpusUtterance(f"utt{i:05d}", f"spk{i:05d}", pool[i % len(pool)][0], pool[i % len(pool)][1]) for i in range(args.utts)]
pt = world.lexicon.phone_table
sil = [pt.find("sil"), pt.find("spn")]
topo = S._topology(max(k for k, s in pt if s != "<eps>"), sil)

eng = AlignmentEngine(0)
frames = int(eng.num_frames_array(np.full(args.utts, samples)).sum())
opt = AlignOptions(boost_silence=1.25, batch_frames=frames + 1)          # one batch, as the benchmark's step
tr = MonophoneTrainer(utts, world.lexicon, topo, num_iterations=args.iterations, max_gaussians=args.max_gaussians,
                      align_options=opt, silence_phones=sil, engine=eng)
rows, cur = [], {}


def timed(name, fn):
    def run(*a, **kw):
        torch.cuda.synchronize()
        eng.reset_kernel_times()
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize()
        cur[name + "_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        for slot in {"equal_align": ("equal_align",), "align": ("gmm", "viterbi"),
                     "accumulate": ("acc_lookup", "acc_sort", "acc_sums", "acc_reduce")}[name]:
            cur[slot + "_kernel_ms"] = round(eng._kernel_time(KERNEL_SLOTS.index(slot))["ms"], 4)
        return out
    return run


b = tr.backend
b.equal_align, b.align, b.accumulate = timed("equal_align", b.equal_align), timed("align", b.align), timed("accumulate", b.accumulate)
update = tr._update


def timed_update(*a, **kw):
    t0 = time.perf_counter()
    update(*a, **kw)
    cur["host_update_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rows.append(dict(tr.history[-1], **cur))
    cur.clear()


tr._update = timed_update
eng.kernel_timing(True)
tr.train()
eng.kernel_timing(False)

rep = {"commit": commit, "utterances": args.utts, "seconds_per_utterance": args.seconds, "distinct_utterances": len(pool),
       "frames": frames, "pdfs": tr.raw_am.num_pdfs, "max_gaussians": args.max_gaussians, "iterations": rows}
for r in rows:
    print(" ".join(f"{k}={v}" for k, v in r.items() if k.endswith("_ms") or k in ("iteration", "gaussians", "failed", "loglike")), flush=True)
print(json.dumps(rep))
if args.out:
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
eng.close()
