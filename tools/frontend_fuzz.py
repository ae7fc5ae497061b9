"""Randomised check of the front end against the oracle: MFCC (random utterance lengths around every framing boundary, odd
sample offsets inside the batch buffer, silence, DC offsets, clipping, both snip_edges settings), per-speaker CMVN, the
delta, delta+fMLLR and splice+LDA+fMLLR feature kernels.  GPU.  python tools/frontend_fuzz.py [n_seeds] [first_seed]"""
import sys
sys.path.insert(0, ".")
import numpy as np
import torch
import synth_workload as synth
from montreal_forced_aligner_amd.engine import AlignmentEngine
from oracle import oracle as O
from tests import helpers
from tests.delta_fmllr_helpers import seeded_delta_fmllr

n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
eng = AlignmentEngine(0)
lda = synth.seeded_lda()
fm = synth.seeded_fmllr(16)
fm_delta = seeded_delta_fmllr(16)                                  # 39×40: the transforms of the Δ+ΔΔ path
bad = 0
for seed in range(seed0, seed0 + n_seeds):
    case = helpers.frontend_fuzz_case(seed)
    snip, segs, kinds, n = case["snip_edges"], case["segs"], case["kinds"], len(case["segs"])
    eng.configure_mfcc(snip_edges=snip)
    opts = O.default_mfcc_opts(snip_edges=snip)
    so = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    pcm = torch.from_numpy(np.concatenate(segs)).to(eng.device)
    out, fo = eng.mfcc(pcm, so)
    out = out.cpu().numpy()
    refs = [O.mfcc(s.astype(np.float32), opts) for s in segs]
    worst = 0.0
    try:
        for u, ref in enumerate(refs):
            got = out[fo[u]: fo[u + 1]]
            assert got.shape == ref.shape, (u, len(segs[u]), got.shape, ref.shape)
            if ref.size:
                d = float(np.abs(got - ref).max())
                worst = max(worst, d)
                if d >= 1e-2:   # (speech-like signals agree to 1e-3; a strong tone over a weak floor leaves bins at the FFT's own rounding noise: ≤ 7e-3 seen)
                    fr, cf = np.unravel_index(np.argmax(np.abs(got - ref)), ref.shape)
                    raise AssertionError(f"utterance {u} ({kinds[u]}, {len(segs[u])} samples, std {segs[u].astype(np.float64).std():.1f}): |d| {d:.4f} at frame {fr} coefficient {cf}: device {got[fr, cf]:.4f} oracle {ref[fr, cf]:.4f}")
        # CMVN over random speaker groups + both feature kernels, from the DEVICE's MFCCs on both sides
        n_spk, rows = case["n_spk"], case["rows"]
        stats = eng.cmvn_stats(torch.from_numpy(out).to(eng.device), fo, rows, n_spk)
        st = stats.cpu().numpy()
        mf = [out[fo[u]: fo[u + 1]] for u in range(n)]
        for s_ in range(n_spk):
            mine = [mf[u] for u in range(n) if rows[u] == s_ and mf[u].shape[0] > 0]
            if mine:
                ref_st = O.cmvn_stats(mine)
                assert np.allclose(st[s_], ref_st, rtol=1e-12, atol=1e-9), ("cmvn", s_)
        d_mfcc = torch.from_numpy(out).to(eng.device)
        f_delta = eng.features(d_mfcc, fo, rows, stats).cpu().numpy()
        f_dfm = eng.features(d_mfcc, fo, rows, stats, fmllr=torch.from_numpy(fm_delta[:n_spk]).to(eng.device)).cpu().numpy()
        spk_fm = torch.from_numpy(fm[:n_spk]).to(eng.device)       # one transform per speaker row
        f_lda = eng.features(d_mfcc, fo, rows, stats, lda=torch.from_numpy(lda).to(eng.device), fmllr=spk_fm).cpu().numpy()
        wd = wf = wl = 0.0
        for u in range(n):
            if mf[u].shape[0] == 0:
                continue
            base = O.cmvn_apply(st[rows[u]], mf[u])
            rd = O.deltas(base)
            rl = O.affine(O.affine(O.splice(base), lda), fm[rows[u]])
            wd = max(wd, float(np.abs(f_delta[fo[u]: fo[u + 1]] - rd).max()))
            wf = max(wf, float(np.abs(f_dfm[fo[u]: fo[u + 1]] - O.affine(rd, fm_delta[rows[u]])).max()))
            wl = max(wl, float(np.abs(f_lda[fo[u]: fo[u + 1]] - rl).max()))
        assert wd < 1e-3 and wf < 1e-3 and wl < 1e-3, ("features", wd, wf, wl)
        print(seed, f"snip_edges {snip}, {n} utterances, mfcc worst {worst:.2e}, deltas {wd:.1e}, deltas+fmllr {wf:.1e}, lda+fmllr {wl:.1e}", flush=True)
    except AssertionError as e:
        bad += 1
        print(seed, "MISMATCH", str(e)[:300], flush=True)
print("mismatches:", bad)
sys.exit(1 if bad else 0)
