"""GPU tests of the N4 rows: boundary fine-tuning at 1 ms and phone confidence, on the reference's own
plumbing fixture.  Both are re-uses of the hot-path kernels, so the checks are (a) the host arithmetic against a direct
restatement of the reference's formulas and (b) the device results against the oracle run on the same windows."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu


def _first_pass(fx, KA, tmp_path, seconds=4.2):
    import torch

    from montreal_forced_aligner_amd import kaldi_io as K

    ar = K.load_acoustic_model_archive(helpers.REF / "mono_model.zip")
    (tmp_path / "final.mdl").write_bytes(ar["final.mdl"])
    (tmp_path / "tree").write_bytes(ar["tree"])
    pcm = fx.pcm[: int(16000 * seconds)]
    text = "this is the acoustic corpus i'm talking pretty fast here"
    aligner = KA.GmmAligner(tmp_path / "final.mdl", beam=100, retry_beam=400, transition_scale=1.0, acoustic_scale=0.1,
                            self_loop_scale=0.1)
    eng = aligner._engine()
    eng.configure_mfcc()
    so = np.array([0, len(pcm)], dtype=np.int64)
    mfcc, frame_off = eng.mfcc(torch.from_numpy(pcm.astype(np.int16)).to(eng.device), so)
    cmvn = eng.cmvn_stats(mfcc, frame_off, np.zeros(1, np.int32), 1)
    feats = eng.features(mfcc, frame_off, np.zeros(1, np.int32), cmvn)
    al = aligner.align_utterance(fx.mono_gc.compile_fst(text), feats.cpu().numpy())
    assert al is not None
    ivs = al.generate_ctm(aligner.transition_model, fx.mono_lex.phone_table, 0.01)
    return aligner, eng, pcm, cmvn, feats, frame_off, ivs


def test_fine_tune_boundaries_matches_oracle_windows(fx, tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from montreal_forced_aligner_amd import finetune as FT
    from montreal_forced_aligner_amd import graph as G
    from montreal_forced_aligner_amd import kalpy_api as KA

    aligner, eng, pcm, cmvn, feats, frame_off, ivs = _first_pass(fx, KA, tmp_path)
    tm = aligner.transition_model
    new_ivs, deleted = FT.fine_tune_boundaries(aligner, fx.mono_gc, [pcm], [ivs], utt2spk=[0], cmvn=cmvn)
    new_ivs, deleted = new_ivs[0], deleted[0]
    assert len(new_ivs) + len(deleted) == len(ivs)
    # contiguous, ordered, first begin and last end untouched
    assert new_ivs[0].begin == ivs[0].begin and new_ivs[-1].end == ivs[-1].end
    assert all(a.end == b.begin for a, b in zip(new_ivs[:-1], new_ivs[1:]))
    assert all(iv.begin < iv.end for iv in new_ivs)
    kept = [i for i in range(len(ivs)) if i not in deleted]
    moved = 0
    for iv, i in zip(new_ivs, kept):
        # a boundary can only move inside its ±15 ms decoding window (plus the 1 ms grid)
        assert abs(iv.begin - ivs[i].begin) <= 0.0151, (i, iv.begin, ivs[i].begin)
        moved += iv.begin != ivs[i].begin
    assert moved > len(ivs) // 2   # 1 ms resolution: most boundaries leave the 10 ms grid
    # ---- the same windows through the oracle (1 ms MFCC → speaker CMVN → deltas → rows → two-phone Viterbi)
    stats = cmvn.cpu().numpy()[0]
    windows = FT.plan_windows([ivs], [len(pcm) / 16000.0], 0.01)
    opts = O.default_mfcc_opts(frame_shift_ms=1.0)
    checked = 0
    for w in windows[:: max(1, len(windows) // 12)]:
        a, b = int(round(w.feature_begin * 16000)), int(round(w.feature_end * 16000))
        mf = O.mfcc(pcm[a:b].astype(np.float32), opts)
        x = O.deltas(O.cmvn_apply(stats, mf))
        r0 = min(int(round(w.begin_offset * 1000)), x.shape[0])
        r1 = min(max(int(round(w.end_offset * 1000)), r0), x.shape[0])
        x = x[r0:r1]
        if x.shape[0] == 0:
            continue
        fst = G.add_transition_probs(FT.two_phone_graph(fx.mono_gc, [w.prev_phone], [w.phone]), aligner._scaled)
        pl = np.unique(tm.id2pdf[fst.arcs["ilabel"]])
        am = aligner.acoustic_model
        ll = O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl)
        ref = helpers.oracle_align(tm, fst, ll, pl, acoustic_scale=1.0, beam=100.0, retry_beam=400.0)
        if ref["status"] not in (0, 1):
            continue
        from montreal_forced_aligner_amd import ctm as C
        ctm = C.generate_ctm(ref["ali"], tm, None, 0.001)
        want = round(ctm[1].begin + w.feature_begin + w.begin_offset, 4)
        # before the repair loop the boundary is exactly the oracle's; the loop only touches it when an interval vanishes
        if w.index in kept and not deleted:
            got = new_ivs[kept.index(w.index)].begin
            assert abs(got - want) <= 0.0011, (w.index, got, want)   # 1 ms grid; device MFCC vs oracle MFCC differ by ~1e-4
            checked += 1
    assert checked >= 5          # (nothing is deleted here, on the device as on the oracle: every sampled window was compared)


def test_repair_intervals_restates_reference_loop():
    from montreal_forced_aligner_amd import finetune as FT

    m = [dict(id=0, begin=0.0, end=0.1), dict(id=1, begin=0.12, end=0.2), dict(id=2, begin=0.2, end=0.2),
         dict(id=3, begin=0.2, end=0.3)]
    out, deleted = FT.repair_intervals([dict(x) for x in m])
    assert deleted == [2]
    assert [(x["id"], x["begin"], x["end"]) for x in out] == [(0, 0.0, 0.12), (1, 0.12, 0.2), (3, 0.2, 0.3)]


def test_phone_confidence_matches_numpy_restatement(fx, tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from montreal_forced_aligner_amd import finetune as FT
    from montreal_forced_aligner_amd import kalpy_api as KA

    aligner, eng, pcm, cmvn, feats, frame_off, ivs = _first_pass(fx, KA, tmp_path, seconds=3.0)
    tm, am = aligner.transition_model, aligner.acoustic_model
    strip = lambda s: s.rsplit("_", 1)[0] if s[-2:] in ("_B", "_E", "_I", "_S") else s
    # phone → pdf counts as MFA's phone_pdf_counts.json holds them: here from the transition model's own (phone, pdf) pairs
    counts = {}
    for tid in range(1, tm.num_transition_ids + 1):
        ph = fx.mono_lex.phone_table.find(int(tm.id2phone[tid]))
        counts.setdefault(ph, {}).setdefault(str(int(tm.id2pdf[tid])), 0)
        counts[ph][str(int(tm.id2pdf[tid]))] += 1 + (tid % 3)
    got = FT.phone_confidence(eng, feats, frame_off, counts, [ivs], strip_position=strip, silence_label="sil")[0]
    # numpy restatement of PhoneConfidenceFunction._run on oracle scores
    x = feats.cpu().numpy()
    likes = O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, np.arange(am.num_pdfs))
    names, table = FT.phone_pdf_weights(counts, strip)
    phone_likes = np.stack([likes[:, table[p][0]].astype(np.float64) @ table[p][1] for p in names], axis=1)
    top = phone_likes.argmax(1)
    want = []
    for i, iv in enumerate(ivs):
        name = strip(str(iv.label))
        if name == "sil" or name not in names:
            continue
        fb, fe = int((iv.begin * 1000) / 10), int((iv.end * 1000) / 10)
        fe = min(fe + (fb == fe), x.shape[0])
        sc = [0.0 if names[top[t]] == name else phone_likes[t, top[t]] - phone_likes[t, names.index(name)] for t in range(fb, fe)]
        if sc:
            want.append((i, float(np.mean(sc))))
    assert [i for i, _ in got] == [i for i, _ in want] and len(got) > 5
    assert np.allclose([g for _, g in got], [w for _, w in want], atol=2e-3)
