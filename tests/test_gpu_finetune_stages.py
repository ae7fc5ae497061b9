"""Boundary fine-tuning stage by stage: every stage of ``finetune.fine_tune_boundaries`` (its ``trace``) against the oracle
applied to the PREVIOUS device stage's output, with the bars the project already holds each kernel to — so that a stage
that is off cannot hide behind the 1 ms grid or the ±15 ms window.  Inputs: tests/finetune_ref.py (tests/test_finetune_cpu.py
proves without a GPU that they reach the 0.1 fallback, failures at both scales, phones unseen in the utterance, deletions,
snip_edges truncation, windows of too few and of no rows, two speakers).  Also here: chunking, batch invariance, the phone
table, the engine's MFCC options after the call, the feature-width refusals, and phone confidence on a mixture model."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import finetune_ref as R
from tests import gmm_ref
from tests import helpers
from tests.test_gpu_frontend_options import SPEECH_BAR

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _default_mfcc_options_afterwards():
    """These tests leave the process's engine at the options they passed (that is what they check): put the defaults back."""
    yield
    import torch
    if torch.cuda.is_available():
        from montreal_forced_aligner_amd import kalpy_api as KA
        KA.get_engine().configure_mfcc()


# ---- the device side ----------------------------------------------------------------------------------------------------

def _aligner(model_bytes, beam, retry_beam):
    from montreal_forced_aligner_amd import kalpy_api as KA
    return KA.GmmAligner(model_bytes, beam=beam, retry_beam=retry_beam, transition_scale=1.0, acoustic_scale=0.1,
                         self_loop_scale=0.1)


def _mono_model(fx):
    from montreal_forced_aligner_amd import kaldi_io as K
    return K.load_acoustic_model_archive(helpers.REF / "mono_model.zip")["final.mdl"]


def _mono_case(fx, name):
    """Everything a run and its checks need, for a configuration of the mono batch (or the hand-made one)."""
    if name == "hand":
        batch, cfg = R.hand_batch(fx), dict(group=lambda p: (p,), beam=100.0, retry_beam=400.0)
        cfg["intervals"] = batch.intervals
    else:
        batch, cfg = R.mono_batch(fx), R.mono_config(fx, name)
    return dict(batch=batch, intervals=cfg["intervals"], group=cfg["group"], beam=cfg["beam"], retry_beam=cfg["retry_beam"],
                model=_mono_model(fx), compiler=fx.mono_gc, tm=fx.mono_tm, am=fx.mono_am, lda=None, fmllr=None,
                phone_table=fx.mono_lex.phone_table)


def _lda_case(fx):
    s = R.lda_setup(fx)
    return dict(batch=s.batch, intervals=s.batch.intervals, group=s.group, beam=100.0, retry_beam=400.0,
                model=fx.g2p_archive["final.mdl"], compiler=s.compiler, tm=s.tm, am=s.am, lda=s.lda, fmllr=s.fmllr,
                phone_table=s.lex.phone_table)


def _run(case, snip_edges, utts=None, trace=None, **kw):
    """fine_tune_boundaries on the case (``utts``: a subset of its utterances)."""
    torch = _torch()
    from montreal_forced_aligner_amd import finetune as FT
    aligner = _aligner(case["model"], case["beam"], case["retry_beam"])
    eng = aligner._engine()
    b = case["batch"]
    utts = list(range(len(b.pcm))) if utts is None else utts
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)      # noqa: E731
    out = FT.fine_tune_boundaries(
        aligner, case["compiler"], [b.pcm[u] for u in utts], [case["intervals"][u] for u in utts],
        utt2spk=[b.utt2spk[u] for u in utts], cmvn=dev(b.spk_stats, np.float64),
        lda=None if case["lda"] is None else dev(case["lda"], np.float32),
        fmllr=None if case["fmllr"] is None else dev(case["fmllr"], np.float32), phone_group=case["group"],
        mfcc_options=dict(snip_edges=snip_edges), phone_table=case["phone_table"], trace=trace, **kw)
    return aligner, eng, out


def _check_stages(case, snip_edges, aligner, out, trace, max_windows=None):
    """The five stages.  Returns counters for the caller's own conditions."""
    b, intervals, tm, am = case["batch"], case["intervals"], case["tm"], case["am"]
    windows = trace["windows"]
    ref_windows = R.plan(intervals, [len(x) / R.SR for x in b.pcm])
    assert [vars(w) for w in windows] == [vars(w) for w in ref_windows]
    opts = O.default_mfcc_opts(frame_shift_ms=1.0, snip_edges=snip_edges)
    n_gauss = np.diff(am.pdf_offsets)
    mono = bool((n_gauss == 1).all())
    alis, scale_of, n = {}, {}, dict(windows=len(windows), fallback=0, failed=0, truncated=0, empty=0, chunks=len(trace["chunks"]))
    worst = dict(mfcc=0.0, feats=0.0, score=0.0)
    covered = 0
    for ch in trace["chunks"]:
        first, fo, new_off = ch["first"], ch["frame_off"], ch["new_off"]
        chunk = windows[first: first + len(fo) - 1]
        assert len(chunk) == len(fo) - 1 == len(new_off) - 1 and first == covered
        assert max_windows is None or len(chunk) <= max_windows
        covered += len(chunk)
        mfcc, sub = ch["mfcc"].cpu().numpy(), ch["sub"].cpu().numpy()
        assert mfcc.shape == (fo[-1], 13) and sub.shape == (new_off[-1], am.dim)
        for k, w in enumerate(chunk):
            # ---- frames: the cut's frame count and MFCCs
            a, e = R.cut_samples(w)
            cut = b.pcm[w.utt][a:e]
            T = max(O.mfcc_num_frames(len(cut), opts), 0)
            assert int(fo[k + 1] - fo[k]) == T, (first + k, int(fo[k + 1] - fo[k]), T)
            dev_mfcc = mfcc[fo[k]: fo[k + 1]]
            if T:
                worst["mfcc"] = max(worst["mfcc"], float(np.abs(dev_mfcc - O.mfcc(cut.astype(np.float32), opts)).max()))
            # ---- features: the oracle chain on the DEVICE's MFCCs, this window's speaker, this window's rows
            r0, r1, truncated = R.row_range(w, T)
            n["truncated"] += truncated
            n["empty"] += r1 == r0
            assert int(new_off[k + 1] - new_off[k]) == r1 - r0, (first + k, r0, r1)
            if r1 > r0:
                spk = b.utt2spk[w.utt]
                assert int(ch["spk"][k]) == spk
                want = R.feature_chain(dev_mfcc, b.spk_stats[spk], case["lda"], None if case["fmllr"] is None else case["fmllr"][spk])[r0:r1]
                err = float(np.abs(sub[new_off[k]: new_off[k + 1]] - want).max())
                worst["feats"] = max(worst["feats"], err)
                assert err < R.FEATURE_BAR, (first + k, spk, err)
        assert worst["mfcc"] < SPEECH_BAR, worst["mfcc"]
        # ---- scores and decoding, per attempt
        att = ch["attempts"]
        with_rows = [first + k for k in range(len(chunk)) if new_off[k + 1] > new_off[k]]
        assert len(att) <= 2 and (not with_rows) == (not att)
        for j, at in enumerate(att):
            assert at["scale"] == (1.0, 0.1)[j]
            sel, afo, ll, ll_off = at["windows"], at["frame_off"], at["ll"].cpu().numpy(), at["ll_off"]
            if j == 0:
                assert sel == with_rows
            else:       # the set decoded again at 0.1 is exactly the set that failed at 1.0
                assert sel == [k for k, st in zip(att[0]["windows"], att[0]["status"]) if st not in (0, 1)]
            x = at["x"].cpu().numpy()
            for i, k in enumerate(sel):
                kk = k - first
                xi = x[afo[i]: afo[i + 1]]
                assert np.array_equal(xi, sub[new_off[kk]: new_off[kk + 1]])
                pl, ff = at["pdf_lists_host"][i], at["pdf_first_frame"][i]
                Tk = xi.shape[0]
                got = ll[ll_off[i]: ll_off[i + 1]].reshape(Tk, len(pl))
                asked = ff[None, :] <= np.arange(Tk)[:, None]          # cells a decoder token can ask for
                orc = O.gmm_loglikes(xi, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl)
                single = n_gauss[pl] == 1
                assert np.array_equal(got[:, single][asked[:, single]], orc[:, single][asked[:, single]]), \
                    f"window {k} at {at['scale']}: single-Gaussian scores differ from the oracle's bits"
                if not mono and (~single).any():
                    ref = gmm_ref.ref64(xi, am, pl)
                    ratio = (np.abs(got.astype(np.float64) - ref) / gmm_ref.bound(xi, am, pl, ref))[:, ~single][asked[:, ~single]]
                    if ratio.size:
                        worst["score"] = max(worst["score"], float(ratio.max()))
                        assert ratio.max() <= 1.0, f"window {k} at {at['scale']}: a mixture score is {ratio.max():.3f} B off"
                # the oracle decoder on the DEVICE's scores
                fst = ch["fsts"][kk]
                want = helpers.oracle_align(tm, fst, got, pl, acoustic_scale=at["scale"], beam=aligner.beam, retry_beam=aligner.retry_beam)
                st = int(at["status"][i])
                assert st == want["status"], (k, at["scale"], st, want["status"])
                if st in (0, 1):
                    ali = at["ali"][afo[i]: afo[i + 1]]
                    assert np.array_equal(ali, want["ali"]), (k, at["scale"])
                    assert k not in alis
                    alis[k], scale_of[k] = ali, at["scale"]
        if len(att) == 2:
            n["fallback"] += int(np.isin(att[1]["status"], (0, 1)).sum())
            n["failed"] += int((~np.isin(att[1]["status"], (0, 1))).sum())
    assert covered == len(windows)
    assert trace["scale"] == [scale_of.get(k) for k in range(len(windows))]
    # ---- assembly
    want_iv, want_del = R.assemble(windows, intervals, alis, tm, case["phone_table"])
    assert R.as_tuples(out[0]) == want_iv and out[1] == want_del
    n["deleted"] = sum(len(d) for d in want_del)
    print(f"snip_edges={snip_edges}: {n}; worst MFCC {worst['mfcc']:.2e}, features {worst['feats']:.2e}, mixture err / B {worst['score']:.3f}")
    return n, alis


# ---- the mono batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("snip_edges", [0, 1])
@pytest.mark.parametrize("name", R.CONFIGS + ("hand",))
def test_stages_mono(fx, name, snip_edges):
    case = _mono_case(fx, name)
    trace = {}
    aligner, eng, out = _run(case, snip_edges, trace=trace)
    n, alis = _check_stages(case, snip_edges, aligner, out, trace)
    assert n["chunks"] == 1
    # the options the caller passed are in force again
    assert eng.mfcc_opts.snip_edges == snip_edges and eng.mfcc_opts.frame_shift_ms == 10.0
    if name == "groups40":
        assert n["fallback"] >= 1 and n["failed"] >= 1
        seen = [{int(iv.symbol) for iv in ivs} for ivs in case["intervals"]]
        unseen = [iv for u, ivs in enumerate(out[0]) for iv in ivs if iv.symbol not in seen[u]]
        assert unseen and all(isinstance(iv.label, str) and iv.label == fx.mono_lex.phone_table.find(iv.symbol) for ivs in out[0] for iv in ivs)
    if name == "identity":
        assert n["fallback"] == n["failed"] == 0
    if name == "squeezed":
        assert n["deleted"] >= 1
    if name == "hand":
        assert n["empty"] >= 1 and n["failed"] >= 1 and out[0][2] == [] and len(out[0][1]) == 1
    if snip_edges:
        assert n["truncated"] >= 1


def test_without_a_phone_table_an_unseen_phone_stays_an_id(fx):
    case = dict(_mono_case(fx, "groups40"), phone_table=None)
    trace = {}
    aligner, eng, out = _run(case, 0, trace=trace)
    _check_stages(case, 0, aligner, out, trace)
    labels = [iv.label for ivs in out[0] for iv in ivs]
    assert any(isinstance(x, int) for x in labels) and any(isinstance(x, str) for x in labels)


def test_chunks_of_seven_windows_change_nothing(fx):
    case = _mono_case(fx, "groups40")
    _a, _e, whole = _run(case, 1)
    trace = {}
    aligner, eng, out = _run(case, 1, trace=trace, max_windows=7)
    n, _ = _check_stages(case, 1, aligner, out, trace, max_windows=7)
    assert n["chunks"] == -(-n["windows"] // 7) and n["fallback"] >= 1
    assert R.as_tuples(out[0]) == R.as_tuples(whole[0]) and out[1] == whole[1]
    with pytest.raises(ValueError, match="max_windows"):
        _run(case, 1, max_windows=65536)


def test_batch_equals_utterances_one_at_a_time(fx):
    case = _mono_case(fx, "groups40")
    _a, _e, whole = _run(case, 0)
    for u in range(3):
        _a, _e, one = _run(case, 0, utts=[u])
        assert R.as_tuples(one[0]) == R.as_tuples(whole[0])[u: u + 1] and one[1] == whole[1][u: u + 1], u


# ---- LDA + fMLLR, mixtures -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("snip_edges", [0, 1])
def test_stages_lda_fmllr_mixture_model(fx, snip_edges):
    case = _lda_case(fx)
    trace = {}
    aligner, eng, out = _run(case, snip_edges, trace=trace)
    n, alis = _check_stages(case, snip_edges, aligner, out, trace)
    assert len(alis) == n["windows"] == 21


# ---- the feature width -----------------------------------------------------------------------------------------------------

def _no_launch(monkeypatch, eng):
    """No scoring or decoding launch can reach the device: whatever gets as far as one fails the test instead."""
    def refuse(*a, **kw):
        raise AssertionError("a launch with features of the wrong width was about to reach the device")
    for name in ("_launch_score", "_launch_align", "_launch_align_features"):
        monkeypatch.setattr(eng, name, refuse)


def test_features_of_another_width_are_refused_on_the_host(fx, monkeypatch):
    torch = _torch()
    from montreal_forced_aligner_amd import _lib
    aligner = _aligner(_mono_model(fx), 10.0, 40.0)
    eng = aligner._engine()
    fst = fx.mono_graph("this is")
    graphs, general = eng.pack_graphs([fst], fx.mono_tm), eng.pack_graphs_general([fst], fx.mono_tm)
    _no_launch(monkeypatch, eng)
    fo = np.array([0, 40], dtype=np.int64)
    for width in (48, 13):
        feats = torch.zeros((40, width), dtype=torch.float32, device=eng.device)
        for call in (lambda: eng.score(feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts),
                     lambda: eng.align_features(graphs, feats, fo), lambda: eng.align_general(general, feats, fo)):
            with pytest.raises(_lib.MfaHipError, match=rf"{width} columns.* 39 dimensions"):
                call()


def test_fine_tuning_a_wider_model_is_refused_and_leaves_the_options(fx, monkeypatch):
    """A use_pitch model has 48 dimensions, the 1 ms features fine-tuning computes 39 (it pastes no pitch)."""
    _torch()
    from montreal_forced_aligner_amd import _lib
    from montreal_forced_aligner_amd import finetune as FT
    case = _mono_case(fx, "identity")
    aligner = _aligner(case["model"], 100.0, 400.0)
    aligner.acoustic_model = helpers.random_gmm(np.random.default_rng(48), 48, [1] * fx.mono_tm.num_pdfs)
    eng = aligner._engine()
    assert eng.gmm.dim == 48
    _no_launch(monkeypatch, eng)
    with pytest.raises(_lib.MfaHipError, match=r"39 columns.* 48 dimensions"):
        FT.fine_tune_boundaries(aligner, fx.mono_gc, case["batch"].pcm[:1], case["intervals"][:1],
                                mfcc_options=dict(snip_edges=1, frame_length_ms=20.0))
    assert (eng.mfcc_opts.snip_edges, eng.mfcc_opts.frame_shift_ms, eng.mfcc_opts.frame_length_ms) == (1, 10.0, 20.0)
    eng.configure_mfcc()


# ---- phone confidence ------------------------------------------------------------------------------------------------------

def test_phone_confidence_two_utterances_mixture_model(fx, engine):
    """The LDA mixture model, two utterances that begin at 1.5 s and 10 s of their file, and intervals that end past the last
    frame (clamped), start at it or past it (skipped), cover no whole frame (one frame) or are silence (skipped)."""
    torch = _torch()
    from montreal_forced_aligner_amd import ctm as C
    from montreal_forced_aligner_amd import finetune as FT
    s = R.lda_setup(fx)
    tm, am, table = s.tm, s.am, s.lex.phone_table
    engine.load_gmm(am)
    begins = [1.5, 10.0]
    mf = [O.mfcc(fx.pcm[int(b * R.SR): int((b + d) * R.SR)].astype(np.float32), O.default_mfcc_opts()) for b, d in zip(begins, (1.0, 0.8))]
    feats = [R.feature_chain(m, O.cmvn_stats([m]), s.lda) for m in mf]
    assert [f.shape[0] for f in feats] == [100, 80]
    frame_off = np.array([0, 100, 180], dtype=np.int64)
    name = {k: n for k, n in table if k > 0}
    ph = [k for k in sorted(name) if name[k] not in ("sil", "spn") and not name[k].startswith("#")]
    iv = lambda b, e, p: C.CtmInterval(b, e, name[p], p)      # noqa: E731
    sil = table.find("sil")
    intervals = [[iv(1.5, 1.62, ph[3]), iv(1.62, 1.625, ph[10]), iv(1.625, 2.0, sil), iv(2.0, 2.3, ph[20]), iv(2.3, 2.6, ph[30]),
                  iv(2.6, 2.7, ph[40])],
                 [iv(10.0, 10.3, ph[50]), iv(10.3, 10.8, ph[60]), iv(10.8, 10.9, ph[5])]]
    counts = {}
    for tid in range(1, tm.num_transition_ids + 1):
        c = counts.setdefault(name[int(tm.id2phone[tid])], {})
        c[str(int(tm.id2pdf[tid]))] = c.get(str(int(tm.id2pdf[tid])), 0) + 1 + (tid % 3)
    d_feats = torch.from_numpy(np.concatenate(feats)).to(engine.device)
    got = FT.phone_confidence(engine, d_feats, frame_off, counts, intervals, utt_begins=begins, silence_label="sil")
    # numpy restatement of PhoneConfidenceFunction._run (:1410-1440) on oracle scores
    names = sorted(counts)
    want = []
    for u, x in enumerate(feats):
        likes = O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, np.arange(am.num_pdfs)).astype(np.float64)
        phone_likes = np.zeros((x.shape[0], len(names)))
        for i, p in enumerate(names):
            total = sum(counts[p].values())
            phone_likes[:, i] = likes[:, [int(k) for k in counts[p]]] @ np.array([v / total for v in counts[p].values()])
        top = phone_likes.argmax(axis=1)
        res = []
        for i, pi in enumerate(intervals[u]):
            if pi.label == "sil":
                continue
            fb, fe = int(((pi.begin - begins[u]) * 1000) / 10), int(((pi.end - begins[u]) * 1000) / 10)
            if fb == fe:
                fe += 1
            fe = min(fe, top.shape[0])
            sc = [0.0 if names[top[t]] == pi.label else phone_likes[t, top[t]] - phone_likes[t, names.index(pi.label)] for t in range(fb, fe)]
            if sc:                      # (statistics.mean of nothing raises in the reference; the library skips the interval)
                res.append((i, float(np.mean(sc))))
        want.append(res)
    assert [[i for i, _ in r] for r in want] == [[0, 1, 3, 4], [0, 1]]     # silence, and the intervals from the last frame on, are skipped
    assert [[i for i, _ in r] for r in got] == [[i for i, _ in r] for r in want]
    for g, w in zip(got, want):
        assert np.allclose([x for _, x in g], [x for _, x in w], atol=2e-3), (g, w)
    assert any(abs(x) > 1.0 for r in want for _, x in r)       # the margins are not all zero: the comparison says something
