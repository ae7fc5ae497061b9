"""The corpus driver over several batches, against the oracle and against itself: ``CorpusAligner.align`` on 40 utterances
of 2 – 6 s from 4 speakers, plus one too short for its transcript, with the synthetic triphone LDA+fMLLR model — in one
batch (run A), in length-bucketed batches through the software pipeline (run B), and in the same batches with capacities
small enough that the status-3/4 redo of ``_collect`` runs in several batches, the last one included (run C).

A capacity redo cannot change a decision: C must equal B bit for bit, first pass and second (fMLLR) pass.  B must equal the
oracle's whole path from PCM with per-speaker CMVN over all of a speaker's utterances (bars of the suite: frame-identical
alignment, identical words, per-frame log-likelihood within 1e-3), and A — whose CMVN statistics are summed in another
order — must give the same alignments, words and likelihoods (bit-identical on the MI355X).  While C runs, no staging pool
that backs a batch's graphs is handed out before that batch is collected (helpers.PoolOwnership)."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance
from montreal_forced_aligner_amd.engine import PackedGraphs
from oracle import oracle as O
from tests import helpers, synth

pytestmark = pytest.mark.gpu

BATCH_FRAMES = 2500            # 41 utterances, ~16 000 frames: 7 batches
MAX_TOKENS, BP_TOKENS = 16, 16          # run C: first decodes overflow in every batch (24 on the MI355X: in none)
SHORT = 40                     # the utterance that cannot be aligned: a 6 s transcript on its first 20 frames


@pytest.fixture(scope="module")
def setup(engine):
    world = synth.SynthWorld.build()
    engine.configure_mfcc()
    lda = synth.seeded_lda()
    fm = synth.seeded_fmllr(16)
    d_lda = torch.from_numpy(lda).to(engine.device)

    def feats_of(pcm, spk):
        so = np.array([0, len(pcm)], dtype=np.int64)
        mfcc, fo = engine.mfcc(torch.from_numpy(pcm).to(engine.device), so)
        own = np.zeros(1, dtype=np.int32)
        return engine.features(mfcc, fo, own, engine.cmvn_stats(mfcc, fo, own, 1), lda=d_lda,
                               fmllr=torch.from_numpy(fm[[spk % 16]]).to(engine.device)).cpu().numpy()

    model = synth.train_triphone(world, feats_of, n_train=40, n_gauss=32, n_classes=2)
    rng = np.random.default_rng(4100)
    raw = []
    for i in range(40):
        ns = int(rng.integers(32000, 96000))
        nw = max(1, ns // int(rng.integers(5500, 8000)))
        pcm, text, _segs, _ = world.utterance(41000 + i, n_words=nw, samples=ns, speaker=i % 4)
        raw.append((pcm, text, i % 4))
    pcm, text, _segs, _ = world.utterance(41000 + SHORT, n_words=30, samples=96000, speaker=1)
    assert len(text.split()) >= 10
    raw.append((pcm[:3200].copy(), text, 1))           # (utterance() itself drops the words that do not fit)
    utts = [CorpusUtterance(f"s{spk}-{i}", f"s{spk}", pcm, text) for i, (pcm, text, spk) in enumerate(raw)]
    prev = fm[np.arange(4) % 16]                # speakers in first-appearance order s0 … s3
    pt = world.lexicon.phone_table
    sil = [pt.find("sil"), pt.find("spn")]
    return dict(world=world, lda=lda, fm=fm, model=model, raw=raw, utts=utts, prev=prev, sil=sil, runs={})


def _aligner(engine, s, **opt):
    m = s["model"]
    return CorpusAligner(m.tm, m.am, m.tree, s["world"].lexicon, lda=s["lda"], engine=engine,
                         options=AlignOptions(beam=10.0, retry_beam=40.0, **opt), silence_phones=s["sil"])


def _run(engine, s, name, speaker_adapted=False):
    """Runs A / B / C (cached per module).  C logs pool hand-outs and which batches the hard-bounds redo ran in."""
    key = (name, speaker_adapted)
    if key in s["runs"]:
        return s["runs"][key]
    opt = {"A": {}, "B": dict(batch_frames=BATCH_FRAMES),
           "C": dict(batch_frames=BATCH_FRAMES, max_tokens=MAX_TOKENS, bp_tokens_per_frame=BP_TOKENS)}[name]
    al = _aligner(engine, s, **opt)
    batches = al._batches(s["utts"])
    info = dict(batches=batches, redo=[], n_pools=None)
    with pytest.MonkeyPatch.context() as mp:
        if name == "C":
            own = helpers.PoolOwnership(mp, al)
            collect, hard_bounds = al._collect, PackedGraphs.hard_bounds
            where = {}

            def collect_(utts, prep, *a, **kw):
                where["b"] = batches.index(list(prep["idx_all"]))
                return collect(utts, prep, *a, **kw)

            def hard_bounds_(g):
                info["redo"].append((where["b"], g.n_utt))
                return hard_bounds(g)

            mp.setattr(al, "_collect", collect_)
            mp.setattr(PackedGraphs, "hard_bounds", hard_bounds_)
        res = al.align(s["utts"], speaker_adapted=speaker_adapted, make_ctm=False, previous_transforms=s["prev"])
        if name == "C":
            info["n_pools"] = own.check()
    out = dict(res=res, failed=list(al.failed), reasons=dict(al.failure_reasons), transforms=al.transforms, info=info)
    s["runs"][key] = out
    return out


def _same(r1, r2):
    """Bit-identical outcome of two runs."""
    assert r1["failed"] == r2["failed"] and r1["reasons"] == r2["reasons"]
    for k, (a, b) in enumerate(zip(r1["res"], r2["res"])):
        assert (a is None) == (b is None), k
        if a is not None:
            assert np.array_equal(a.alignment, b.alignment), k
            assert np.array_equal(a.words, b.words), k
            assert np.float32(a.likelihood).tobytes() == np.float32(b.likelihood).tobytes(), (k, a.likelihood, b.likelihood)


def test_capacity_redo_changes_nothing(engine, setup):
    s = setup
    b, c = _run(engine, s, "B"), _run(engine, s, "C")
    n = len(c["info"]["batches"])
    assert n >= 5
    redo = dict(c["info"]["redo"])                     # batch → utterances decoded again with the hard bounds
    assert n - 1 in redo and min(redo) < n - 2, c["info"]["redo"]          # non-adjacent batches, the last one included
    print(f"run C: {n} batches, hard-bounds redo in batches {sorted(redo)} for {sum(redo.values())} utterances")
    assert c["info"]["n_pools"] == n                    # every batch compiled into a pool no one else had meanwhile
    _same(b, c)


def test_batched_run_matches_the_oracle(engine, setup):
    s = setup
    b = _run(engine, s, "B")
    assert len(b["info"]["batches"]) >= 5
    m, lda, fm, raw = s["model"], s["lda"], s["fm"], s["raw"]
    gc = G.TrainingGraphCompiler(m.tm, m.tree, s["world"].lexicon)
    scaled = m.tm.scaled_log_probs(1.0, 0.1)
    mf = [O.mfcc(p.astype(np.float32), O.default_mfcc_opts()) for p, _t, _s in raw]
    n_ok = 0
    for k, (pcm, text, spk) in enumerate(raw):
        cm = O.cmvn_stats([mf[j] for j in range(len(raw)) if raw[j][2] == spk])
        x = O.affine(O.affine(O.splice(O.cmvn_apply(cm, mf[k])), lda), fm[spk % 16])
        fst = G.add_transition_probs(gc.compile_fst(text), scaled)
        ref = helpers.oracle_align_feats(m.tm, fst, x, m.am, beam=10.0, retry_beam=40.0)
        r = b["res"][k]
        if ref["status"] not in (0, 1):
            assert r is None and s["utts"][k].utt_id in b["reasons"], k
            continue
        assert r is not None, (k, b["reasons"].get(s["utts"][k].utt_id))
        assert np.array_equal(r.alignment, ref["ali"]), f"utterance {k}: alignment differs from the oracle"
        assert np.array_equal(r.words, ref["words"]), k
        assert abs(r.per_frame_likelihood - ref["like"] / len(ref["ali"])) < 1e-3, k
        n_ok += 1
    assert b["res"][SHORT] is None and b["failed"] == [s["utts"][SHORT].utt_id]
    assert n_ok == len(raw) - 1


def test_batched_run_matches_one_batch(engine, setup):
    s = setup
    a, b = _run(engine, s, "A"), _run(engine, s, "B")
    assert len(a["info"]["batches"]) == 1
    assert a["failed"] == b["failed"] and a["reasons"] == b["reasons"]
    for k, (x, y) in enumerate(zip(a["res"], b["res"])):
        assert (x is None) == (y is None), k
        if x is not None:
            assert np.array_equal(x.alignment, y.alignment) and np.array_equal(x.words, y.words), k
            # CMVN statistics are summed per batch, then over batches: another order than one batch's sum, and still the
            # same float64 totals here
            assert np.float32(x.likelihood).tobytes() == np.float32(y.likelihood).tobytes(), (k, x.likelihood, y.likelihood)


def test_two_pass_flow_with_capacity_redo(engine, setup):
    """speaker_adapted: the first passes are identical, so are the fMLLR statistics, the transforms and the second passes."""
    s = setup
    b, c = _run(engine, s, "B", speaker_adapted=True), _run(engine, s, "C", speaker_adapted=True)
    assert b["transforms"] is not None and np.array_equal(b["transforms"], c["transforms"])
    assert np.abs(b["transforms"][:, :, :40] - s["prev"][:, :, :40]).max() > 1e-3     # an estimate, not the given transforms
    assert c["info"]["redo"] and c["info"]["n_pools"] == 2 * len(c["info"]["batches"])
    _same(b, c)
