"""``SatTrainer`` on the host backend of tests/sat_case.py (no GPU): the schedule and the history, the transforms as the
composition of the recorded estimates, the alignment model's layout and purpose, the identity case, the files,
``previous_transforms``, the refusals; ``alignment_model`` itself.

Measured when the distortion of tests/sat_case.py was chosen (6 iterations, fMLLR at 0, 2 and 4, 98 leaves, 46 speakers,
11 435 non-silence frames): the three estimates gain 28.3, 3.44 and 0.69 nats per frame, every speaker's own gain is positive
(the least 5 816, 611 and 129 nats in total); on the unadapted features under the final alignments the alignment model reaches
−102.83 per frame, the speaker-adapted model −121.39: 18 nats of room for the condition asserted below."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import fmllr as F
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd.aligner import AlignOptions
from montreal_forced_aligner_amd.model import DiagGmmModel, TransitionModel
from montreal_forced_aligner_amd.stats import gmm_statistics_host, gmm_statistics_twofeats_host
from montreal_forced_aligner_amd.train import REFERENCE_FMLLR_ITERATIONS, SatTrainer, alignment_model
from tests import sat_case as SC
from tests import train_mono_case as TC

NUM_ITERATIONS, FMLLR_ITERATIONS, NUM_LEAVES = 6, (2, 4), 100


def _same_model(a, b):
    return a.num_pdfs == b.num_pdfs and all(x.tobytes() == y.tobytes() for f in ("gconsts", "weights", "means_invvars", "inv_vars")
                                            for x, y in zip(getattr(a, f), getattr(b, f)))


def _bits(st):
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count], st.tid_count))


def _trainer(backend, **kw):
    corpus = TC.train_corpus()
    kw.setdefault("previous", SC.mono_on_distorted())
    return SatTrainer(lexicon=corpus.world.lexicon, backend=backend, silence_phones=TC.silence_ids(), num_leaves=NUM_LEAVES,
                      max_gaussians=160, align_options=backend.opt, **kw)


@pytest.fixture(scope="module")
def sat_run():
    b = SC.SatHostBackend(TC.train_corpus())
    return _trainer(b, num_iterations=NUM_ITERATIONS, fmllr_iterations=FMLLR_ITERATIONS).train(), b


def test_schedule_history_and_transforms(sat_run):
    sat, b = sat_run
    h = sat.history
    assert sat.power == 0.2 and sat.opt.boost_silence == 1.0 and sat.realignment_iterations == [] and sat.final_gaussian_iteration == -4
    assert SatTrainer(lexicon=1, previous=SC.mono_on_distorted(), backend=b).fmllr_iterations == REFERENCE_FMLLR_ITERATIONS == (2, 4, 6, 12)
    assert [e["iteration"] for e in h] == list(range(NUM_ITERATIONS + 1)) and [e["realigned"] for e in h] == [True] + [False] * NUM_ITERATIONS
    assert [("fmllr" in e) for e in h] == [i in (0,) + FMLLR_ITERATIONS for i in range(NUM_ITERATIONS + 1)]
    assert {"events", "leaves", "questions", "tree_gain_per_frame", "skipped", "loglike", "gaussians", "failed", "target"} <= set(h[0])
    assert h[0]["leaves"] == sat.raw_am.num_pdfs <= NUM_LEAVES and h[0]["tree_gain_per_frame"] > 0
    print([(e["iteration"], round(e["loglike"], 3), e.get("fmllr")) for e in h])
    for e in h:
        if "fmllr" in e:
            f = e["fmllr"]
            assert set(f) == {"speakers", "rejected", "objf_impr_per_frame", "frames"}
            assert f["speakers"] == 46 and f["rejected"] == [] and f["objf_impr_per_frame"] > 0 and f["frames"] > 10000
    # every accepted speaker's own improvement
    assert len(b.gains) == 3 and all(len(g) == 46 and min(g) >= 0 for g in b.gains)
    assert h[0]["fmllr"]["objf_impr_per_frame"] > 1.0
    # the transforms: the composition of the recorded estimates, by hand
    assert sat.speakers == b.speakers and len(sat.fmllr_steps) == 3
    want = np.tile(np.eye(39, 40, dtype=np.float32), (46, 1, 1))
    for step in sat.fmllr_steps:
        for s in range(46):
            want[s] = F.compose_transforms(step[s], want[s])
    assert np.array_equal(sat.transforms, want) and np.abs(want[:, :, :39] - np.eye(39)).max() > 0.05


def test_alignment_model_layout_and_purpose(sat_run):
    sat, b = sat_run
    assert [w.shape[0] for w in sat.ali_raw_am.weights] == [w.shape[0] for w in sat.raw_am.weights]
    assert not _same_model(sat.ali_raw_am, sat.raw_am) and sat.ali_raw_tm.log_probs.shape == sat.raw_tm.log_probs.shape
    assert set(sat.history_alimdl) == {"loglike", "frames", "updated", "floored"}
    assert sat.history_alimdl["frames"] == sat.alimdl_stats.tot_count == 14400.0
    # the statistics: posteriors on the adapted features, sums of the unadapted ones
    tm, ali = TransitionModel(sat.raw_tm), np.concatenate(b.ali)
    final = DiagGmmModel.from_raw(sat.raw_am)
    want = gmm_statistics_twofeats_host(final, b.all_feats, b.all_unadapted, ali, tm)
    assert _bits(sat.alimdl_stats) == _bits(want)
    assert sat.history_alimdl["loglike"] == gmm_statistics_host(final, b.all_feats, ali, tm).loglike_per_frame
    tm2, am2 = alignment_model(sat.raw_tm, sat.raw_am, want)
    assert _same_model(am2, sat.ali_raw_am) and tm2.log_probs.tobytes() == sat.ali_raw_tm.log_probs.tobytes()
    # what it is for: the unadapted features under the final alignments
    ll_ali = gmm_statistics_host(DiagGmmModel.from_raw(sat.ali_raw_am), b.all_unadapted, ali, tm).loglike_per_frame
    ll_sat = gmm_statistics_host(final, b.all_unadapted, ali, tm).loglike_per_frame
    print(f"unadapted features, log-likelihood per frame: alignment model {ll_ali:.3f}, speaker-adapted model {ll_sat:.3f}")
    assert ll_ali > ll_sat + 1.0


def test_files(sat_run, tmp_path):
    sat, _b = sat_run
    files = sat.write(tmp_path / "sat")
    assert [p.name for p in files] == ["final.mdl", "tree", "final.alimdl"]          # no LDA: no lda.mat
    tm, am = K.read_model(files[0].read_bytes())
    ali_tm, ali_am = K.read_model(files[2].read_bytes())
    assert _same_model(am, sat.raw_am) and _same_model(ali_am, sat.ali_raw_am)
    assert ali_tm.log_probs.tobytes() == sat.ali_raw_tm.log_probs.tobytes() and np.array_equal(ali_tm.tuples, sat.raw_tm.tuples)
    # (the last iteration did not realign: its transition update and the alignment model's saw the same counts)
    assert tm.log_probs.tobytes() == sat.raw_tm.log_probs.tobytes()
    assert K.read_tree(files[1].read_bytes()) == sat.tree
    unrun = _trainer(SC.SatHostBackend(TC.train_corpus()), num_iterations=1, fmllr_iterations=())
    with pytest.raises(ValueError, match="train has not been run"):
        unrun.write(tmp_path / "none")


def test_identity_transforms_give_the_one_feature_statistics():
    """``fmllr_min_count`` above every speaker's frames: every estimate is refused, the transforms stay the identity, the
    adapted features are the unadapted ones bit for bit."""
    b = SC.SatHostBackend(TC.train_corpus(), AlignOptions(boost_silence=1.0, fmllr_min_count=1e9))
    sat = _trainer(b, num_iterations=2, fmllr_iterations=(1,)).train()
    assert [e["fmllr"]["speakers"] for e in sat.history if "fmllr" in e] == [0, 0] and len(sat.history[0]["fmllr"]["rejected"]) == 46
    assert np.array_equal(sat.transforms, np.tile(np.eye(39, 40, dtype=np.float32), (46, 1, 1)))
    assert b.all_feats.tobytes() == b.all_unadapted.tobytes()
    one = b.accumulate(sat.raw_tm, sat.raw_am)
    assert _bits(sat.alimdl_stats) == _bits(one)
    assert _same_model(sat.ali_raw_am, mle.mle_update(sat.raw_am, one, remove_low_count_gaussians=False)[0])


def test_previous_transforms_skip_the_first_estimate(sat_run):
    sat, _b = sat_run
    b = SC.SatHostBackend(TC.train_corpus())
    again = _trainer(b, previous=sat, num_iterations=1, fmllr_iterations=(1,)).train()
    assert again.previous_transforms is not None and np.array_equal(again.previous_transforms, sat.transforms)
    assert "fmllr" not in again.history[0] and "fmllr" in again.history[1] and len(again.fmllr_steps) == 1
    want = np.stack([F.compose_transforms(again.fmllr_steps[0][s], sat.transforms[s]) for s in range(46)])
    assert np.array_equal(again.transforms, want)
    # given by hand, and none: the stage starts from the identity and estimates at once
    by_hand = _trainer(SC.SatHostBackend(TC.train_corpus()), previous=(sat.raw_tm, sat.raw_am, sat.tree), previous_transforms=sat.transforms,
                       num_iterations=1, fmllr_iterations=())
    assert np.array_equal(by_hand.previous_transforms, sat.transforms)


def test_refusals():
    mono = SC.mono_on_distorted()
    kw = dict(lexicon=TC.train_corpus().world.lexicon, backend=object())
    for bad in ((2, 7), (0,), (-1, 2)):
        with pytest.raises(ValueError, match="fmllr_iterations"):
            SatTrainer(previous=mono, num_iterations=6, fmllr_iterations=bad, **kw)
    with pytest.raises(ValueError, match="previous"):
        SatTrainer(previous=None, **kw)
    with pytest.raises(ValueError, match="lexicon"):
        SatTrainer(previous=mono, backend=object())
    with pytest.raises(ValueError, match="at least 1"):
        SatTrainer(previous=mono, num_leaves=0, **kw)

    def of_dim(d):
        return K.RawAmDiagGmm(d, [], [], [], [])

    with pytest.raises(ValueError, match="feature dimension 49"):
        SatTrainer(previous=(mono.raw_tm, of_dim(49), mono.tree), **kw)
    with pytest.raises(ValueError, match="dimension 42 above 41"):                 # Δ+ΔΔ of 14 cepstra: fMLLR's limit on that path
        SatTrainer(previous=(mono.raw_tm, of_dim(42), mono.tree), **kw)
    SatTrainer(previous=(mono.raw_tm, of_dim(42), mono.tree), previous_lda=np.zeros((42, 98), np.float32), **kw)      # with an LDA: 48
    with pytest.raises(ValueError, match="LDA matrix of 40 rows"):
        SatTrainer(previous=(mono.raw_tm, of_dim(39), mono.tree), previous_lda=np.zeros((40, 91), np.float32), **kw)
