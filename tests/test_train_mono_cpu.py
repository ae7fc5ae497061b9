"""Flat-start monophone training (montreal_forced_aligner_amd/train.py) on the host backend of tests/train_mono_case.py:
the same loop the device runs, over mfa_debug_align_equal_host, gmm_statistics_host and the oracle's aligner.  48 synthetic
utterances of 3 s, 12 iterations, twice as many Gaussians as pdfs at most.

Measured on this corpus (the figures DESIGN §2 quotes): the share of frames on the generator's phone rises from 0.16 under
the equal alignments to 0.80 under the final model's; the median phone-boundary error on 16 held-out utterances is 7.5 ms
against 3.1 ms for the supervised yardstick (synth_workload.train_monophone on the same 48 utterances, from the generator's
own labels, which are themselves quantised to a 10 ms frame).  Asserted: within one frame of the yardstick."""
import io

import numpy as np
import pytest

from montreal_forced_aligner_amd import adapt as A
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.train import MonophoneTrainer, realignment_iterations
from tests import train_mono_case as C

FRAME = 0.010


def _trainer(backend, **kw):
    kw.setdefault("num_iterations", 12)
    return MonophoneTrainer(lexicon=C.world().lexicon, topology=C.topology(), backend=backend, silence_phones=C.silence_ids(), **kw)


@pytest.fixture(scope="module")
def run():
    corpus = C.train_corpus()
    backend = C.HostBackend(corpus)
    tr = _trainer(backend, max_gaussians=2 * 208)
    assert tr.initial_gaussians == 208 and tr.max_gaussians == 2 * tr.initial_gaussians
    failed = backend.equal_align(tr.raw_tm, tr.raw_am, tr.tree, tr.seed)
    equal_share = C.phone_share(corpus, tr.raw_tm, backend.alignments())
    tr.train()
    return corpus, tr, failed, equal_share


def test_schedule_is_the_references():
    assert realignment_iterations(40) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 38]
    assert realignment_iterations(12) == [0, 1, 2, 3, 5, 8, 11]
    tr = _trainer(C.HostBackend(C.train_corpus()), num_iterations=40, max_gaussians=1000)
    assert tr.final_gaussian_iteration == 30 and tr.gaussian_increment == int((1000 - 208) / 30)
    assert (tr.power, tr.initial_beam, tr.opt.boost_silence, tr.opt.beam, tr.opt.retry_beam) == (0.25, 6.0, 1.25, 10.0, 40.0)


def test_history_and_gaussian_counts(run):
    _corpus, tr, failed, _share = run
    h = tr.history
    assert [e["iteration"] for e in h] == list(range(13)) and failed == 0 and h[0]["failed"] == 0
    assert [e["realigned"] for e in h] == [i in (0, 1, 2, 3, 5, 8, 11) for i in range(13)]
    assert [e["target"] for e in h] == [208, 208, 312, 416] + [416] * 9
    assert h[0]["gaussians"] == h[1]["gaussians"] == 208 and h[2]["gaussians"] == 312 and h[-1]["gaussians"] == tr.num_gaussians
    assert all(e["gaussians"] <= e["target"] for e in h) and tr.num_gaussians <= tr.max_gaussians
    assert all(np.isfinite(e["loglike"]) and e["frames"] > 0 for e in h)
    assert max(w.shape[0] for w in tr.raw_am.weights) <= 128
    for p in range(tr.raw_am.num_pdfs):
        assert abs(float(tr.raw_am.weights[p].astype(np.float64).sum()) - 1.0) <= 130 * 2.0 ** -24
    assert tr.initial_stats is not None and tr.initial_stats.tot_count == h[0]["frames"]


def test_em_never_loses_likelihood(run):
    """What EM guarantees, asserted at every iteration it covers.  With twice as many Gaussians as pdfs on 14 400 frames
    nearly every update removes a starved Gaussian and the mix-up puts one back, so few iterations of the main run qualify;
    a second run that never mixes up (as many Gaussians as pdfs) has six in a row that do."""
    _corpus, tr, _failed, _share = run
    checked, bad = C.em_violations(tr.history)
    print("mixing run: checked", checked, [(e["iteration"], round(e["loglike"], 4)) for e in tr.history])
    assert not bad, bad
    plain = _trainer(C.HostBackend(C.train_corpus()), max_gaussians=208).train()
    checked, bad = C.em_violations(plain.history)
    print("plain run: checked", checked, [(e["iteration"], round(e["loglike"], 4)) for e in plain.history])
    assert not any(e["mixed_up"] for e in plain.history) and plain.num_gaussians == 208
    assert set(checked) >= {4, 6, 7, 9, 10, 12} and not bad, bad


def test_final_alignments_beat_the_equal_ones(run):
    corpus, tr, _failed, equal_share = run
    final = C.host_align(corpus, tr.raw_tm, tr.raw_am, tr.tree, tr.opt)
    share = C.phone_share(corpus, tr.raw_tm, final)
    print(f"frames on the generator's phone: equal alignments {equal_share:.4f}, final model {share:.4f}")
    assert share > equal_share


def test_boundaries_within_a_frame_of_the_supervised_yardstick(run):
    _corpus, tr, _failed, _share = run
    held = C.held_out_corpus()
    flat = C.boundary_errors(held, tr.raw_tm, C.host_align(held, tr.raw_tm, tr.raw_am, tr.tree, tr.opt))
    y = C.supervised_yardstick()
    yard = C.boundary_errors(held, y.tm.raw, C.host_align(held, y.tm.raw, A.raw_from_soa(y.am), y.tree, tr.opt))
    print(f"median phone-boundary error on {C.N_HELD_OUT} held-out utterances: flat start {1e3 * np.median(flat):.2f} ms "
          f"({len(flat)} boundaries), supervised yardstick {1e3 * np.median(yard):.2f} ms ({len(yard)} boundaries)")
    assert len(flat) >= 400 and len(yard) >= 400
    assert np.median(flat) <= np.median(yard) + FRAME


def test_written_model_reads_back(run, tmp_path):
    _corpus, tr, _failed, _share = run
    paths = tr.write(tmp_path / "mono")
    assert [p.name for p in paths] == ["final.mdl", "tree"]
    tm, am = M.load_model_bytes(paths[0].read_bytes())
    assert am.num_gauss == tr.num_gaussians and tm.num_pdfs == tr.raw_am.num_pdfs == 208
    assert K.read_tree(paths[1].read_bytes()) == tr.tree
    f = io.BytesIO()
    K.write_model(f, tr.raw_tm, tr.raw_am)
    assert f.getvalue() == paths[0].read_bytes()


def test_limits_are_refused():
    with pytest.raises(ValueError, match="lexicon and a topology"):
        MonophoneTrainer(backend=C.HostBackend(C.train_corpus()))

    class Wide:
        dim = 49
    with pytest.raises(ValueError, match="48"):
        _trainer(Wide())
    # a target of more than 128 Gaussians in a pdf: one pdf holds nearly all frames
    tr = _trainer(C.HostBackend(C.train_corpus()), max_gaussians=208)
    occ = np.full(208, 25.0)
    occ[3] = 1.0e6
    with pytest.raises(ValueError, match="128"):
        mle.mix_up(tr.raw_am, occ, 208 + 140, rng=np.random.default_rng(0))
