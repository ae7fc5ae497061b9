"""Flat-start monophone training on the device (montreal_forced_aligner_amd/train.py with its ``DeviceBackend``): one run over
the 48-utterance corpus of tests/train_mono_case.py, and the kalpy layer's ``gmm_init_mono`` / ``gmm_align_equal`` /
``mle_update(gmm_accs, mixup=, power=)``.

The iteration-0 statistics are held to the host twin on the device's own features and the twin's equal alignments under the
bound tests/test_gpu_gmm_acc.py uses for its soft tier (13.5·ε32·S + 2·T·2⁻⁵³·S; with one Gaussian per pdf every posterior
is exactly the weight, so the float32 part has nothing to bound and the test is, in effect, the double sums')."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import equal_align as E
from montreal_forced_aligner_amd import graph as G
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import kalpy_api as KA
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.aligner import CorpusAligner
from montreal_forced_aligner_amd.stats import gmm_statistics_host
from montreal_forced_aligner_amd.train import MonophoneTrainer
from tests import gmm_acc_ref as R
from tests import train_mono_case as C
from tests.test_gpu_gmm_acc import DEVICE_VS_TWIN, DEVICE_VS_TWIN_LL, U64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(engine):
    corpus = C.train_corpus()
    tr = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=12, max_gaussians=2 * 208,
                          silence_phones=C.silence_ids(), engine=engine)
    b = tr.backend
    init = (tr.raw_tm, tr.raw_am)
    failed = b.equal_align(tr.raw_tm, tr.raw_am, tr.tree, tr.seed)
    equal_ali = b.alignments()
    feats = [None] * len(equal_ali)
    for idx, f, _ali, fo, _rows in b.kept:
        f = f.cpu().numpy()
        for k, i in enumerate(idx):
            feats[i] = f[int(fo[k]): int(fo[k + 1])]
    tr.train()
    torch.cuda.synchronize()
    return corpus, tr, failed, equal_ali, feats, init


def test_history_holds_what_em_guarantees(run):
    _corpus, tr, failed, _ali, _feats, _init = run
    h = tr.history
    assert [e["iteration"] for e in h] == list(range(13)) and failed == 0
    assert [e["realigned"] for e in h] == [i in (0, 1, 2, 3, 5, 8, 11) for i in range(13)]
    assert h[1]["gaussians"] == 208 and h[2]["gaussians"] == 312 and all(e["gaussians"] <= e["target"] <= 416 for e in h)
    checked, bad = C.em_violations(h)
    print("checked", checked, [(e["iteration"], round(e["loglike"], 4), e["gaussians"], e["failed"]) for e in h])
    assert not bad, bad
    assert h[-1]["loglike"] > h[1]["loglike"] > h[0]["loglike"]


def test_em_on_a_run_that_never_mixes_up(engine):
    """With twice as many Gaussians as pdfs nearly every update of the run above removes a starved Gaussian and the mix-up
    puts one back, so few of its iterations qualify; with as many Gaussians as pdfs every later iteration does."""
    plain = MonophoneTrainer(C.train_corpus().utterances(), C.world().lexicon, C.topology(), num_iterations=12, max_gaussians=208,
                             silence_phones=C.silence_ids(), engine=engine).train()
    checked, bad = C.em_violations(plain.history)
    print("checked", checked, [(e["iteration"], round(e["loglike"], 4)) for e in plain.history])
    assert not any(e["mixed_up"] for e in plain.history) and plain.num_gaussians == 208
    assert set(checked) >= {4, 6, 7, 9, 10, 12} and not bad, bad


def test_equal_alignments_and_iteration_0_statistics_equal_the_twins(run):
    corpus, tr, _failed, equal_ali, feats, (raw_tm0, raw_am0) = run
    tm = M.TransitionModel(raw_tm0)
    gc = G.TrainingGraphCompiler(tm, tr.tree, C.world().lexicon)
    scaled = tm.scaled_log_probs(tr.opt.transition_scale, tr.opt.self_loop_scale)
    fsts = [G.add_transition_probs(gc.compile_fst(t), scaled) for t in corpus.text]
    fo = np.concatenate([[0], np.cumsum([x.shape[0] for x in feats])]).astype(np.int64)
    twin_ali, twin_status = E.equal_align_host(fsts, fo, np.arange(len(fsts), dtype=np.uint32), tr.seed)
    assert not twin_status.any()
    assert np.array_equal(np.concatenate(equal_ali), twin_ali)            # the key is the corpus position, whatever the batches
    am0 = M.DiagGmmModel.from_raw(raw_am0)
    x = np.concatenate(feats)
    twin = gmm_statistics_host(am0, x, twin_ali, tm)
    st = tr.initial_stats
    pdf, fw = R.frame_tables(tm, twin_ali)
    ref = R.gmm_acc(x, pdf, fw, am0)
    T2 = 2.0 * ref["n_frames"] * U64
    for name, got, want, S, t2 in (("occ", st.occ, twin.occ, ref["occ"], T2), ("mean", st.mean_acc, twin.mean_acc, ref["S_mean"], T2[:, None]),
                                   ("var", st.var_acc, twin.var_acc, ref["var"], T2[:, None])):
        err, lim = np.abs(got - want), (DEVICE_VS_TWIN * R.EPS32 + t2) * S
        assert (err <= lim).all(), name
    lim_ll = R.EPS32 * (ref["S_tot"] + DEVICE_VS_TWIN_LL * float(fw.sum())) + 2 * len(pdf) * U64 * ref["S_tot"]
    assert abs(st.tot_like - twin.tot_like) <= lim_ll
    assert st.tot_count == twin.tot_count == float(len(twin_ali)) and np.array_equal(st.tid_count, twin.tid_count)
    assert np.array_equal(st.occ, twin.occ)                                # one Gaussian per pdf: every posterior is 1


def test_written_model_aligns_every_training_utterance_and_beats_the_equal_alignments(run, engine, tmp_path):
    corpus, tr, _failed, equal_ali, _feats, (raw_tm0, _am0) = run
    mdl, tree_path = tr.write(tmp_path / "mono")
    tm, am = M.load_model_bytes(mdl.read_bytes())
    tree = K.read_tree(tree_path.read_bytes())
    assert tree == tr.tree and am.num_gauss == tr.num_gaussians
    al = CorpusAligner(tm, am, tree, C.world().lexicon, engine=engine, silence_phones=C.silence_ids(), options=tr.opt)
    res = al.align(corpus.utterances(), make_ctm=False)
    assert all(r is not None for r in res), al.failure_reasons           # status 0 or 1 for every training utterance
    share = C.phone_share(corpus, tr.raw_tm, [r.alignment for r in res])
    equal_share = C.phone_share(corpus, raw_tm0, equal_ali)
    print(f"frames on the generator's phone: equal alignments {equal_share:.4f}, trained model {share:.4f}")
    assert share > equal_share
    again = tr.aligner().align(corpus.utterances()[:4], make_ctm=False)
    assert all(np.array_equal(a.alignment, b.alignment) for a, b in zip(again, res[:4]))


def test_kalpy_layer(run, engine, tmp_path, monkeypatch):
    corpus, tr, _failed, equal_ali, feats, (raw_tm0, raw_am0) = run
    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    topo = C.topology()
    KA.gmm_init_mono(topo, feats[:8], [], str(tmp_path / "0.mdl"), str(tmp_path / "tree"))
    tm, am = KA.read_gmm_model(tmp_path / "0.mdl")
    tree = K.read_tree((tmp_path / "tree").read_bytes())
    assert tree == tr.tree and am.num_pdfs == am.num_gauss == 208 and am.dim == 39 and tm.num_pdfs == 208
    x = np.concatenate(feats[:8]).astype(np.float64)
    mean = am.means_invvars[0].astype(np.float64) / am.inv_vars[0]
    assert np.allclose(mean, x.mean(axis=0), rtol=0, atol=1e-5 * (1 + np.abs(x.mean(axis=0)).max()))
    assert np.allclose(1.0 / am.inv_vars[5].astype(np.float64), x.var(axis=0), rtol=1e-5)
    # gmm_align_equal on one graph: the batch entry's result for key 0
    gc = G.TrainingGraphCompiler(tm, tree, C.world().lexicon)
    fst = gc.compile_fst(corpus.text[0])
    ali, words = KA.gmm_align_equal(fst, feats[0], seed=tr.seed)
    want, status = E.equal_align_host([fst], np.array([0, feats[0].shape[0]]), [0], tr.seed)
    assert status[0] == 0 and ali == want.tolist() and ali == equal_ali[0].tolist()
    assert words == [C.world().lexicon.to_int(w) for w in corpus.text[0].split()]
    assert KA.gmm_align_equal(fst, feats[0][:3]) == (None, None)
    # the training form of mle_update, on the accumulator object the adaptation layer has
    acc = KA.AccumAmDiagGmm()
    acc.stats = tr.initial_stats.copy()
    soa = M.DiagGmmModel.from_raw(raw_am0)
    impr, count = soa.mle_update(acc, mixup=260, power=0.25, min_gaussian_occupancy=3.0, rng=np.random.default_rng(1))
    assert impr > 0 and count == tr.initial_stats.occ.sum() and 208 < soa.num_gauss <= 260
    want_am, *_ = mle.mle_update(raw_am0, tr.initial_stats, min_gaussian_occupancy=3.0)
    want_am, _t = mle.mix_up(want_am, mle.pdf_occupancies(raw_am0, tr.initial_stats), 260, 0.25, rng=np.random.default_rng(1))
    assert np.array_equal(soa.means_invvars, np.concatenate(want_am.means_invvars)) and np.array_equal(soa.gconsts, np.concatenate(want_am.gconsts))
