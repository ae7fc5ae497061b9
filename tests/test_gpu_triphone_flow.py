"""The triphone stage through the host layers, on the device: ``CorpusAligner.tree_statistics`` against the chain by hand
(downloaded features and alignments → ``tree_statistics_host``); one short ``TriphoneTrainer`` run held to what the host run
is held to (tests/test_tree_cpu.py), written, reloaded and aligned with; ``LdaTrainer(num_leaves=…)`` for one iteration; the
kalpy names.  The corpus is the 48 utterances of tests/train_mono_case.py, the previous model a monophone model of 6
iterations trained here."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import kalpy_api as KA
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd import tree as T
from montreal_forced_aligner_amd.aligner import CorpusAligner
from montreal_forced_aligner_amd.stats import TreeStats, tree_statistics_host
from montreal_forced_aligner_amd.train import REFERENCE_MLLT_ITERATIONS, LdaTrainer, MonophoneTrainer, TriphoneTrainer
from tests import train_mono_case as C
from tests import tree_ref as R
from tests.test_tree_cpu import NUM_LEAVES, check_triphone_training

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mono(engine):
    corpus = C.train_corpus()
    tr = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=6, max_gaussians=208,
                          silence_phones=C.silence_ids(), engine=engine)
    tr.backend.equal_align(tr.raw_tm, tr.raw_am, tr.tree, tr.seed)
    equal_share = C.phone_share(corpus, tr.raw_tm, tr.backend.alignments())
    tr.train()
    res = tr.aligner().align(corpus.utterances(), make_ctm=False)
    mono_share = C.phone_share(corpus, tr.raw_tm, [None if r is None else r.alignment for r in res])
    return corpus, tr, equal_share, mono_share


def by_hand(al, utts):
    """What ``tree_statistics`` works on, downloaded: per batch (final features, frame offsets, alignments, corpus positions)."""
    with al._run():
        _res, kept = al._align(utts, False, False, None, keep_last=True)
        return [(feats.cpu().numpy(), np.asarray(fo, np.int64), ali.cpu().numpy(), list(idx)) for idx, feats, ali, fo, _rows in kept]


def host_stats(al, batches):
    want, skipped = TreeStats.zeros(batches[0][0].shape[1]), 0
    for feats, fo, ali, _idx in batches:
        st, _fe, sk = tree_statistics_host(feats, fo, ali, al.tm, C.silence_ids())
        want += st
        skipped += sk
    return want, skipped


def test_tree_statistics_against_the_chain_by_hand(mono):
    corpus, tr, _e, _m = mono
    utts = corpus.utterances()
    al = tr.aligner()
    got = al.tree_statistics(utts)
    want, skipped = host_stats(al, by_hand(al, utts))
    assert got is al.tree_stats and got.num_events > 1000 and al.tree_skipped == skipped <= 2
    assert np.array_equal(got.keys, want.keys) and np.array_equal(got.count, want.count)
    assert int(got.count.sum()) > 12000
    # per event the two sides add the same exact terms in two orders: (2n + 2)·2⁻⁵³·Σ|x| ≤ (2n + 2)·2⁻⁵³·√(n·Σx²)
    n = got.count[:, None].astype(np.float64)
    assert np.all(np.abs(got.sum - want.sum) <= (2 * n + 2) * R.U64 * np.sqrt(n * want.sumsq))
    assert np.all(np.abs(got.sumsq - want.sumsq) <= (2 * n + 2) * R.U64 * want.sumsq)
    W = got.windows()
    sil = np.isin(W[:, 1], C.silence_ids())
    assert sil.any() and np.all(W[sil][:, [0, 2]] == 0) and (W[~sil][:, [0, 2]] > 0).any()
    # other context-independent phones: other events
    none = al.tree_statistics(utts, ci_phones=[])
    assert none.num_events > got.num_events and int(none.count.sum()) == int(got.count.sum())


@pytest.fixture(scope="module")
def tri_run(mono, engine):
    corpus, tr, _e, _m = mono
    tri = TriphoneTrainer(corpus.utterances(), C.world().lexicon, previous=tr, num_iterations=11, num_leaves=NUM_LEAVES,
                          max_gaussians=NUM_LEAVES + 60, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    return tri


def test_triphone_trainer_on_the_device(mono, tri_run, engine, tmp_path):
    corpus, tr, equal_share, mono_share = mono
    tri = tri_run
    utts = corpus.utterances()
    own = tri.aligner().align(utts, make_ctm=False)
    share = check_triphone_training(corpus, tr, tri, [None if r is None else r.alignment for r in own], equal_share, mono_share)
    assert share >= mono_share > equal_share               # no spread to borrow from the monophone test: the margin is zero
    # write, reload the two files, align every training utterance: the same alignments; the tree is the one in memory
    mdl, tree_path = tri.write(tmp_path / "tri")
    tm, am = M.load_model_bytes(mdl.read_bytes())
    tree = K.read_tree(tree_path.read_bytes())
    assert tree == tri.tree and am.num_pdfs == tri.history[0]["leaves"]
    al = CorpusAligner(tm, am, tree, C.world().lexicon, options=tri.opt, engine=engine, silence_phones=C.silence_ids())
    res = al.align(utts, make_ctm=False)
    assert [r is None for r in res] == [r is None for r in own] and sum(r is None for r in res) <= 2
    for a, b in zip(res, own):
        assert a is None or np.array_equal(a.alignment, b.alignment)


def test_lda_trainer_builds_its_own_tree(mono, tri_run, engine):
    corpus, tr, _e, _m = mono
    ldat = LdaTrainer(corpus.utterances(), C.world().lexicon, previous=tri_run, num_iterations=1, num_leaves=260,
                      max_gaussians=300, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    h = ldat.history
    assert [e["iteration"] for e in h] == [0, 1] and all(np.isfinite(e["loglike"]) for e in h)
    assert 100 < h[0]["leaves"] <= 260 and h[0]["events"] == ldat.tree_stats.num_events and h[0]["tree_gain_per_frame"] > 0
    assert ldat.raw_am.dim == 40 and ldat.raw_am.num_pdfs == h[0]["leaves"] == len(set(ldat.tree.to_pdf.leaves()))
    assert ldat.tree is not tri_run.tree and ldat.tree_stats.dim == 40
    # EM over the one plain iteration, and the model aligns
    checked, bad = C.em_violations(h)
    assert bad == []
    res = ldat.aligner().align(corpus.utterances(), make_ctm=False)
    assert sum(r is None for r in res) <= 2
    # the default leaves the tree alone
    plain = LdaTrainer(corpus.utterances(), C.world().lexicon, previous=tri_run, num_iterations=1, max_gaussians=300,
                       silence_phones=C.silence_ids(), engine=engine).train()
    assert plain.tree is tri_run.tree and plain.raw_am.num_pdfs == tri_run.raw_am.num_pdfs and "leaves" not in plain.history[0]


def test_monophone_to_triphone_to_lda_mllt_without_a_tree_from_outside(mono, tri_run, engine, tmp_path):
    """The chain the stages exist for: the monophone model of ``mono`` → ``tri_run`` → the reference's LDA+MLLT stage on a
    tree of its own."""
    corpus, tr, equal_share, _m = mono
    ldat = LdaTrainer(corpus.utterances(), C.world().lexicon, previous=tri_run, num_iterations=12, num_leaves=260,
                      max_gaussians=320, mllt_iterations=REFERENCE_MLLT_ITERATIONS, silence_phones=C.silence_ids(), engine=engine).train()
    torch.cuda.synchronize()
    h = ldat.history
    assert [e["iteration"] for e in h] == list(range(13)) and [("mllt" in e) for e in h] == [i in REFERENCE_MLLT_ITERATIONS for i in range(13)]
    assert all(e["mllt"]["objf_impr_per_frame"] > 0 for e in h if "mllt" in e) and len(ldat.mllt_mats) == 4
    assert ldat.raw_am.num_pdfs == h[0]["leaves"] <= 260 and ldat.lda_mat.shape == (40, 91)
    mdl, tree_path, mat_path = ldat.write(tmp_path / "lda")
    tm, am = M.load_model_bytes(mdl.read_bytes())
    assert K.read_tree(tree_path.read_bytes()) == ldat.tree and am.num_pdfs == ldat.raw_am.num_pdfs
    al = CorpusAligner(tm, am, K.read_tree(tree_path.read_bytes()), C.world().lexicon, lda=K.read_matrix_file(mat_path.read_bytes()),
                       options=ldat.opt, engine=engine, silence_phones=C.silence_ids())
    res = al.align(corpus.utterances(), make_ctm=False)
    share = C.phone_share(corpus, ldat.raw_tm, [None if r is None else r.alignment for r in res])
    print(f"frames on the generator's phone after monophone -> triphone -> LDA+MLLT: {share:.4f}")
    assert sum(r is None for r in res) <= 2 and share > equal_share


def test_kalpy_layer(mono, engine, tmp_path, monkeypatch):
    corpus, tr, _e, _m = mono
    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    utts = corpus.utterances()
    al = tr.aligner()
    batches = by_hand(al, utts)
    mdl, _tree = tr.write(tmp_path / "mono")
    feats, alis = {}, []
    for x, fo, ali, idx in batches:
        for k, i in enumerate(idx):
            if np.all(ali[fo[k]: fo[k + 1]] > 0):
                feats[utts[i].utt_id] = x[fo[k]: fo[k + 1]]
                alis.append((utts[i].utt_id, ali[fo[k]: fo[k + 1]]))
    alis.sort(key=lambda e: e[0])
    K.write_table(tmp_path / "ali.ark", alis, "int_vector")
    acc = KA.TreeStatsAccumulator(mdl, context_independent_symbols=C.silence_ids(), batch_frames=4000)
    seen = []
    acc.accumulate_stats(feats, KA.AlignmentArchive(tmp_path / "ali.ark"), callback=seen.append)
    assert sorted(seen) == [k for k, _a in alis] and acc.skipped == 0
    st = acc.tree_stats
    want, _skipped = host_stats(al, batches)
    assert np.array_equal(st.keys, want.keys) and np.array_equal(st.count, want.count)
    n = st.count[:, None].astype(np.float64)                # other batch cuts, the same exact terms: the bound of the test above
    assert np.all(np.abs(st.sum - want.sum) <= (2 * n + 2) * R.U64 * np.sqrt(n * want.sumsq))
    assert np.all(np.abs(st.sumsq - want.sumsq) <= (2 * n + 2) * R.U64 * want.sumsq)
    topo = tr.raw_tm.topo
    phone_sets = [[int(p)] for p in topo.phones]
    qs = KA.automatically_obtain_questions(st, phone_sets, [1], 1)
    roots = tmp_path / "roots.int"
    sil = set(C.silence_ids())
    roots.write_text("".join(("not-shared not-split" if p[0] in sil else "shared split") + f" {p[0]}\n" for p in phone_sets))
    record = KA.build_tree(topo, qs, st, str(roots), str(tmp_path / "tree"), max_leaves=240, cluster_thresh=-1)
    tree = KA.read_tree(tmp_path / "tree")
    assert 100 < record["leaves"] <= 240
    KA.gmm_init_model(topo, tree, st, str(tmp_path / "1.mdl"))
    new_tm, new_am = KA.read_gmm_model(tmp_path / "1.mdl")
    assert new_am.num_pdfs == record["leaves"]
    old_tm = KA.read_transition_model(mdl)
    key, old = alis[0]
    new = np.asarray(KA.convert_alignments(old_tm, new_tm, tree, old.tolist()))
    assert np.array_equal(old_tm.id2phone[old], new_tm.id2phone[new]) and np.array_equal(old_tm.is_self_loop[old], new_tm.is_self_loop[new])
    # the device gather gives the same
    st1, fe1, _sk = tree_statistics_host(feats[key], np.array([0, len(old)]), old, old_tm, ())
    table = T.convert_table(old_tm, new_tm, tree, st1)
    dev = T.convert_alignments(table, T.local_of_tid(old_tm), torch.from_numpy(fe1).to(engine.device), torch.from_numpy(old).to(engine.device))
    assert np.array_equal(dev.cpu().numpy(), new)
    with pytest.raises(NotImplementedError):
        KA.gmm_init_model_from_previous()
