"""MLLT through the host layers, on the device: ``CorpusAligner.estimate_mllt`` against the chain by hand (the same resident
features and alignments, downloaded → ``mllt_statistics_host`` → ``mllt_accs`` → ``estimate_mllt``), one short ``LdaTrainer``
run with an MLLT iteration, written, reloaded and aligned with, and the kalpy names.  The corpus is the 48 utterances of
tests/train_mono_case.py, the model a monophone model of 6 iterations, trained here, with its fullest pdfs split once (so that
posteriors are soft).

How the statistics' bound reaches the matrix.  Device and twin statistics differ by at most
B_F[g] = (13.5·ε32 + 2·T_p·2⁻⁵³)·S_full[g] elementwise (tests/mllt_ref.py), so G_j = Σ_g inv_var_g[j]·F_g by at most
B_G[j] = Σ_g inv_var_g[j]·B_F[g], and beta by B_beta = Σ_g (13.5·ε32 + 2·T_p·2⁻⁵³)·occ_g.  The estimate is a smooth function of
(beta, G); to first order its response to a perturbation E inside that box is J·E.  J is probed at the reference: the
estimate is run again on the twin's statistics moved by ±B with random signs (a symmetric pattern per G_j), which gives
responses r with E[r²] = Σ_k J_k²·B_k² per element of the matrix; by Cauchy–Schwarz the worst case over the box,
Σ_k |J_k|·B_k, is at most √N times that root mean square, N = D·D·(D + 1)/2 + 1 the number of independent entries.  The
matrix from the device statistics is held to √N · (largest probe response) plus one float32 ulp of the result's cast."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import kalpy_api as KA
from montreal_forced_aligner_amd import lda, mllt
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.aligner import CorpusAligner
from montreal_forced_aligner_amd.stats import MlltStats, mllt_statistics_host, silence_weights
from montreal_forced_aligner_amd.train import LdaTrainer, MonophoneTrainer
from tests import gmm_acc_ref as R
from tests import mllt_ref as MR
from tests import train_mono_case as C

pytestmark = pytest.mark.gpu
SWEEPS = 40


@pytest.fixture(scope="module")
def mono(engine):
    corpus = C.train_corpus()
    tr = MonophoneTrainer(corpus.utterances(), C.world().lexicon, C.topology(), num_iterations=6, max_gaussians=208,
                          silence_phones=C.silence_ids(), engine=engine).train()
    # six iterations never mix up (final_gaussian_iteration = −4): split the fullest pdfs once by hand
    from montreal_forced_aligner_amd import mle
    stats = tr.backend.accumulate(tr.raw_tm, tr.raw_am)
    tr.raw_am, _targets = mle.mix_up(tr.raw_am, mle.pdf_occupancies(tr.raw_am, stats), 260, tr.power, rng=tr.rng)
    assert tr.num_gaussians == 260 and tr.raw_am.num_pdfs == 208
    return corpus, tr


def by_hand(al, utts):
    """What ``estimate_mllt`` works on, downloaded: (final features, alignments, utterance ids) per batch."""
    out = []
    with al._run():
        _res, kept = al._align(utts, False, False, None, keep_last=True)
        for idx, feats, ali, fo, _rows in kept:
            out.append((feats.cpu().numpy(), ali.cpu().numpy(), np.asarray(fo, np.int64), [utts[i].utt_id for i in idx]))
    return out


def host_chain(al, batches):
    am, tm = M.DiagGmmModel.from_raw(al.raw_am), al.tm
    weights = silence_weights(tm, C.silence_ids(), 0.0)
    st = None
    for feats, ali, _fo, _ids in batches:
        st = mllt_statistics_host(am, feats, ali, tm, weights, into=st)
    feats, ali = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    pdf, fw = R.frame_tables(tm, ali, weights)
    ref = MR.mllt_acc(feats, pdf, fw, am)
    return am, st, ref


def test_estimate_mllt_against_the_chain_by_hand(mono):
    corpus, tr = mono
    utts = corpus.utterances()
    al = tr.aligner()
    mat, impr, count, trace = al.estimate_mllt(utts, num_sweeps=SWEEPS)
    got = al.mllt_stats
    am, want, ref = host_chain(al, by_hand(al, utts))
    D = am.dim
    assert mat.shape == (D, D) and mat.dtype == np.float32 and len(trace) == SWEEPS and impr > 0
    rel = (MR.DEVICE_VS_TWIN * R.EPS32 + 2.0 * ref["n_frames"] * MR.U64)
    B_F = rel[:, None, None] * ref["S_full"]
    assert got.tot_count == want.tot_count and count == float(got.occ.sum()) and count > 5000
    assert (np.abs(got.full - want.full) <= B_F).all() and (np.abs(got.occ - want.occ) <= rel * ref["occ"]).all()
    assert (ref["post"].max(axis=1) < 0.9).sum() > 50                          # soft posteriors took part
    # the box on (beta, G), probed at the reference (module docstring)
    iv = am.inv_vars.astype(np.float64)
    B_G = (iv.T @ B_F.reshape(len(iv), D * D)).reshape(D, D, D)
    B_beta = float((rel * ref["occ"]).sum())
    beta, G = mllt.mllt_accs(want, am)
    base = mllt.estimate_mllt(beta, G, num_sweeps=SWEEPS, dtype=np.float64)[0]
    rng = np.random.default_rng(1)
    response = 0.0
    for _probe in range(2):
        sign = np.sign(rng.normal(size=(D, D, D)))
        sign = np.tril(sign) + np.swapaxes(np.tril(sign, -1), 1, 2)
        moved = mllt.estimate_mllt(beta + rng.choice([-1.0, 1.0]) * B_beta, G + sign * B_G, num_sweeps=SWEEPS, dtype=np.float64)[0]
        response = max(response, float(np.abs(moved - base).max()))
    N = D * D * (D + 1) // 2 + 1
    lim = np.sqrt(N) * response + 2.0 ** -23 * np.abs(base)
    err = np.abs(mat.astype(np.float64) - base)
    print(f"estimate_mllt: |device - chain by hand| max {err.max():.3g}, probe response {response:.3g}, sqrt(N) {np.sqrt(N):.1f}")
    assert (err <= lim).all()
    # the device statistics through the same host code: the same matrix, bit for bit
    again = mllt.estimate_mllt(*mllt.mllt_accs(got, al.raw_am), num_sweeps=SWEEPS)
    assert np.array_equal(again[0], mat) and again[1] == impr and again[2] == count
    # the aligner still aligns with its own (boosted) model afterwards
    assert all(r is not None for r in al.align(utts[:4], make_ctm=False))


def test_lda_trainer_with_an_mllt_iteration_on_the_device(mono, engine, tmp_path):
    corpus, tr = mono
    utts = corpus.utterances()
    ldat = LdaTrainer(utts, C.world().lexicon, previous=(tr.raw_tm, tr.raw_am, tr.tree), num_iterations=2, max_gaussians=208,
                      silence_phones=C.silence_ids(), engine=engine, mllt_iterations=(1,), mllt_sweeps=SWEEPS).train()
    torch.cuda.synchronize()
    h = ldat.history
    assert [("mllt" in e) for e in h] == [False, True, False] and len(ldat.mllt_mats) == 1
    assert h[1]["mllt"]["objf_impr_per_frame"] > 0 and ldat.logdet_total == h[1]["mllt"]["logdet"]
    # same alignments throughout, no mix-up: the comparable log-likelihood does not fall (em_violations' rule and allowance)
    comparable = [dict(e, loglike=e["loglike"] + (ldat.logdet_total if e["iteration"] >= 1 else 0.0)) for e in h]
    checked, bad = C.em_violations(comparable)
    assert checked == [1, 2] and bad == []
    first, _full = lda.estimate_lda(ldat.lda_stats, dim=40)
    want = mllt.compose_transforms(ldat.mllt_mats[0], first)
    assert np.array_equal(ldat.lda_mat, want) and not np.array_equal(want, first)
    mdl, tree_path, mat_path = ldat.write(tmp_path / "lda_mllt")
    tm, am = M.load_model_bytes(mdl.read_bytes())
    mat = K.read_matrix_file(mat_path.read_bytes())
    assert am.dim == 40 and np.array_equal(mat, want)
    al = CorpusAligner(tm, am, K.read_tree(tree_path.read_bytes()), C.world().lexicon, lda=mat, options=ldat.opt, engine=engine,
                       silence_phones=C.silence_ids())
    res = al.align(utts, make_ctm=False)
    assert all(r is not None for r in res) and al.failed == []
    own = ldat.aligner().align(utts, make_ctm=False)
    for a, b in zip(res, own):
        assert np.array_equal(a.alignment, b.alignment)


def test_kalpy_layer(mono, engine, tmp_path, monkeypatch):
    corpus, tr = mono
    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    utts = corpus.utterances()
    al = tr.aligner()
    batches = by_hand(al, utts)
    _am, _want, ref = host_chain(al, batches)
    al.estimate_mllt(utts, num_sweeps=1)          # (before the accumulators load their model into the shared engine)
    own = al.mllt_stats
    mdl, _tree = tr.write(tmp_path / "mono")
    feats, alis = {}, []
    for x, ali, fo, ids in batches:
        for k, uid in enumerate(ids):
            feats[uid] = x[fo[k]: fo[k + 1]]
            alis.append((uid, ali[fo[k]: fo[k + 1]]))
    alis.sort(key=lambda e: e[0])
    K.write_table(tmp_path / "ali.ark", alis, "int_vector")
    acc = KA.MlltStatsAccumulator(mdl, C.silence_ids(), rand_prune=4.0)          # accepted and ignored
    seen = []
    acc.accumulate_stats(feats, KA.AlignmentArchive(tmp_path / "ali.ark"), callback=seen.append)
    assert sorted(seen) == sorted(u.utt_id for u in utts)
    st = acc.mllt_accs.stats
    assert isinstance(st, MlltStats) and st.tot_count > 5000
    plain = KA.MlltStatsAccumulator(mdl, C.silence_ids(), rand_prune=0.0)
    plain.accumulate_stats(feats, KA.AlignmentArchive(tmp_path / "ali.ark"))
    assert plain.mllt_accs.stats.full.tobytes() == st.full.tobytes()
    # the statistics are the aligner's own (the utterances in another order: under the summation bound)
    T2 = (2.0 * ref["n_frames"] * MR.U64)
    assert (np.abs(st.full - own.full) <= T2[:, None, None] * ref["S_full"]).all() and st.tot_count == own.tot_count
    # Add → update → compose_transforms: estimate_mllt on the same statistics
    total = KA.MlltAccs()
    total.Add(acc.mllt_accs)
    mat, objf_impr, count = total.update(num_sweeps=SWEEPS)
    want = mllt.estimate_mllt(*mllt.mllt_accs(st, acc.acoustic_model), num_sweeps=SWEEPS)
    assert np.array_equal(mat, want[0]) and objf_impr == want[1] and count == want[2] == float(st.occ.sum())
    total.Add(acc.mllt_accs)                                                     # twice the statistics: the same transform
    twice, impr2, count2 = total.update(num_sweeps=SWEEPS)
    assert count2 == 2 * count and np.allclose(twice, mat, rtol=1e-5, atol=1e-6) and abs(impr2 - 2 * objf_impr) <= 1e-9 * impr2
    prev = np.random.default_rng(0).normal(size=(mat.shape[0], 91)).astype(np.float32)
    assert np.array_equal(KA.compose_transforms(mat, prev, False), mllt.compose_transforms(mat, prev))
    with pytest.raises(ValueError, match="affine"):
        KA.compose_transforms(mat, prev, True)
    with pytest.raises(ValueError, match="no statistics"):
        KA.MlltAccs().update()
