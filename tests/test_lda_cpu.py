"""The LDA stage without a GPU: the host twin of the statistics (mfa_debug_lda_acc_host) against the float64 restatement of
tests/lda_ref.py, the random prune, ``estimate_lda`` against its identities, a brute-force restatement and a known answer, the
refusals, the twin's translation unit under the host sanitizers as a stand-alone program (nothing is preloaded anywhere), and
``LdaTrainer`` on a host backend."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib, lda
from montreal_forced_aligner_amd.stats import LdaStats, lda_statistics_host
from tests import lda_case, lda_ref

ROOT = Path(__file__).resolve().parents[1]


def host(case, **kw):
    return lda_statistics_host(case.mfcc, case.frame_off, case.utt2spk, case.cmvn, case.ali, case.tables, case.ctx,
                               num_classes=case.n_classes, **kw)


def assert_same_bits(a: LdaStats, b: LdaStats, what=""):
    assert a.zero.tobytes() == b.zero.tobytes(), what
    assert np.array_equal(a.first, b.first), what
    assert np.array_equal(a.second, b.second), what


def assert_within_bound(got: LdaStats, case, what="", **kw):
    ref, abs2, abs1, n = lda_ref.statistics(case, want_abs=True, **kw)
    assert n > 0, what
    assert np.array_equal(got.zero, ref.zero), what                     # weights are short dyadic numbers: exact
    assert np.all(np.abs(got.second - ref.second) <= lda_ref.bound(n, abs2)), what
    assert np.all(np.abs(got.first - ref.first) <= lda_ref.bound(n, abs1)), what
    assert np.array_equal(got.second, got.second.T), what
    return ref


@pytest.mark.parametrize("dim,ctx", [(13, 3), (5, 1), (16, 3), (13, 0), (8, 7), (128, 0)])
def test_twin_exact_on_integers(dim, ctx):
    rng = np.random.default_rng(100 * dim + ctx)
    case = lda_ref.integer_case(rng, dim, ctx, [1, 2, max(ctx, 1), ctx + 1, 0, 57, 130], 3)
    got, ref = host(case), lda_ref.statistics(case)
    assert ref.zero.sum() > 0
    assert_same_bits(got, ref, f"dim {dim} ctx {ctx}")


def test_twin_on_real_features_within_the_derived_bound():
    case = lda_ref.real_case(np.random.default_rng(7), 13, 3, [300, 1, 211, 2, 450, 3, 4], 11)
    assert_within_bound(host(case), case)
    # without CMVN: another spliced vector
    import dataclasses
    plain = dataclasses.replace(case, utt2spk=None, cmvn=None)
    ref = assert_within_bound(host(plain), plain)
    assert not np.allclose(ref.second, lda_ref.statistics(case).second)


def test_frames_that_take_no_part_leave_no_trace():
    rng = np.random.default_rng(5)
    case = lda_ref.integer_case(rng, 13, 3, [40, 60, 50], 4)
    n_tids = len(case.tid2class)
    case.tid2class[5] = 4          # a class outside [0, C)
    case.tid2class[6] = -1
    start = LdaStats(rng.normal(size=4), rng.normal(size=(4, 91)), np.zeros((91, 91)))
    sym = rng.normal(size=(91, 91))
    start.second = sym + sym.T
    case.ali[:] = np.concatenate([np.zeros(30), np.full(30, n_tids), np.full(30, -3), np.full(20, 5), np.full(20, 6),
                                  np.full(20, 1)]).astype(np.int32)      # id 1 has weight 0
    counts = np.arange(n_tids, dtype=np.int64)
    got = host(case, into=start.copy(), tid_count=counts)
    assert_same_bits(got, start)
    assert np.array_equal(counts, np.arange(n_tids))
    # and frames that do take part are counted
    case.ali[:10] = 3
    host(case, tid_count=counts)
    assert counts[3] == 3 + 10 and counts.sum() == np.arange(n_tids).sum() + 10


def test_prune_share_weight_and_batch_cuts():
    rng = np.random.default_rng(11)
    lengths = [20000 // 8] * 8
    case = lda_ref.integer_case(rng, 2, 1, lengths, 3)
    case.tid_weight[1:] = 1.0
    keys = np.arange(8, dtype=np.uint32) + 40
    got = host(case, rand_prune=4.0, utt_keys=keys, seed=9)
    kept = got.zero.sum() / 4.0
    n, p = 20000, 0.25
    assert kept == round(kept)                                            # the kept frames weigh 4
    assert abs(kept - n * p) <= 4 * np.sqrt(n * p * (1 - p)), kept
    assert_same_bits(got, lda_ref.statistics(case, rand_prune=4.0, utt_keys=keys, seed=9))
    assert not np.array_equal(got.zero, host(case, rand_prune=4.0, utt_keys=keys, seed=10).zero)
    # the same utterances cut into three batches: the same kept set (integers: the sums are exact)
    cut = LdaStats.zeros(3, case.S)
    for a, b in ((0, 3), (3, 4), (4, 8)):
        fa, fb = int(case.frame_off[a]), int(case.frame_off[b])
        lda_statistics_host(case.mfcc[fa:fb], case.frame_off[a:b + 1] - fa, None, None, case.ali[fa:fb], case.tables, case.ctx,
                            num_classes=3, rand_prune=4.0, utt_keys=keys[a:b], seed=9, into=cut)
    assert_same_bits(got, cut)
    # weights at or above theta are left alone
    case.tid_weight[1:] = 4.0
    assert host(case, rand_prune=4.0, utt_keys=keys, seed=9).zero.sum() == 4.0 * 20000


# ---- the estimate --------------------------------------------------------------------------------------------------------------
def test_estimate_identities_on_the_corpus():
    """Measured here on the 48-utterance corpus (9 982 frames, 198 classes, S = 91): the brute-force restatement's own
    residuals are 1.0e-14 (full·within·fullᵀ − I) and 8.8e-16 (off-diagonal of full·between·fullᵀ over its largest entry) in
    float64 — it whitens by an eigendecomposition, not by Cholesky.  The result is cast to float32 (relative 2⁻²⁴ per entry of
    full, entering each identity twice over S terms), which no float64 residual can bound: the tolerance is 64 × the cast's
    own effect, measured the same way on the restatement's matrix cast to float32 (6.1e-8 and 3.3e-8 here; ``estimate_lda``'s
    float32 result measures the same 6.1e-8 and 3.3e-8, the projected spectrum 13.36 … 0.0306 at row 40, the smallest
    relative gap among the first 41 eigenvalues 0.44 %)."""
    st = lda_case.generator_stats()
    case = lda_case.generator_case()
    assert st.first.shape == (case.n_classes, 91) and st.zero.sum() > 5000
    print("frames", st.zero.sum(), "classes", case.n_classes, "with frames", int((st.zero > 0).sum()))
    _N, _m, within, between = lda_ref.scatter(st)
    ref_full, ref_s = lda_ref.estimate(st)
    r64 = lda_ref.identity_residuals(ref_full, within, between)
    r32 = lda_ref.identity_residuals(ref_full.astype(np.float32), within, between)
    print("restatement residuals float64", r64[:2], "cast to float32", r32[:2])
    assert r64[0] < 1e-12 and r64[1] < 1e-12
    mat, full = lda.estimate_lda(st, dim=40)
    assert mat.dtype == np.float32 and mat.shape == (40, 91) and full.shape == (91, 91)
    assert np.array_equal(mat, full[:40])
    got = lda_ref.identity_residuals(full, within, between)
    print("estimate_lda residuals", got[:2], "spectrum", got[2][0], got[2][39], got[2][-1])
    assert got[0] <= 64 * r32[0] and got[1] <= 64 * r32[1]
    d = got[2]
    assert np.all(np.diff(d) <= 64 * r32[1] * d[0])                       # s descending
    assert np.allclose(d, ref_s, rtol=0, atol=64 * r32[1] * d[0])
    # against the restatement: the first 41 eigenvalues are apart (smallest relative gap 0.4 %), so the rows are determined
    # up to the perturbation (residual / gap)
    gap = np.min((ref_s[:40] - ref_s[1:41]) / ref_s[:40])
    print("smallest relative gap among the first 41", gap)
    assert gap > 1e-4
    cos = np.abs(np.sum(mat.astype(np.float64) @ within * ref_full[:40], axis=1))      # rows are within-orthonormal
    assert np.all(cos > 1 - 1e-6), cos.min()
    assert np.all(np.sign(mat[np.arange(40), np.abs(mat).argmax(axis=1)]) > 0)
    # with the offset column: −full·m
    mat_o, full_o = lda.estimate_lda(st, dim=40, remove_offset=True)
    m = st.first.sum(axis=0) / st.zero.sum()
    assert mat_o.shape == (40, 92) and np.array_equal(full_o[:, :91], full)
    assert np.allclose(full_o[:, 91], -(full.astype(np.float64) @ m), rtol=1e-5, atol=1e-5)


def test_known_answer_two_classes():
    rng = np.random.default_rng(3)
    S = 6
    A = rng.normal(size=(S, S))
    cov = A @ A.T + S * np.eye(S)
    d = rng.normal(size=S)
    n = 25000.0                                                            # per class: exact moments fed as statistics
    st = LdaStats(np.array([n, n]), np.stack([n * d, -n * d]), 2 * n * (cov + np.outer(d, d)))
    mat, _full = lda.estimate_lda(st, dim=1)
    want = np.linalg.solve(cov, d)
    row = mat[0].astype(np.float64)
    cos = abs(row @ want) / np.linalg.norm(row) / np.linalg.norm(want)
    assert cos > 1 - 1e-9, cos


def test_estimate_refusals():
    st = lda_case.generator_stats()
    with pytest.raises(ValueError, match="no frames"):
        lda.estimate_lda(LdaStats.zeros(3, 5), dim=2)
    for dim in (0, 92):
        with pytest.raises(ValueError, match="outside 1..91"):
            lda.estimate_lda(st, dim=dim)
    rng = np.random.default_rng(1)
    x = rng.normal(size=(400, 4))
    cls = rng.integers(0, 3, size=400)

    def stats_of(x, cls, C=3):
        s = LdaStats.zeros(C, x.shape[1])
        np.add.at(s.zero, cls, 1.0)
        np.add.at(s.first, cls, x)
        s.second = x.T @ x
        return s

    with pytest.raises(ValueError, match="between-class rank 2"):
        lda.estimate_lda(stats_of(x, cls), dim=3)
    mat, _ = lda.estimate_lda(stats_of(x, cls), dim=3, allow_large_dim=True)
    assert mat.shape == (3, 4)
    flat = x.copy()
    flat[:, 2] = 1.5                                                       # a constant column
    with pytest.raises(ValueError, match="not positive definite"):
        lda.estimate_lda(stats_of(flat, cls), dim=2)
    dep = x.copy()
    dep[:, 3] = dep[:, 0] - 2 * dep[:, 1]                                  # a dependent column
    with pytest.raises(ValueError, match="not positive definite"):
        lda.estimate_lda(stats_of(dep, cls), dim=2)
    with pytest.raises(ValueError, match="not positive definite"):        # fewer frames than dimensions
        lda.estimate_lda(stats_of(x[:3], np.array([0, 1, 2])), dim=1)


def test_twin_refusals():
    case = lda_ref.integer_case(np.random.default_rng(2), 43, 1, [5], 2)    # S = 129
    with pytest.raises(_lib.MfaHipError, match="128"):
        host(case)
    lib = _lib.lib()
    assert lib.mfa_lda_acc_max_dim() == 128 and lib.mfa_lda_acc_slab_frames() >= 64 and lib.mfa_lda_acc_chunk_frames() >= 64
    ok = lda_ref.integer_case(np.random.default_rng(2), 4, 1, [5], 2)
    with pytest.raises(ValueError, match="utt_keys"):
        host(ok, rand_prune=4.0)
    with pytest.raises(ValueError, match="into"):
        host(ok, into=LdaStats.zeros(2, 11))


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "lda_acc_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "lda_acc_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "lda_acc_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout


# ---- the trainer on the host backend -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lda_run():
    from montreal_forced_aligner_amd.train import LdaTrainer, MonophoneTrainer
    from tests import train_mono_case as TC

    corpus = TC.train_corpus()
    mono_backend = TC.HostBackend(corpus)
    mono = MonophoneTrainer(lexicon=corpus.world.lexicon, topology=TC.topology(), backend=mono_backend,
                            silence_phones=TC.silence_ids(), num_iterations=6, max_gaussians=208)
    mono_backend.equal_align(mono.raw_tm, mono.raw_am, mono.tree, mono.seed)
    equal_share = TC.phone_share(corpus, mono.raw_tm, mono_backend.alignments())
    mono.train()
    mono_share = TC.phone_share(corpus, mono.raw_tm, TC.host_align(corpus, mono.raw_tm, mono.raw_am, mono.tree, mono.opt))
    backend = lda_case.LdaHostBackend(corpus)
    tr = LdaTrainer(lexicon=corpus.world.lexicon, previous=(mono.raw_tm, mono.raw_am, mono.tree), backend=backend,
                    silence_phones=TC.silence_ids(), num_iterations=8, max_gaussians=208).train()
    return corpus, mono, tr, backend, equal_share, mono_share


def check_lda_training(corpus, mono, tr, final_alignments, equal_share, mono_share):
    """What the host and the device runs of the 8-iteration stage are both held to."""
    from tests import train_mono_case as TC

    h = tr.history
    assert [e["iteration"] for e in h] == list(range(9))
    # the 8-iteration schedule: no realignment after iteration 0 (every tenth), final_gaussian_iteration = −2 so no mix-up.
    # em_violations checks iteration i when its predecessor neither realigned nor mixed up, or when i did not realign and its
    # predecessor did not mix up: here the second clause holds for every i ≥ 1
    assert tr.realignment_iterations == [] and tr.final_gaussian_iteration == -2 and tr.gaussian_increment == 0
    assert [e["realigned"] for e in h] == [True] + [False] * 8 and not any(e["mixed_up"] for e in h)
    checked, bad = TC.em_violations(h)
    print("checked", checked, [(e["iteration"], round(e["loglike"], 4)) for e in h])
    assert checked == list(range(1, 9)) and checked
    assert bad == []
    # dimension 40, the tree it was given, as many pdfs
    assert tr.raw_am.dim == 40 and tr.lda_mat.shape == (40, 91) and tr.lda_mat.dtype == np.float32
    assert tr.tree is mono.tree and tr.raw_am.num_pdfs == mono.raw_am.num_pdfs == 208
    assert tr.lda_stats.first.shape == (208, 91) and tr.initial_stats.occ.shape == (208,)
    share = TC.phone_share(corpus, tr.raw_tm, final_alignments)
    print(f"frames on the generator's phone: equal alignments {equal_share:.4f}, monophone (6 iterations) {mono_share:.4f}, "
          f"LDA stage (8 iterations) {share:.4f}")
    assert share > equal_share


def test_lda_trainer_on_the_host_backend(lda_run):
    corpus, mono, tr, backend, equal_share, mono_share = lda_run
    backend.align(tr.raw_tm, tr.raw_am, tr.tree, tr.opt.beam)
    check_lda_training(corpus, mono, tr, backend.alignments(), equal_share, mono_share)


def test_lda_trainer_options_and_refusals(lda_run, tmp_path):
    from montreal_forced_aligner_amd import kaldi_io
    from montreal_forced_aligner_amd.train import LdaTrainer

    corpus, mono, tr, backend, _e, _m = lda_run
    prev = (mono.raw_tm, mono.raw_am, mono.tree)
    full = LdaTrainer(lexicon=corpus.world.lexicon, previous=prev, backend=backend)
    assert (full.num_iterations, full.max_gaussians, full.power, full.lda_dimension, full.splice_context) == (35, 15000, 0.25, 40, 3)
    assert full.realignment_iterations == [10, 20, 30] and full.final_gaussian_iteration == 25
    assert full.initial_gaussians == 208 and full.gaussian_increment == int((15000 - 208) / 25)
    assert full.random_prune == 0.0 and full.opt.boost_silence == 1.0
    with pytest.raises(ValueError, match="lda_dimension 49"):
        LdaTrainer(lexicon=corpus.world.lexicon, previous=prev, backend=backend, lda_dimension=49)
    with pytest.raises(ValueError, match="spliced dimension of 143"):
        LdaTrainer(lexicon=corpus.world.lexicon, previous=prev, backend=backend, splice_context=5)
    with pytest.raises(ValueError, match="previous"):
        LdaTrainer(lexicon=corpus.world.lexicon, backend=backend)
    paths = tr.write(tmp_path / "lda")
    assert [p.name for p in paths] == ["final.mdl", "tree", "lda.mat"]
    assert np.array_equal(kaldi_io.read_matrix_file(paths[2].read_bytes()), tr.lda_mat)
    raw_tm, raw_am = kaldi_io.read_model(paths[0].read_bytes())
    assert raw_am.dim == 40 and raw_am.num_pdfs == 208
