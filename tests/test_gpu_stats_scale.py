"""The training statistics on the device (csrc/gmm_acc.hip, mllt_acc.hip, lda_acc.hip, tree_acc.hip, tid_lookup.hpp) at real
key counts and long segments: the cases of tests/stats_scale_cases.py, which tests/test_stats_scale_cpu.py runs through the
host twins.  The neighbours (test_gpu_gmm_acc.py, test_gpu_mllt_acc.py, test_gpu_lda_acc.py, test_gpu_tree_acc.py) stay below
40 pdfs, 300 classes, 9 phones and four units a key; here are hundreds and thousands of keys, keys of 8, 9, 10 and 17 units,
sort widths on either side of a radix digit, alignment-shaped frame orders and more events and units than the tree kernels
have wavefronts.

Every case is on an exact tier (integers or a dyadic grid), so the device is held to the numpy expectation and to the host
twin bit for bit: occ, mean and variance sums, full (both triangles), first and second moments, the counts, keys, sums and
``frame_event``.  Each test asserts from the reference's own counts that its case reaches its path (the helpers of
tests/test_stats_scale_cpu.py, whose docstring lists the paths) and prints the frame, key and unit counts.  Last, one
real-valued long segment per kernel (9 units on one key) under the existing derived bounds, unchanged."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd.stats import (gmm_statistics, gmm_statistics_host, lda_statistics, lda_statistics_host,
                                               mllt_statistics, mllt_statistics_host, tree_key, tree_statistics)
from tests import gmm_acc_ref as R
from tests import lda_ref
from tests import mllt_ref as MR
from tests import stats_scale_cases as S
from tests import test_stats_scale_cpu as C
from tests import tree_ref as TR
from tests.test_gmm_acc_cpu import check_against_float64
from tests.test_lda_cpu import assert_within_bound

pytestmark = pytest.mark.gpu


def _dev(e, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _constants_are_the_librarys(engine):
    lib = engine.lib
    assert (C.CG, C.CM) == (int(lib.mfa_gmm_acc_chunk_frames()), int(lib.mfa_mllt_acc_chunk_frames()))
    assert (C.LDA_CHUNK, C.LDA_SLAB, C.TREE_CHUNK) == (int(lib.mfa_lda_acc_chunk_frames()), int(lib.mfa_lda_acc_slab_frames()),
                                                       int(lib.mfa_tree_acc_chunk_frames()))


def _cus(engine):
    return int(torch.cuda.get_device_properties(engine.device).multi_processor_count)


# ---- GMM and MLLT statistics ----------------------------------------------------------------------------------------------------
def gmm_dev(engine, case, load=True):
    if load:
        engine.load_gmm(case.am)
    return gmm_statistics(engine, _dev(engine, case.feats), _dev(engine, case.ali), case.tm, case.weights)


def mllt_dev(engine, case, load=True):
    if load:
        engine.load_gmm(case.am)
    return mllt_statistics(engine, _dev(engine, case.feats), _dev(engine, case.ali), case.tm, case.weights)


def gmm_bits(st, tot_like=True):
    tot = [st.tot_like, st.tot_count] if tot_like else [st.tot_count]
    return b"".join(np.asarray(a).tobytes() for a in (st.occ, st.mean_acc, st.var_acc, tot, st.tid_count))


def mllt_bits(st, tot_like=True):
    tot = [st.tot_like, st.tot_count] if tot_like else [st.tot_count]
    return st.occ.tobytes() + st.full.tobytes() + np.array(tot).tobytes()


def gmm_and_mllt_are_exact(engine, case, expect, expect_full):
    """Device GMM and MLLT statistics of ``case`` against the numpy expectation and the host twins, bit for bit; MLLT occ and
    totals against the GMM statistics' bits; a second run against the first.  tot_like is a sum of real numbers: the two
    device calls and the two runs agree on it; the twin sums it in another order, so it is not compared here."""
    occ, mean, var, tid_count, tot_count = expect
    g = gmm_dev(engine, case)
    assert g.occ.tobytes() == occ.tobytes() and g.mean_acc.tobytes() == mean.tobytes() and g.var_acc.tobytes() == var.tobytes(), case.name
    assert np.array_equal(g.tid_count, tid_count) and g.tot_count == tot_count, case.name
    pdf, _fw = R.frame_tables(case.tm, case.ali, case.weights)
    assert np.array_equal(g.tid_count, np.bincount(case.ali[pdf >= 0], minlength=len(case.weights))), case.name
    m = mllt_dev(engine, case, load=False)
    assert m.occ.tobytes() == occ.tobytes() and m.full.tobytes() == expect_full.tobytes(), case.name
    assert np.array_equal(m.full, np.swapaxes(m.full, 1, 2)), case.name
    assert (m.tot_like, m.tot_count) == (g.tot_like, g.tot_count), case.name
    gt = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    mt = mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    assert gmm_bits(g, tot_like=False) == gmm_bits(gt, tot_like=False) and mllt_bits(m, tot_like=False) == mllt_bits(mt, tot_like=False), case.name
    assert np.isfinite(g.tot_like), case.name
    assert gmm_bits(gmm_dev(engine, case, load=False)) == gmm_bits(g) and mllt_bits(mllt_dev(engine, case, load=False)) == mllt_bits(m), case.name
    return g, m


@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("name,dim,counts,want", C.KEY_CASES, ids=C.KEY_IDS)
def test_integer_pdfs_at_real_key_counts(engine, name, dim, counts, want, order):
    _constants_are_the_librarys(engine)
    case = S.integer_case(dim, counts, order)
    print(C.reaches_its_path(name, case, counts, want, order))
    expect = S.gmm_expect(case)
    mocc, full = MR.integer_expect(case)
    assert mocc.tobytes() == expect[0].tobytes()
    gmm_and_mllt_are_exact(engine, case, expect, full)


def test_mixed_mixtures_at_many_pdfs(engine):
    """Dim 13 (tests/test_stats_scale_cpu.py says why).  The twins' posteriors are asserted exactly one-hot on every frame."""
    _constants_are_the_librarys(engine)
    case, gauss, _g, _m = C.mixed_twin()
    print(C.mixed_reaches_its_path(case))
    mocc, full = MR.one_hot_expect(case, gauss)
    expect = S.gmm_expect(case, gauss)
    assert mocc.tobytes() == expect[0].tobytes()
    gmm_and_mllt_are_exact(engine, case, expect, full)


def test_a_smaller_call_after_a_larger_one_gives_its_own_result(engine):
    """The workspace is the context's and only grows: the calls at 255 pdfs run in what the calls at 4 960 pdfs (and the
    mixed mixtures' 14 104 Gaussians) left behind, with another model loaded in between."""
    by_name = {c[0]: c for c in C.KEY_CASES}
    for name, order in (("P=4960", "aligned"), ("P=255", "shuffled"), ("P=4960 sparse", "shuffled"), ("P=600 dim 48 occupied 257", "aligned"),
                        ("P=256", "aligned")):
        _n, dim, counts, want = by_name[name]
        case = S.integer_case(dim, counts, order)
        print(C.reaches_its_path(name, case, counts, want, order))
        gmm_and_mllt_are_exact(engine, case, S.gmm_expect(case), MR.integer_expect(case)[1])


# ---- LDA statistics -------------------------------------------------------------------------------------------------------------
def lda_dev(engine, case, **kw):
    return lda_statistics(engine, _dev(engine, case.mfcc), case.frame_off, case.utt2spk, _dev(engine, case.cmvn), _dev(engine, case.ali),
                          case.tables, case.ctx, num_classes=case.n_classes, **kw)


def lda_host(case, **kw):
    return lda_statistics_host(case.mfcc, case.frame_off, case.utt2spk, case.cmvn, case.ali, case.tables, case.ctx,
                               num_classes=case.n_classes, **kw)


def lda_bits(st):
    return st.zero.tobytes() + st.first.tobytes() + st.second.tobytes()


def lda_is_exact(engine, case):
    n_tids = len(case.tid2class)
    c_dev, c_host = np.zeros(n_tids, np.int64), np.zeros(n_tids, np.int64)
    got, twin, ref = lda_dev(engine, case, tid_count=c_dev), lda_host(case, tid_count=c_host), lda_ref.statistics(case)
    assert lda_bits(got) == lda_bits(twin) == lda_bits(ref)
    assert np.array_equal(got.second, got.second.T)
    cls, _w = lda_ref.frame_tables(case)
    assert np.array_equal(c_dev, c_host) and np.array_equal(c_dev, np.bincount(case.ali[cls >= 0], minlength=n_tids))
    assert lda_bits(lda_dev(engine, case)) == lda_bits(got)


@pytest.mark.parametrize("name,args,want", C.LDA_CASES, ids=C.LDA_IDS)
def test_lda_at_many_classes_and_slabs(engine, name, args, want):
    _constants_are_the_librarys(engine)
    case = S.lda_case(*args)
    print(C.lda_reaches_its_path(name, case, want))
    lda_is_exact(engine, case)


def test_lda_smaller_call_after_a_larger_one(engine):
    for name, args, want in (C.LDA_CASES[2], C.LDA_CASES[3], C.LDA_CASES[1], C.LDA_CASES[5]):
        case = S.lda_case(*args)
        print(C.lda_reaches_its_path(name, case, want))
        lda_is_exact(engine, case)


# ---- tree statistics ------------------------------------------------------------------------------------------------------------
def tree_dev(engine, case, **kw):
    st, fe, skipped = tree_statistics(engine, _dev(engine, case.feats), case.frame_off, _dev(engine, case.ali), case.tm, case.ci, **kw)
    return st, fe.cpu().numpy(), skipped


def tree_bits(got):
    st, fe, skipped = got
    return st.keys.tobytes() + st.count.tobytes() + st.sum.tobytes() + st.sumsq.tobytes() + fe.tobytes() + bytes([skipped])


def tree_is_exact(engine, case):
    """Device against the restatement and the twin, outright; a second run against the first."""
    got = tree_dev(engine, case)
    st = C.tree_equal_to_ref(case, got)
    assert tree_bits(got) == tree_bits(C.tree_host(case))
    assert tree_bits(tree_dev(engine, case)) == tree_bits(got)
    return st, got[1]


def test_tree_on_sparse_phone_ids(engine):
    """n_phones = 65 535, the largest the key holds, is accepted (65 536 is refused: tests/test_gpu_tree_acc.py)."""
    case = S.tree_sparse_case()
    st, _fe = tree_is_exact(engine, case)
    print(C.tree_line("sparse phone ids", case, st))
    assert int(max(case.tm.topo.phones)) == 65535 and st.keys[-1] == tree_key(65535, 65535, 65535, 0)
    W = st.windows()
    assert (W[:, 0] >= 1 << 15).any() and (W[:, 2] >= 1 << 15).any() and set(S.SPARSE_CI) <= set(W[:, 1].tolist())


@pytest.mark.parametrize("n_phones", S.PHONE_COUNTS)
def test_tree_at_every_key_width(engine, n_phones):
    case = S.tree_phone_count_case(n_phones)
    assert int(max(case.tm.topo.phones)) == n_phones
    st, _fe = tree_is_exact(engine, case)
    print(C.tree_line(f"n_phones {n_phones}", case, st))
    W = st.windows()
    assert (W[:, 0] == n_phones).any() and (W[:, 1] == n_phones).any() and (W[:, 2] == n_phones).any()


def test_tree_on_pdf_classes_up_to_255(engine):
    case = S.tree_pdf_class_case()
    st, _fe = tree_is_exact(engine, case)
    print(C.tree_line("pdf-classes 0, 254, 255", case, st))
    assert set(st.pdf_classes().tolist()) == {0, 254, 255}


@pytest.mark.parametrize("dim", (13, 48))
def test_tree_on_long_events(engine, dim):
    _constants_are_the_librarys(engine)
    case = S.tree_long_event_case(C.TREE_CHUNK, dim)
    st, _fe = tree_is_exact(engine, case)
    print(C.tree_line(f"long events dim {dim}", case, st))
    assert sorted(S.units(st.count, C.TREE_CHUNK).tolist())[-2:] == [9, 17]
    assert {8 * C.TREE_CHUNK + 1, 17 * C.TREE_CHUNK} <= set(st.count.tolist())


def test_tree_on_events_at_the_reductions_step(engine):
    """Events of 8, 9 and 10 chunks: tree_big_reduce_kernel adds 7, 8 and 9 partials to the first (eight a step, then the rest)."""
    _constants_are_the_librarys(engine)
    case = S.tree_step_event_case(C.TREE_CHUNK)
    st, _fe = tree_is_exact(engine, case)
    print(C.tree_line("events of 8, 9, 10 chunks", case, st))
    assert sorted(S.units(st.count, C.TREE_CHUNK).tolist())[-3:] == [8, 9, 10]


def test_tree_with_more_events_than_wavefronts(engine):
    cus = _cus(engine)
    k = S.small_event_phones(cus)
    case = S.tree_every_frame_case(k)
    st, fe = tree_is_exact(engine, case)
    print(C.tree_line(f"de Bruijn over {k} phones on {cus} CUs", case, st))
    assert (k - 1) ** 3 <= 32 * cus < k ** 3 == st.num_events == len(case.ali) and np.all(st.count == 1)
    assert sorted(fe.tolist()) == list(range(len(case.ali)))


def test_tree_with_more_units_of_one_event_than_wavefronts(engine):
    _constants_are_the_librarys(engine)
    cus = _cus(engine)
    case = S.tree_one_event_case(C.TREE_CHUNK, cus)
    T = int(case.frame_off[-1])
    assert len(case.frame_off) == 9 and T > C.TREE_CHUNK * 32 * cus and case.feats.shape == (T, 1)
    got = st, fe, skipped = tree_dev(engine, case)
    print(C.tree_line(f"one event on {cus} CUs", case, st))
    n, s, q = C.one_event_expect(case)
    assert skipped == 0 and st.keys.tolist() == [int(tree_key(0, 3, 0, 0))] and st.count.tolist() == [n] == [T]
    assert st.sum.tolist() == [[s]] and st.sumsq.tolist() == [[q]] and not fe.any()
    assert S.units(st.count, C.TREE_CHUNK)[0] > 32 * cus
    assert tree_bits(got) == tree_bits(C.tree_host(case)) == tree_bits(tree_dev(engine, case))
    # and a small call in the workspace this one left behind
    small = S.tree_phone_count_case(15)
    tree_is_exact(engine, small)


# ---- real features: one long segment per kernel, under the existing bounds --------------------------------------------------------
def test_gmm_soft_posteriors_on_a_long_pdf(engine):
    case = S.soft_long_case(13, 8 * C.CG + 1)
    counts = S.frame_counts(case)
    assert S.units(counts, C.CG)[0] == 9
    print(f"{case.name}: {len(case.ali)} frames, {len(counts)} pdfs, longest {int(S.units(counts, C.CG).max())} GMM units")
    st = gmm_dev(engine, case)
    check_against_float64(case, st, f"device, {case.name}")
    check_against_float64(case, gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights), f"host twin, {case.name}")
    assert gmm_bits(gmm_dev(engine, case, load=False)) == gmm_bits(st)


def test_mllt_soft_posteriors_on_a_long_pdf(engine):
    case = S.soft_long_case(13, 8 * C.CM + 1)
    counts = S.frame_counts(case)
    assert S.units(counts, C.CM)[0] == 9
    print(f"{case.name}: {len(case.ali)} frames, {len(counts)} pdfs, longest {int(S.units(counts, C.CM).max())} MLLT units, "
          f"{int(S.units(counts, C.CG).sum())} sub-units")
    st = mllt_dev(engine, case)
    MR.check_against_float64(case, st, f"device, {case.name}")
    MR.check_against_float64(case, mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights), f"host twin, {case.name}")
    g = gmm_dev(engine, case, load=False)
    assert st.occ.tobytes() == g.occ.tobytes() and (st.tot_like, st.tot_count) == (g.tot_like, g.tot_count)
    assert mllt_bits(mllt_dev(engine, case, load=False)) == mllt_bits(st)


def test_lda_real_features_on_long_classes_and_many_slabs(engine):
    case = lda_ref.real_case(np.random.default_rng(41), 13, 3, [8 * C.LDA_SLAB + 1 - 4000, 4000], 2)
    counts = S.lda_counts(case)
    T = int(case.frame_off[-1])
    assert S.units(counts, C.LDA_CHUNK).max() >= 9 and -(-T // C.LDA_SLAB) == 9
    print(f"LDA real: {T} frames in 9 slabs, 2 classes, longest {int(S.units(counts, C.LDA_CHUNK).max())} units")
    got = lda_dev(engine, case)
    assert_within_bound(got, case, "device")
    twin = lda_host(case)
    assert_within_bound(twin, case, "host twin")
    _st, abs2, abs1, n = lda_ref.statistics(case, want_abs=True)
    assert np.all(np.abs(got.second - twin.second) <= lda_ref.bound(n, abs2)) and np.all(np.abs(got.first - twin.first) <= lda_ref.bound(n, abs1))
    assert lda_bits(lda_dev(engine, case)) == lda_bits(got)


def test_tree_real_features_on_long_events(engine):
    case = S.tree_long_event_case(C.TREE_CHUNK, 13, integer=False)
    got = st, fe, skipped = tree_dev(engine, case)
    print(C.tree_line("long events, real features", case, st))
    keys, count, s, q, rfe, rskipped, a1, a2 = TR.accumulate(case, want_abs=True)
    assert sorted(S.units(count, C.TREE_CHUNK).tolist())[-2:] == [9, 17]
    assert np.array_equal(st.keys, keys) and np.array_equal(st.count, count) and np.array_equal(fe, rfe) and skipped == rskipped == 0
    for stats in (st, C.tree_host(case)[0]):
        assert np.all(np.abs(stats.sum - s) <= TR.bound(count, a1)) and np.all(np.abs(stats.sumsq - q) <= TR.bound(count, a2))
    assert tree_bits(tree_dev(engine, case)) == tree_bits(got)
