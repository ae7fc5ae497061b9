"""The training statistics' host twins at real key counts and long segments (tests/stats_scale_cases.py), bit for bit against
the numpy restatements: this validates the cases and the references without a device and pins the twins at these sizes;
tests/test_gpu_stats_scale.py holds the device to both.  Every test first asserts, from the reference's own per-key counts,
that its case reaches the device path it is there for, and prints the counts:

  8-wide body of the chunk-order reductions      a key of 8 units (no remainder), of 9 / 10 (remainder after it), of 17
  scans with several keys a thread               P = 257 … 513 (per = 2, 3), 4 960 (per = 20); 600 classes (per = 3)
  second trip of the totals loop                 more than 256 units in a call; exactly 256 and 257
  sort width                                     P or C of 255, 256, 257, 511, 512, 513: end_bit 8, 9, 10 with the key P itself
  tree key widths                                n_phones 15 / 16, 255 / 256, 4 095 / 4 096, 65 535; pdf-classes 0, 254, 255
  event and unit strides of the tree kernels     more events, and more units of one event, than 32 · CUs wavefronts (the CPU
                                                 tests take 256 CUs)
  run compression of the lookups                 the aligned order of every key-count case and of two LDA cases
  far fewer frames than keys                     300 frames over 4 960 pdfs"""
import time

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd.stats import (gmm_statistics_host, lda_statistics_host, mllt_statistics_host, tree_key,
                                               tree_statistics_host)
from tests import gmm_acc_ref as R
from tests import lda_ref
from tests import mllt_ref as MR
from tests import stats_scale_cases as S
from tests import tree_ref as TR

L = _lib.lib()
CG, CM = int(L.mfa_gmm_acc_chunk_frames()), int(L.mfa_mllt_acc_chunk_frames())
LDA_CHUNK, LDA_SLAB = int(L.mfa_lda_acc_chunk_frames()), int(L.mfa_lda_acc_slab_frames())
TREE_CHUNK = int(L.mfa_tree_acc_chunk_frames())
CUS = 256                                     # the stand-in for the device's compute units


# ---- GMM and MLLT statistics ----------------------------------------------------------------------------------------------------
def key_count_cases():
    """(name, dim, frames per pdf, what the case must reach) of every integer case; shared with the device tests."""
    out = []
    for P in S.KEY_COUNTS:
        out.append((f"P={P}", 13, S.key_count_frames(P, CG, CM), dict(gmm_units=(1, 10), mllt_units=(1, 2, 8), min_units=257 if P >= 511 else 0)))
    out.append(("P=257 long last", 13, S.key_count_frames(257, CG, CM, last=9 * CM + 1), dict(gmm_units=(10,), mllt_units=(10,))))
    out.append(("P=6 at the reduction step", 13, S.step_frames(CG, CM), dict(gmm_step=(7, 8, 9), mllt_step=(7,))))
    out.append(("P=4960 sparse", 13, S.sparse_frames(4960), dict(sparse=True)))
    for dim in (40, 48):
        for occupied in (256, 257, 400):
            out.append((f"P=600 dim {dim} occupied {occupied}", dim, S.occupied_frames(600, occupied), dict(exact_units=occupied)))
    return [(name, dim, tuple(int(c) for c in counts), want) for name, dim, counts, want in out]


KEY_CASES = key_count_cases()
KEY_IDS = [c[0].replace(" ", "-") for c in KEY_CASES]


def reaches_its_path(name, case, counts, want, order):
    """The path conditions of a key-count case, from the contract's frame tables; returns the line the tests print."""
    got = S.frame_counts(case)
    assert np.array_equal(got, counts), name
    P, T = len(got), len(case.ali)
    ug, um = S.units(got, CG), S.units(got, CM)
    for n in want.get("gmm_units", ()):
        assert n in ug, (name, "GMM units", n)
    for n in want.get("mllt_units", ()):
        assert n in um, (name, "MLLT units", n)
    for n in want.get("gmm_step", ()):
        assert n in ug, (name, "GMM units", n)
    for n in want.get("mllt_step", ()):
        assert n in um, (name, "MLLT units", n)
    if "gmm_units" in want:
        assert ug.max() >= 8 and um.max() >= 8 and got[0] == 9 * CG + 1 and CG in got, name
    assert int(ug.sum()) >= want.get("min_units", 0), name
    if "exact_units" in want:
        assert int(ug.sum()) == want["exact_units"] == int(np.count_nonzero(got)), name
    if want.get("sparse"):
        assert T <= P // 16 + 2 and got[0] > 0 and got[-1] > 0 and np.count_nonzero(got) < P // 16, name
    shape = S.run_shape(case)
    if order == "shuffled":
        assert shape["longest"] < 63, (name, shape)                # a permutation: short runs, by chance only
    else:
        assert shape["runs"] < T or T < 400, name
        if got.max() >= 1000:
            assert shape["lengths"] >= set(S.RUN_LENGTHS), (name, shape)
            assert all(shape[k] for k in ("starts_at_lane_63", "crosses_a_block", "cut_by_id_0", "cut_by_weight_0", "ends_inside_a_run")), (name, shape)
    return (f"{name} {order}: {T} frames, {P} pdfs (scan: {(P + 255) // 256} a thread, sort: {int(P).bit_length()} bits), "
            f"{int(ug.sum())} GMM units (longest pdf {int(ug.max())}), {int(um.sum())} MLLT units (longest {int(um.max())}), "
            f"{shape['runs']} runs (longest {shape['longest']})")


@pytest.mark.parametrize("order", S.ORDERS)
@pytest.mark.parametrize("name,dim,counts,want", KEY_CASES, ids=KEY_IDS)
def test_twins_on_integer_pdfs_at_real_key_counts(name, dim, counts, want, order):
    case = S.integer_case(dim, counts, order)
    print(reaches_its_path(name, case, counts, want, order))
    occ, mean, var, tid_count, tot_count = S.gmm_expect(case)
    g = gmm_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    assert g.occ.tobytes() == occ.tobytes() and g.mean_acc.tobytes() == mean.tobytes() and g.var_acc.tobytes() == var.tobytes()
    assert np.array_equal(g.tid_count, tid_count) and g.tot_count == tot_count == float(sum(counts))
    assert np.array_equal(tid_count, np.bincount(case.ali[R.frame_tables(case.tm, case.ali, case.weights)[0] >= 0], minlength=len(case.weights)))
    m = mllt_statistics_host(case.am, case.feats, case.ali, case.tm, case.weights)
    mocc, full = MR.integer_expect(case)
    assert m.occ.tobytes() == mocc.tobytes() == occ.tobytes() and m.full.tobytes() == full.tobytes()
    assert (m.tot_like, m.tot_count) == (g.tot_like, g.tot_count)
    # the aligned order holds the same frames: the shuffled order's sums
    if order == "aligned":
        other = S.gmm_expect(S.integer_case(dim, counts, "shuffled"))
        assert other[0].tobytes() == occ.tobytes() and other[1].tobytes() == mean.tobytes() and other[2].tobytes() == var.tobytes()


def mixed_reaches_its_path(case):
    got = S.frame_counts(case)
    sizes = np.diff(case.am.pdf_offsets)
    um, ug = S.units(got, CM), S.units(got, CG)
    assert len(sizes) >= 300 and set(sizes.tolist()) == set(MR.ONE_HOT_SIZES)
    assert um[sizes == 128].max() == 8 and um[sizes == 5].max() == 9 and ug[sizes == 65].max() == 10
    assert len({int(n) for n in sizes[:7]}) == 7                   # non-uniform Gaussian counts under one thread of the scans
    return (f"mixed mixtures: {len(case.ali)} frames, {len(sizes)} pdfs of {case.am.num_gauss} Gaussians, {int(ug.sum())} GMM units, "
            f"{int(um.sum())} MLLT units (longest pdf {int(um.max())})")


def mixed_twin(dim=13):
    """(case, gauss, GMM twin, MLLT twin) of the mixed case with the twins' posteriors asserted exactly one-hot."""
    case, gauss = S.mixed_case(dim, CG, CM)
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    expect = None
    twins = []
    for fn in (gmm_statistics_host, mllt_statistics_host):
        st, post = fn(case.am, case.feats, case.ali, case.tm, case.weights, want_post=True)
        if expect is None:
            expect = np.zeros_like(post)
            expect[np.arange(len(gauss)), gauss - case.am.pdf_offsets[pdf]] = fw
        assert np.array_equal(post, expect), "host twin: posteriors are not exactly one-hot"
        twins.append(st)
    return case, gauss, twins[0], twins[1]


def test_twins_on_mixed_mixtures_at_many_pdfs():
    """Dim 13: at dim 48 the 14 104 Gaussians' full sums alone are 260 MB a copy."""
    t0 = time.time()
    case, gauss, g, m = mixed_twin()
    print(mixed_reaches_its_path(case), f"(twins {time.time() - t0:.1f} s)")
    occ, mean, var, tid_count, tot_count = S.gmm_expect(case, gauss)
    assert g.occ.tobytes() == occ.tobytes() and g.mean_acc.tobytes() == mean.tobytes() and g.var_acc.tobytes() == var.tobytes()
    assert np.array_equal(g.tid_count, tid_count) and g.tot_count == tot_count
    mocc, full = MR.one_hot_expect(case, gauss)
    assert m.occ.tobytes() == mocc.tobytes() == occ.tobytes() and m.full.tobytes() == full.tobytes()
    assert (m.tot_like, m.tot_count) == (g.tot_like, g.tot_count)


def test_one_hot_case_keeps_its_bits_without_sizes():
    """``sizes`` left out is today's case: the argument changes no existing test."""
    counts = (40, 60, 77, 150, 90, 120, 200)
    a, ga = MR.one_hot_case(13, counts)
    b, gb = MR.one_hot_case(13, counts, tuple(MR.ONE_HOT_SIZES))
    assert a.feats.tobytes() == b.feats.tobytes() and a.ali.tobytes() == b.ali.tobytes() and np.array_equal(ga, gb)
    assert a.am.gconsts.tobytes() == b.am.gconsts.tobytes() and a.weights.tobytes() == b.weights.tobytes()


# ---- LDA statistics -------------------------------------------------------------------------------------------------------------
def lda_cases():
    """(name, builder arguments, what the case must reach); shared with the device tests."""
    out = []
    T = 8 * LDA_SLAB + 1
    long_classes = ((0, 9 * LDA_CHUNK + 1), (599, 8 * LDA_CHUNK))
    for dim, order in ((13, "shuffled"), (13, "aligned"), (16, "shuffled")):
        out.append((f"dim {dim}: 600 classes, 8 slabs + 1, {order}", (dim, 3, (T - 4000, 4000), 600, long_classes, order),
                    dict(slabs=9, units=(8, 10), order=order)))
    for C, order in ((255, "shuffled"), (256, "shuffled"), (256, "aligned"), (257, "shuffled")):
        out.append((f"dim 13: {C} classes, slab + 1, {order}", (13, 3, (LDA_SLAB - 40, 41), C, ((C - 1, LDA_CHUNK + 1),), order),
                    dict(slabs=2, units=(2,), order=order)))
    # the reductions add eight partials a step, then the rest: 7 and 8 slabs (9 above), classes of 7, 8 and 9 units
    step_classes = ((0, 7 * LDA_CHUNK), (300, 8 * LDA_CHUNK), (599, 8 * LDA_CHUNK + 1))
    for slabs in (7, 8):
        out.append((f"dim 13: 600 classes, {slabs} slabs, shuffled", (13, 3, (slabs * LDA_SLAB - 4000, 4000), 600, step_classes, "shuffled"),
                    dict(slabs=slabs, units=(7, 8, 9), order="shuffled")))
    return out


LDA_CASES = lda_cases()
LDA_IDS = [c[0].replace(" ", "-").replace(":", "").replace(",", "") for c in LDA_CASES]


def lda_reaches_its_path(name, case, want):
    got = S.lda_counts(case)
    T = int(case.frame_off[-1])
    slabs, un = -(-T // LDA_SLAB), S.units(got, LDA_CHUNK)
    assert slabs == want["slabs"] and len(case.frame_off) == 3, name
    for n in want["units"]:
        assert n in un, (name, n)
    assert np.count_nonzero(got) > 0.9 * case.n_classes and np.median(got) < 64, name        # the rest hold a handful
    ali = case.ali.astype(np.int64)
    start = np.flatnonzero(np.concatenate([[True], ali[1:] != ali[:-1]]))
    length = np.diff(np.concatenate([start, [len(ali)]]))[lda_ref.frame_tables(case)[0][start] >= 0]      # runs that take part
    if want["order"] == "aligned":
        assert set(S.RUN_LENGTHS if want["slabs"] > 2 else S.RUN_LENGTHS[:3]) <= set(length.tolist()) and length.max() >= 65, name
    else:
        assert length.max() < 63, name
    return (f"LDA {name}: {T} frames in {slabs} slabs, {case.n_classes} classes (scan: {(case.n_classes + 255) // 256} a thread, sort: "
            f"{int(case.n_classes).bit_length()} bits), {int(un.sum())} units (longest class {int(un.max())}), S = {case.S}, longest run {int(length.max())}")


@pytest.mark.parametrize("name,args,want", LDA_CASES, ids=LDA_IDS)
def test_lda_twin_at_many_classes_and_slabs(name, args, want):
    case = S.lda_case(*args)
    print(lda_reaches_its_path(name, case, want))
    counts = np.zeros(len(case.tid2class), np.int64)
    got = lda_statistics_host(case.mfcc, case.frame_off, case.utt2spk, case.cmvn, case.ali, case.tables, case.ctx,
                              num_classes=case.n_classes, tid_count=counts)
    ref = lda_ref.statistics(case)
    assert got.zero.tobytes() == ref.zero.tobytes() and np.array_equal(got.first, ref.first) and np.array_equal(got.second, ref.second)
    cls, _w = lda_ref.frame_tables(case)
    assert np.array_equal(counts, np.bincount(case.ali[cls >= 0], minlength=len(counts)))


# ---- tree statistics ------------------------------------------------------------------------------------------------------------
def tree_host(case):
    return tree_statistics_host(case.feats, case.frame_off, case.ali, case.tm, case.ci)


def tree_equal_to_ref(case, got):
    st, fe, skipped = got
    keys, count, s, q, rfe, rskipped = TR.accumulate(case)
    assert skipped == rskipped == 0
    assert st.keys.dtype == np.uint64 and np.array_equal(st.keys, keys) and np.array_equal(fe, rfe)
    assert np.array_equal(st.count, count) and np.array_equal(st.sum, s) and np.array_equal(st.sumsq, q)
    assert int(count.sum()) == int(case.frame_off[-1])
    return st


def tree_line(name, case, st):
    n_phones = int(max(case.tm.topo.phones))
    bits = n_phones.bit_length()
    un = S.units(st.count, TREE_CHUNK)
    return (f"tree {name}: {int(case.frame_off[-1])} frames, {st.num_events} events, n_phones {n_phones} ({bits} bits a phone, sort: "
            f"{3 * bits + 9} bits), longest event {int(un.max())} chunks, {int(un[un > 1].sum())} units of long events")


def test_tree_twin_on_sparse_phone_ids():
    case = S.tree_sparse_case()
    assert np.diff(case.frame_off).tolist() == list(S.SPARSE_LENGTHS)
    st = tree_equal_to_ref(case, tree_host(case))
    print(tree_line("sparse phone ids", case, st))
    W = st.windows()
    assert int(st.keys.max()) == 0xFFFF0FFFF0FFFF00 and st.keys[-1] == tree_key(65535, 65535, 65535, 0)
    assert set(S.SPARSE_PHONES) <= set(W[:, 1].tolist()) | set(W[:, 0].tolist()) | set(W[:, 2].tolist())
    for ci in S.SPARSE_CI:                                        # both context-independent phones occur, without context
        assert (W[:, 1] == ci).any() and np.all(W[W[:, 1] == ci][:, [0, 2]] == 0)
    assert (W[:, 0] >= 1 << 15).any() and (W[:, 2] >= 1 << 15).any() and set(st.pdf_classes().tolist()) == {0, 1, 2}


@pytest.mark.parametrize("n_phones", S.PHONE_COUNTS)
def test_tree_twin_at_every_key_width(n_phones):
    case = S.tree_phone_count_case(n_phones)
    assert int(max(case.tm.topo.phones)) == n_phones
    st = tree_equal_to_ref(case, tree_host(case))
    print(tree_line(f"n_phones {n_phones}", case, st))
    W = st.windows()
    assert [n_phones, n_phones, 2] in W.tolist() or [n_phones, n_phones, n_phones] in W.tolist()
    assert (W[:, 0] == n_phones).any() and (W[:, 2] == n_phones).any()


def test_tree_twin_on_pdf_classes_up_to_255():
    case = S.tree_pdf_class_case()
    st = tree_equal_to_ref(case, tree_host(case))
    print(tree_line("pdf-classes 0, 254, 255", case, st))
    assert set(st.pdf_classes().tolist()) == {0, 254, 255}


def test_tree_twin_on_long_events():
    case = S.tree_long_event_case(TREE_CHUNK)
    st = tree_equal_to_ref(case, tree_host(case))
    print(tree_line("long events", case, st))
    assert {8 * TREE_CHUNK + 1, 17 * TREE_CHUNK} <= set(st.count.tolist())
    assert sorted(S.units(st.count, TREE_CHUNK).tolist())[-2:] == [9, 17]


def test_tree_twin_on_events_at_the_reductions_step():
    case = S.tree_step_event_case(TREE_CHUNK)
    st = tree_equal_to_ref(case, tree_host(case))
    print(tree_line("events of 8, 9, 10 chunks", case, st))
    assert sorted(S.units(st.count, TREE_CHUNK).tolist())[-3:] == [8, 9, 10]


def test_tree_twin_with_every_frame_its_own_event():
    k = S.small_event_phones(CUS)
    case = S.tree_every_frame_case(k)
    st, fe, _skipped = got = tree_host(case)
    tree_equal_to_ref(case, got)
    print(tree_line(f"de Bruijn over {k} phones", case, st))
    assert (k - 1) ** 3 <= 32 * CUS < k ** 3 == st.num_events == len(case.ali) and np.all(st.count == 1)
    assert sorted(fe.tolist()) == list(range(len(case.ali)))


def one_event_expect(case):
    """(count, Σx, Σx²) of the single event in integers."""
    x = case.feats[:, 0].astype(np.int64)
    return len(x), float(x.sum()), float((x * x).sum())


def test_tree_twin_on_one_event_of_every_frame():
    case = S.tree_one_event_case(TREE_CHUNK, CUS)
    T = int(case.frame_off[-1])
    assert len(case.frame_off) == 9 and T > TREE_CHUNK * 32 * CUS and case.feats.shape == (T, 1)
    st, fe, skipped = tree_host(case)
    print(tree_line("one event", case, st))
    n, s, q = one_event_expect(case)
    assert skipped == 0 and st.keys.tolist() == [int(tree_key(0, 3, 0, 0))] and st.count.tolist() == [n] == [T]
    assert st.sum.tolist() == [[s]] and st.sumsq.tolist() == [[q]] and not fe.any()
    assert S.units(st.count, TREE_CHUNK)[0] > 32 * CUS


def test_phone_ids_end_at_65535():
    """65 535 is the largest phone id the key holds (the sparse case runs it); 65 536 is refused before any table is built."""
    tm = S.sparse_tm((1, 65536), (1,))
    with pytest.raises(_lib.MfaHipError, match="65536"):
        tree_statistics_host(np.zeros((1, 1), np.float32), np.array([0, 1]), np.array(TR.phone_path(tm, 1, [1]), np.int32), tm)
