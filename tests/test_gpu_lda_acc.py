"""The LDA statistics on the device (mfa_lda_acc_batch, csrc/lda_acc.hip) against the float64 restatement of
tests/lda_ref.py and the host twin.

Exact tier: integer-valued features in [−8, 8] and weights from {0, ½, 1, 2} — every product and every partial sum is exact
in double, so the device must give the restatement's bits whatever its summation order.  That is the test of the f64 matrix
instruction's operand and result layouts, of the clamped splice and of the tile mirror.  Soft tier: real features with
per-speaker CMVN under the derived bound (2T + 2)·2⁻⁵³·Σ|terms|.  Shapes: the smallest at which each mechanism can go wrong —
utterances of 1, 2, ctx, ctx + 1 frames and of slab − 1, slab, slab + 1; spliced widths that are no multiple of 16, one that
is, and the widest; a class of chunk + 1 frames.  Key counts (255 – 600 classes), classes of eight chunks and more and batches
of nine slabs are in tests/test_gpu_stats_scale.py."""
import dataclasses

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.stats import LdaStats, lda_statistics, lda_statistics_host
from tests import lda_ref
from tests.test_lda_cpu import assert_same_bits, assert_within_bound, host

pytestmark = pytest.mark.gpu


def dev(engine, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(engine.device)


def device(engine, case, **kw):
    return lda_statistics(engine, dev(engine, case.mfcc), case.frame_off, case.utt2spk, dev(engine, case.cmvn), dev(engine, case.ali),
                          case.tables, case.ctx, num_classes=case.n_classes, **kw)


def _slab(engine):
    return int(engine.lib.mfa_lda_acc_slab_frames())


def _chunk(engine):
    return int(engine.lib.mfa_lda_acc_chunk_frames())


SHAPES = [(13, 3), (5, 1), (16, 3), (13, 0), (8, 7), (128, 0)]


@pytest.mark.parametrize("dim,ctx", SHAPES)
def test_exact_on_integers(engine, dim, ctx):
    rng = np.random.default_rng(1000 * dim + ctx)
    slab, chunk = _slab(engine), _chunk(engine)
    # one utterance, every short length and the three around a slab; one class
    for n in (1, 2, max(ctx, 1), ctx + 1, slab - 1, slab, slab + 1):
        case = lda_ref.integer_case(rng, dim, ctx, [n], 1)
        assert_same_bits(device(engine, case), lda_ref.statistics(case), f"one utterance of {n}")
    # five utterances whose boundaries fall inside slabs and inside tiles, and empty ones between and around them; three classes
    case = lda_ref.integer_case(rng, dim, ctx, [0, slab - 1, ctx + 1, 0, 70, max(ctx, 1), slab + 1, 0], 3)
    ref = lda_ref.statistics(case)
    assert np.all(ref.zero > 0)
    assert_same_bits(device(engine, case), ref, "five utterances")
    # 300 classes, one of them holding chunk + 1 frames (two units), most of the others a handful
    T = slab + 1
    cls = rng.integers(1, 300, size=T)
    cls[rng.permutation(T)[: chunk + 1]] = 0
    case = lda_ref.integer_case(rng, dim, ctx, [T - 40, 40], 300, class_of_frame=cls)
    case.tid_weight[1:5] = [1.0, 0.5, 1.0, 2.0]                 # class 0: no weight 0, so that chunk + 1 frames take part
    ref = lda_ref.statistics(case)
    cls_ref, _w = lda_ref.frame_tables(case)
    assert (cls_ref == 0).sum() == chunk + 1
    assert_same_bits(device(engine, case), ref, "300 classes")


def test_counts_and_frames_that_take_no_part(engine):
    rng = np.random.default_rng(5)
    case = lda_ref.integer_case(rng, 13, 3, [40, 60, 50, 300], 4)
    n_tids = len(case.tid2class)
    case.tid2class[5] = 4
    case.tid2class[6] = -1
    case.ali[:150] = np.concatenate([np.zeros(30), np.full(30, n_tids), np.full(30, -3), np.full(20, 5), np.full(20, 6),
                                     np.full(20, 1)]).astype(np.int32)
    case.mfcc[:150] = np.nan                                    # whatever those frames hold: the first three utterances
    case.mfcc[:75] = np.inf                                     # take no part, and no frame of the fourth splices them in
    start = LdaStats(rng.integers(0, 9, size=4).astype(np.float64), rng.integers(-9, 9, size=(4, 91)).astype(np.float64),
                     np.zeros((91, 91)))
    sym = rng.integers(-9, 9, size=(91, 91)).astype(np.float64)
    start.second = sym + sym.T
    c_dev, c_host = np.arange(n_tids, dtype=np.int64), np.arange(n_tids, dtype=np.int64)
    got = device(engine, case, into=start.copy(), tid_count=c_dev)
    want = host(case, into=start.copy(), tid_count=c_host)
    assert np.all(np.isfinite(got.second))
    assert_same_bits(got, want)
    assert np.array_equal(c_dev, c_host) and c_dev.sum() > np.arange(n_tids).sum()
    # the same frames alone: no trace of the others
    keep = dataclasses.replace(case, mfcc=case.mfcc[150:], ali=case.ali[150:], frame_off=np.array([0, 300], np.int64))
    only = device(engine, keep)
    assert_same_bits(LdaStats(got.zero - start.zero, got.first - start.first, got.second - start.second), only)


def test_spliced_vectors_are_the_feature_kernels(engine):
    """Real MFCC-like rows, two speakers with CMVN.  The feature kernel with an identity as its matrix returns the spliced
    vectors themselves (1·x added to zeros: exact); it takes at most 64 rows, so the 91 × 91 identity goes in two halves.
    The statistics of that output, in numpy, are the restatement's to the bit: both read the same float32 vectors."""
    case = lda_ref.real_case(np.random.default_rng(17), 13, 3, [300, 1, 211, 2, 450, 3, 4], 11)
    eye = np.eye(91, dtype=np.float32)
    mfcc, cmvn = dev(engine, case.mfcc), dev(engine, case.cmvn)
    parts = [engine.features(mfcc, case.frame_off, case.utt2spk, cmvn, lda=dev(engine, eye[a:b]), splice_context=3).cpu().numpy()
             for a, b in ((0, 46), (46, 91))]
    x_dev = np.concatenate(parts, axis=1)
    assert np.array_equal(x_dev, lda_ref.spliced(case))
    # device against the twin and the restatement under the derived bound
    got = device(engine, case)
    ref = assert_within_bound(got, case, "device")
    twin = host(case)
    _st, abs2, abs1, n = lda_ref.statistics(case, want_abs=True)
    assert np.all(np.abs(got.second - twin.second) <= lda_ref.bound(n, abs2))
    assert np.all(np.abs(got.first - twin.first) <= lda_ref.bound(n, abs1))
    assert np.array_equal(got.zero, twin.zero) and ref.zero.sum() > 0


def test_two_calls_give_the_same_bits_and_batches_add_up(engine):
    slab = _slab(engine)
    case = lda_ref.real_case(np.random.default_rng(23), 13, 3, [slab // 2 + 11, 300, 5, slab // 2, 100, 77], 40)
    one, again = device(engine, case), device(engine, case)
    assert_same_bits(one, again)
    # `into`: the caller's value first.  On integers the sum is exact whatever the order
    ints = lda_ref.integer_case(np.random.default_rng(3), 13, 3, [200, 100], 3)
    plain = device(engine, ints)
    twice = device(engine, ints, into=plain.copy())
    assert_same_bits(twice, LdaStats(2 * plain.zero, 2 * plain.first, 2 * plain.second))
    # two batches against one: under the bound
    cut = 3
    fa = int(case.frame_off[cut])
    a = dataclasses.replace(case, mfcc=case.mfcc[:fa], ali=case.ali[:fa], frame_off=case.frame_off[:cut + 1], utt2spk=case.utt2spk[:cut])
    b = dataclasses.replace(case, mfcc=case.mfcc[fa:], ali=case.ali[fa:], frame_off=case.frame_off[cut:] - fa, utt2spk=case.utt2spk[cut:])
    both = device(engine, b, into=device(engine, a))
    _st, abs2, abs1, n = lda_ref.statistics(case, want_abs=True)
    assert np.all(np.abs(both.second - one.second) <= lda_ref.bound(n, abs2))
    assert np.all(np.abs(both.first - one.first) <= lda_ref.bound(n, abs1))
    assert np.array_equal(both.zero, one.zero)


def test_prune_keeps_the_twins_set(engine):
    rng = np.random.default_rng(11)
    case = lda_ref.integer_case(rng, 5, 1, [700, 1, 350, 1200, 90], 3)
    case.tid_weight[1:] = np.tile(np.array([1.0, 0.5, 3.0, 4.0], np.float32), 3)
    keys = np.array([7, 1000, 2, 65536, 99], dtype=np.uint32)
    got = device(engine, case, rand_prune=4.0, utt_keys=keys, seed=9)
    want = host(case, rand_prune=4.0, utt_keys=keys, seed=9)
    assert_same_bits(got, want)
    assert_same_bits(got, lda_ref.statistics(case, rand_prune=4.0, utt_keys=keys, seed=9))
    assert 0 < got.zero.sum() < 4.0 * case.ali.shape[0] and np.all(got.zero % 4.0 == 0)
    # batch cuts do not change the kept set
    cut = LdaStats.zeros(3, case.S)
    for a, b in ((0, 2), (2, 3), (3, 5)):
        fa, fb = int(case.frame_off[a]), int(case.frame_off[b])
        part = dataclasses.replace(case, mfcc=case.mfcc[fa:fb], ali=case.ali[fa:fb], frame_off=case.frame_off[a:b + 1] - fa)
        device(engine, part, rand_prune=4.0, utt_keys=keys[a:b], seed=9, into=cut)
    assert_same_bits(got, cut)


def test_refusals_leave_the_context_usable(engine):
    ok = lda_ref.integer_case(np.random.default_rng(2), 4, 1, [50, 3], 2)
    want = lda_ref.statistics(ok)
    lib, ctx = engine.lib, engine.ctx
    from montreal_forced_aligner_amd._lib import _ptr
    mfcc, ali = dev(engine, ok.mfcc), dev(engine, ok.ali)
    fo, t2c, tw = dev(engine, ok.frame_off), dev(engine, ok.tid2class), dev(engine, ok.tid_weight)
    zero, first = torch.zeros(2, dtype=torch.float64, device=engine.device), torch.zeros((2, 12), dtype=torch.float64, device=engine.device)
    second = torch.zeros((12, 12), dtype=torch.float64, device=engine.device)
    cmvn = torch.zeros((1, 2, 5), dtype=torch.float64, device=engine.device)

    def call(dim=4, ctx_=1, C=2, total=53, mfcc_=mfcc, second_=second, cmvn_=None, theta=0.0):
        return lib.mfa_lda_acc_batch(ctx, _ptr(mfcc_), _ptr(fo), 2, total, dim, None, _ptr(cmvn_), ctx_, _ptr(ali), _ptr(t2c), _ptr(tw),
                                     len(ok.tid2class), C, theta, None, 0, _ptr(zero), _ptr(first), _ptr(second_), None)

    for kw, word in ((dict(dim=43), "128"), (dict(dim=0), "spliced"), (dict(ctx_=-1), "spliced"), (dict(C=0), "classes"),
                     (dict(mfcc_=None), "NULL"), (dict(second_=None), "NULL"), (dict(cmvn_=cmvn), "utt2spk"),
                     (dict(theta=4.0), "keys"), (dict(total=2 ** 31), "2^31")):
        assert call(**kw) != 0, kw
        assert word in lib.mfa_last_error(ctx).decode(), (kw, lib.mfa_last_error(ctx))
        assert_same_bits(device(engine, ok), want, str(kw))                # the context works afterwards
    assert float(second.abs().sum().item()) == 0.0                         # a refused call wrote nothing
    assert call(total=0) == 0 and float(zero.sum().item()) == 0.0          # no frames: no error, nothing written
    big = lda_ref.integer_case(np.random.default_rng(2), 43, 1, [5], 2)
    with pytest.raises(MfaHipError, match="128"):
        device(engine, big)
