"""The tree statistics on the device (mfa_tree_acc_batch, csrc/tree_acc.hip) against the host twin and the dict-of-events
restatement of tests/tree_ref.py.

Keys, ``frame_event``, ``n_events``, ``skipped`` and counts are equal outright.  Sums: integer-valued features in [−8, 8] make
every partial sum exact in double, so the device must give the twin's bits whatever its order; real features stay under the
derived bound (2n + 2)·2⁻⁵³·Σ|terms| per event.  Shapes: the smallest at which each mechanism can go wrong — utterances of 0,
1, 2, 63, 64, 65 and 129 frames (the 64-frame step of the key pass), one-frame phones, events of chunk − 1, chunk, chunk + 1
and 2·chunk + 1 frames (the partial rows and their reduction), one event holding every frame, every frame its own event.  Key
widths (phone ids up to 65 535, pdf-classes up to 255), events of nine chunks and more and more events and units than the
kernels have wavefronts are in tests/test_gpu_stats_scale.py."""
import ctypes

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError, _ptr
from montreal_forced_aligner_amd.stats import tree_statistics, tree_statistics_host, tree_tid_tables
from tests import tree_ref as R

pytestmark = pytest.mark.gpu


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def device(engine, case, **kw):
    st, fe, skipped = tree_statistics(engine, dev(engine, case.feats), case.frame_off, dev(engine, case.ali), case.tm, case.ci, **kw)
    return st, fe.cpu().numpy(), skipped


def host(case):
    return tree_statistics_host(case.feats, case.frame_off, case.ali, case.tm, case.ci)


def assert_same(got, want, exact=True, case=None):
    (st, fe, skipped), (ht, hfe, hskipped) = got, want
    assert skipped == hskipped
    assert st.keys.dtype == np.uint64 and np.array_equal(st.keys, ht.keys)
    assert np.array_equal(fe, hfe)
    assert np.array_equal(st.count, ht.count)
    if exact:
        assert np.array_equal(st.sum, ht.sum) and np.array_equal(st.sumsq, ht.sumsq)
    else:
        _k, count, s, q, _fe, _sk, a1, a2 = R.accumulate(case, want_abs=True)
        for stats in (st, ht):
            assert np.all(np.abs(stats.sum - s) <= R.bound(count, a1)) and np.all(np.abs(stats.sumsq - q) <= R.bound(count, a2))


def _chunk(engine):
    return int(engine.lib.mfa_tree_acc_chunk_frames())


@pytest.mark.parametrize("dim", [1, 13, 39, 40, 48])
def test_exact_on_integers(engine, dim):
    rng = np.random.default_rng(dim)
    for n in R.LENGTHS:                                            # one utterance of every length
        case = R.make_case(rng, [n], dim)
        assert_same(device(engine, case), host(case))
    case = R.make_case(rng, list(R.LENGTHS) + [300, 0, 77], dim)   # together, empty ones between and at the end
    got = device(engine, case)
    assert got[0].num_events > 20 and int(got[0].count.sum()) == int(case.frame_off[-1])
    assert_same(got, host(case))
    keys, count, s, q, fe, skipped = R.accumulate(case)            # and the restatement itself
    assert np.array_equal(got[0].keys, keys) and np.array_equal(got[1], fe) and np.array_equal(got[0].sum, s)
    assert np.array_equal(got[0].sumsq, q) and np.array_equal(got[0].count, count) and got[2] == skipped == 0


def test_real_features_within_the_derived_bound(engine):
    chunk = _chunk(engine)
    tm = R.mono_tm()
    rng = np.random.default_rng(8)
    case = R.make_case(rng, [400, 1, 129, 64, 700], 13, integer=False)
    # and a long event: its chunks are added in another order than the twin's one loop
    long = np.concatenate([R.phone_path(tm, 1, [2 * chunk + 1, 5, 5]), R.utterance(rng, tm, 100)]).astype(np.int32)
    case = R.Case(tm, np.concatenate([case.feats, (rng.normal(size=(len(long), 13)) * 9).astype(np.float32)]),
                  np.append(case.frame_off, case.frame_off[-1] + len(long)), np.concatenate([case.ali, long]), case.ci)
    assert_same(device(engine, case), host(case), exact=False, case=case)


@pytest.mark.parametrize("dim", [13, 48])
def test_events_around_a_chunk(engine, dim):
    chunk = _chunk(engine)
    tm = R.mono_tm()
    rng = np.random.default_rng(31 + dim)
    # context-independent three-state phones: a state's frames are one event
    ali = np.concatenate([R.phone_path(tm, 1, [chunk - 1, chunk, chunk + 1]), R.phone_path(tm, 3, [1]),
                          R.phone_path(tm, 2, [2 * chunk + 1, 1, 3 * chunk])]).astype(np.int32)
    x = rng.integers(-8, 9, size=(len(ali), dim)).astype(np.float32)
    case = R.Case(tm, x, np.array([0, len(ali)], dtype=np.int64), ali, R.CI)
    got = device(engine, case)
    assert sorted(got[0].count.tolist()) == sorted([chunk - 1, chunk, chunk + 1, 1, 2 * chunk + 1, 1, 3 * chunk])
    assert_same(got, host(case))
    # the same frames spread over three utterances, each ending at a final id: the long events gather frames of all three
    reps = [R.phone_path(tm, 1, [chunk - 1, 3, 2]), R.phone_path(tm, 1, [chunk, 3, 2]), R.phone_path(tm, 1, [5, 3, chunk + 1])]
    ali = np.concatenate(reps).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum([len(r) for r in reps])]).astype(np.int64)
    case = R.Case(tm, rng.integers(-8, 9, size=(len(ali), dim)).astype(np.float32), fo, ali, R.CI)
    got = device(engine, case)
    assert got[0].count.tolist() == [2 * chunk + 4, 9, chunk + 5]
    assert_same(got, host(case))


def test_one_event_and_every_frame_its_own(engine):
    chunk = _chunk(engine)
    rng = np.random.default_rng(6)
    # one context-independent one-state phone over every frame of three utterances
    tm = R.mono_tm()
    lens = [3 * chunk + 17, 1, 130]
    ali = np.concatenate([R.phone_path(tm, 3, [n]) for n in lens]).astype(np.int32)
    case = R.Case(tm, rng.integers(-8, 9, size=(len(ali), 40)).astype(np.float32),
                  np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), ali, (3,))
    got = device(engine, case)
    assert got[0].num_events == 1 and got[0].count[0] == sum(lens) and np.all(got[1] == 0)
    assert_same(got, host(case))
    # one-frame phones in a de Bruijn order: every (left, centre, right) window of the utterance is another one
    k = 6
    tm1 = R.mono_tm(k, tuple(range(1, k + 1)))
    seq, a = [], [0] * (3 * k)

    def db(t, p):
        if t > 3:
            if 3 % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    phones = [s + 1 for s in seq]
    assert len(phones) == k ** 3
    ali = np.concatenate([R.phone_path(tm1, p, [1]) for p in phones]).astype(np.int32)
    case = R.Case(tm1, rng.integers(-8, 9, size=(len(ali), 13)).astype(np.float32), np.array([0, len(ali)], dtype=np.int64), ali, ())
    got = device(engine, case)
    assert got[0].num_events == len(ali) and np.all(got[0].count == 1)
    assert sorted(got[1].tolist()) == list(range(len(ali)))
    assert_same(got, host(case))


def test_skipped_utterances(engine):
    rng = np.random.default_rng(9)
    case = R.make_case(rng, [50, 64, 65, 129, 40, 200], 5)
    tm, fo = case.tm, case.frame_off
    case.ali[fo[1] + 7] = 0                                             # a transition-id 0
    case.ali[fo[3] - 1] = R.phone_path(tm, 4, [2, 1, 1])[0]             # an unfinished last phone
    seg = R.phone_path(tm, 4, [1, 1, 1])
    case.ali[fo[3]: fo[3] + 3] = [seg[0], R.phone_path(tm, 5, [1, 1, 1])[1], seg[2]]   # a phone change inside a segment
    case.ali[fo[3] + 3: fo[4]] = R.utterance(rng, tm, 126)
    case.ali[fo[5] + 150] = tm.num_transition_ids + 1                   # an id past the table, beyond the second step
    got = device(engine, case)
    assert got[2] == 4 and np.all(got[1][fo[1]: fo[4]] == -1) and np.all(got[1][fo[5]:] == -1) and np.all(got[1][fo[4]: fo[5]] >= 0)
    assert_same(got, host(case))


def raw_call(engine, case, cap, feats=True, total=None, dim=None, n_phones=None):
    """mfa_tree_acc_batch itself with ``cap`` rows of sentinels: (rc, n_events, skipped, key, count, sum, sumsq)."""
    d = engine.device
    phone, cls, final, ci = tree_tid_tables(case.tm, case.ci)
    tabs = [torch.from_numpy(a).to(d) for a in (phone, cls, final, ci)]
    x, ali, fo = dev(engine, case.feats), dev(engine, case.ali), dev(engine, case.frame_off)
    D = int(case.feats.shape[1]) if dim is None else dim
    T = int(case.frame_off[-1]) if total is None else total
    fe = torch.full((max(int(case.frame_off[-1]), 1),), -7, dtype=torch.int32, device=d)
    scal = torch.full((2,), -7, dtype=torch.int64, device=d)
    key = torch.full((max(cap, 1),), -7, dtype=torch.int64, device=d)
    cnt = torch.full((max(cap, 1),), -7, dtype=torch.int64, device=d)
    s = torch.full((max(cap, 1), D), -7.0, dtype=torch.float64, device=d)
    q = torch.full((max(cap, 1), D), -7.0, dtype=torch.float64, device=d)
    rc = engine.lib.mfa_tree_acc_batch(engine.ctx, _ptr(x) if feats else None, _ptr(fo), len(case.frame_off) - 1, T, D, _ptr(ali),
                                       _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), int(phone.shape[0]), _ptr(tabs[3]),
                                       int(ci.shape[0]) - 1 if n_phones is None else n_phones, cap, _ptr(fe), ctypes.c_void_p(scal.data_ptr()),
                                       ctypes.c_void_p(scal.data_ptr() + 8), _ptr(key), _ptr(cnt), _ptr(s), _ptr(q))
    torch.cuda.synchronize()
    n_events, skipped = scal.cpu().tolist()
    return rc, n_events, skipped, key.cpu().numpy(), cnt.cpu().numpy(), s.cpu().numpy(), q.cpu().numpy(), fe.cpu().numpy()


def test_capacity_and_empty_calls(engine):
    case = R.make_case(np.random.default_rng(2), [64, 129, 30], 13)
    want = host(case)
    E = want[0].num_events
    for cap in (0, E - 1):
        rc, n_events, skipped, key, cnt, s, q, fe = raw_call(engine, case, cap)
        assert rc == 0 and n_events == E and skipped == 0
        assert np.all(key == -7) and np.all(cnt == -7) and np.all(s == -7.0) and np.all(q == -7.0)     # no row written
        assert np.array_equal(fe, want[1])
    rc, n_events, _sk, key, cnt, s, q, _fe = raw_call(engine, case, E)
    assert rc == 0 and n_events == E and np.array_equal(key.view(np.uint64), want[0].keys) and np.array_equal(s, want[0].sum)
    # the Python layer repeats the call
    assert_same(device(engine, case, cap=1), want)
    assert_same(device(engine, case, cap=0), want)
    # no utterance, and utterances without a frame
    empty = R.Case(case.tm, np.zeros((0, 13), np.float32), np.zeros(1, np.int64), np.zeros(0, np.int32), case.ci)
    st, fe, skipped = device(engine, empty)
    assert st.num_events == 0 and st.sum.shape == (0, 13) and fe.shape == (0,) and skipped == 0
    empty.frame_off = np.zeros(4, np.int64)
    st, fe, skipped = device(engine, empty)
    assert st.num_events == 0 and skipped == 0


def test_two_calls_give_the_same_bits(engine):
    chunk = _chunk(engine)
    rng = np.random.default_rng(77)
    tm = R.mono_tm()
    case = R.make_case(rng, [900, 64, 3 * chunk, 129], 39, integer=False, tm=tm, phones=[1, 4, 1, 5, 1, 2, 1])
    a, b = device(engine, case), device(engine, case)
    assert a[0].sum.tobytes() == b[0].sum.tobytes() and a[0].sumsq.tobytes() == b[0].sumsq.tobytes()
    assert np.array_equal(a[0].keys, b[0].keys) and np.array_equal(a[1], b[1])
    assert_same(a, host(case), exact=False, case=case)


def test_refusals_leave_the_context_usable(engine):
    ok = R.make_case(np.random.default_rng(1), [64, 30], 13)
    want = host(ok)

    def refused(match, **kw):
        rc = raw_call(engine, ok, 8, **kw)[0]
        assert rc != 0
        msg = engine.lib.mfa_last_error(engine.ctx).decode()
        assert match in msg, msg
        assert_same(device(engine, ok), want)

    wide = R.make_case(np.random.default_rng(1), [20], 49)
    with pytest.raises(MfaHipError, match="48"):
        device(engine, wide)
    assert_same(device(engine, ok), want)
    refused("NULL", feats=False)
    refused("frames in one call", total=1 << 31)
    refused("feature dim", dim=0)
    refused("phones", n_phones=1 << 16)                    # the key's left field has 16 bits (refused before the table is read)
    assert raw_call(engine, ok, 8, total=(1 << 31) - 1, feats=False)[0] != 0      # the largest count is let past that check
    assert "NULL" in engine.lib.mfa_last_error(engine.ctx).decode()
    with pytest.raises(MfaHipError, match="only 3 and 1"):
        tree_statistics(engine, dev(engine, ok.feats), ok.frame_off, dev(engine, ok.ali), ok.tm, ok.ci, context_width=5, central_position=2)
    with pytest.raises(MfaHipError, match="on the device"):
        tree_statistics(engine, torch.from_numpy(ok.feats), ok.frame_off, dev(engine, ok.ali), ok.tm, ok.ci)
