"""mfa_align_equal_batch (csrc/align_equal.hip) against its host twin, exactly: both run csrc/align_equal_math.hpp and
everything is integer arithmetic.  The case set of tests/align_equal_cases.py as one batch of 70 utterances of 0 – 300 frames
(18 workgroups of 4 wavefronts; paths of more than 64 positions, so several rounds of the spreading's prefix sum), the same
utterances alone, the batch in reversed order with the same keys, two runs, an empty batch, and each refusal followed by a
correct small call."""
import ctypes as C

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import equal_align as E
from montreal_forced_aligner_amd._lib import GraphBatch, MfaHipError, _ptr, check
from tests import align_equal_cases as A

pytestmark = pytest.mark.gpu

SEED = 1234


@pytest.fixture(scope="module")
def batch(engine):
    cs = A.cases()
    keys = np.arange(100, 100 + len(cs), dtype=np.uint32)
    fo = A.frame_offsets(cs)
    ref_ali, ref_status = E.equal_align_host([c.fst for c in cs], fo, keys, SEED)
    graphs = E.pack_bare(engine, [c.fst for c in cs])
    ali, status = E.equal_align(engine, graphs, fo, keys, SEED)
    torch.cuda.synchronize()
    return cs, keys, fo, graphs, ali.cpu().numpy(), status.cpu().numpy(), ref_ali, ref_status


def test_batch_of_70_equals_the_twin(batch):
    cs, _keys, fo, _graphs, ali, status, ref_ali, ref_status = batch
    assert len(cs) == 70
    assert np.array_equal(status, ref_status), np.flatnonzero(status != ref_status)
    for k, c in enumerate(cs):
        assert np.array_equal(ali[fo[k]: fo[k + 1]], ref_ali[fo[k]: fo[k + 1]]), c.name
    assert (status == 0).sum() >= 40 and (status == 2).sum() >= 10


def test_second_run_gives_the_same_bits(engine, batch):
    cs, keys, fo, graphs, ali, status, _ra, _rs = batch
    a2, s2 = E.equal_align(engine, graphs, fo, keys, SEED)
    assert np.array_equal(a2.cpu().numpy(), ali) and np.array_equal(s2.cpu().numpy(), status)


def test_utterances_alone_equal_their_batch_result(engine, batch):
    cs, keys, fo, _graphs, ali, status, _ra, _rs = batch
    for k in (0, 1, 5, 9, 12, 19, 33, 41, 58, 69):            # hand cases, 0 frames, the longest, with epsilon arcs
        c = cs[k]
        a1, s1 = E.equal_align(engine, E.pack_bare(engine, [c.fst]), np.array([0, c.T]), keys[k: k + 1], SEED)
        assert int(s1.cpu()[0]) == int(status[k]), c.name
        assert np.array_equal(a1.cpu().numpy(), ali[fo[k]: fo[k + 1]]), c.name


def test_reversed_batch_with_the_same_keys(engine, batch):
    cs, keys, fo, _graphs, ali, status, _ra, _rs = batch
    rev = list(range(len(cs)))[::-1]
    ar, sr = E.equal_align(engine, E.pack_bare(engine, [cs[k].fst for k in rev]), A.frame_offsets([cs[k] for k in rev]),
                           keys[rev], SEED)
    assert np.array_equal(sr.cpu().numpy(), status[rev])
    assert np.array_equal(ar.cpu().numpy(), np.concatenate([ali[fo[k]: fo[k + 1]] for k in rev]))


def test_packed_decoding_graphs_with_epsilon_arcs(engine, fx):
    """The layout CorpusAligner decodes from: pack_graphs stores every state's arcs [emitting | epsilon]; the twin on the
    arrays the device holds gives the device's bits."""
    from tests import helpers
    engine.load_gmm(fx.mono_am)
    rng = np.random.default_rng(3)
    fsts = [helpers.with_eps(rng, fx.mono_graph(t), 0.3) for t in ("this is", "the acoustic corpus", "i'm talking pretty fast here")]
    graphs = engine.pack_graphs(fsts, fx.mono_tm)
    fo = np.array([0, 150, 151, 451], dtype=np.int64)
    keys = np.array([7, 8, 9], dtype=np.uint32)
    ali, status = E.equal_align(engine, graphs, fo, keys, 5)
    ref_ali, ref_status = E.equal_align_host_packed(graphs, fo, keys, 5)
    assert np.array_equal(status.cpu().numpy(), ref_status) and np.array_equal(ali.cpu().numpy(), ref_ali)
    assert ref_status.tolist() == [0, 2, 0]


def _small_call_is_right(engine, batch):
    cs, keys, fo, _graphs, ali, status, _ra, _rs = batch
    a1, s1 = E.equal_align(engine, E.pack_bare(engine, [cs[5].fst]), np.array([0, cs[5].T]), keys[5:6], SEED)
    assert int(s1.cpu()[0]) == int(status[5]) == 0 and np.array_equal(a1.cpu().numpy(), ali[fo[5]: fo[6]])


def test_empty_batch_and_refusals_leave_the_context_usable(engine, batch):
    cs, keys, fo, graphs, _ali, _status, _ra, _rs = batch
    lib, ctx = engine.lib, engine.ctx
    gs = graphs.struct()
    d_fo, d_keys = engine._dev(fo), engine._dev(keys)
    out_a = torch.zeros(int(fo[-1]), dtype=torch.int32, device=engine.device)
    out_s = torch.full((len(cs),), -1, dtype=torch.int32, device=engine.device)
    args = (_ptr(d_keys), SEED, _ptr(out_a), _ptr(out_s))
    # n_utt = 0 is no error, whatever the arrays are
    assert lib.mfa_align_equal_batch(ctx, C.byref(GraphBatch(0)), None, 0, 0, None, SEED, None, None) == 0
    # NULL graph arrays with n_utt > 0
    for name in ("d_state_off", "d_arc_base", "d_start", "d_arc_off", "d_final", "d_arc_next", "d_arc_ilabel"):
        bad = graphs.struct()
        setattr(bad, name, None)
        assert lib.mfa_align_equal_batch(ctx, C.byref(bad), _ptr(d_fo), int(fo[-1]), int(graphs.tensors["final"].shape[0]), *args) != 0
        assert b"NULL" in lib.mfa_last_error(ctx)
        _small_call_is_right(engine, batch)
    # 2^31 frames or more
    assert lib.mfa_align_equal_batch(ctx, C.byref(gs), _ptr(d_fo), 1 << 31, int(graphs.tensors["final"].shape[0]), *args) != 0
    assert b"2^31" in lib.mfa_last_error(ctx)
    _small_call_is_right(engine, batch)
    torch.cuda.synchronize()
    assert not out_a.any().item() and (out_s == -1).all().item()      # a refused call writes nothing
    bad = graphs.struct()
    bad.d_final = None
    with pytest.raises(MfaHipError, match="NULL"):
        check(ctx, lib.mfa_align_equal_batch(ctx, C.byref(bad), _ptr(d_fo), int(fo[-1]), 1, *args), "mfa_align_equal_batch")
