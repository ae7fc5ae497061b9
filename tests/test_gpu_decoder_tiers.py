"""The wavefront decoder's large-graph tiers against the oracle, bit for bit: token lists in HBM (viterbi_kernel<false, *>),
HBM lists resumed across a 256-frame window, the capacity shrink and the ladder that makes up for it, the hashed
state→slot table above the first tier, and score rows too wide for the LDS row cache or for speculation.

The cases are tests/decoder_tier_cases.py's (tests/test_decoder_tiers_cpu.py holds them to what they claim, with the oracle
alone); every test first asks mfa_debug_viterbi_plan — the plan align_impl itself consumes — which tier the batch it
packed takes, asserts that it is the one meant, and prints the launches.  Outputs are compared as tests/test_gpu_parity.py's
``_align_case`` and tests/test_gpu_general.py's ``_check_fast`` compare them: status through ``helpers.device_status``;
``ali``, ``words``, ``n_words``, ``like`` and ``frame_like`` equal to the oracle's.  No tolerances.

What a regression in the three places these tiers depend on would show here, argued from viterbi_wave.hpp (nothing below
was tried on a device):
  * ``__threadfence_block()`` after the list write (HBM lists only).  Frame t writes the next token list to HBM at positions
    given by the list order, frame t + 1 reads it back chunk by chunk: a token is read by another lane than the one that
    wrote it.  Without the fence nothing makes the wavefront wait for those stores before the loads of GetCutoff are
    issued.  Every test of the hbm, hbm_default, resume, shrink and wide_rows cases decodes frames of several hundred to
    two thousand tokens that way and compares every frame's alignment and likelihood; whether the hardware's in-order
    vector memory path hides the missing wait is not something a host-side argument can settle.
  * the ``hbits`` handed to the kernel.  The LDS carve is sized from the plan's ``hbits``; the kernel lays its table out from
    ``p.hbits``.  They are now one value (``L.hbits``).  A kernel given a larger table than was carved (direct map, 2 600
    entries, against the 2 048 carved in hashed512) pushes every later array up, the last of them past the allocation;
    one given fewer than N buckets cannot file a frame's tokens: status 3 or 6 where the oracle aligns, in
    test_hashed_table_of_2048_buckets_fits_and_overflows and the capacity scans.  A smaller table that still holds N
    entries only probes longer: results cannot show that, which is why the CPU tests pin ``hbits`` = 11 and the native
    sweep pins ``hbits`` = hash_bits(S, N) of the launch's final N.
  * the ``cur`` carry-over (``cur = vs.cur & 1`` on resume).  It cannot be seen in any result: the list passes' windows are
    K = max(window, 256) frames with ``window`` a multiple of 64, ``cur`` starts at 0 and flips once per frame, so at every
    window boundary it is 0, which is what a kernel without the carry-over would assume.  The resume test would fail for a
    kernel that resumed on the wrong list (``cur = 1``: 256 frames of stale tokens), not for one that dropped the field.
"""
import numpy as np
import pytest
import torch

from tests import decoder_tier_cases as D
from tests import helpers

pytestmark = pytest.mark.gpu

EPS = [False, True]
PATHS = ["dense", "lazy"]
KEYS = ("status", "ali", "words", "n_words", "like", "frame_like")


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


def _decode(engine, c, idx, beam, retry, caps, path, expect=None):
    """Utterances ``idx`` of case ``c`` as one batch through ``engine.align`` ("dense") or ``engine.align_features``
    ("lazy").  ``expect(plan)`` asserts the tier on the plan of the batch as packed.  Returns (host results, frame offsets,
    packed graphs, plan)."""
    fsts, feats = [c["fsts"][k] for k in idx], [c["frames"][k] for k in idx]
    engine.load_gmm(c["am"])
    g = engine.pack_graphs(fsts, c["tm"])
    assert g.has_eps == D.has_eps(fsts)
    plan = D.plan(g.max_states, g.max_arcs, g.has_eps, path == "lazy", retry_beam=retry, **caps)
    print(f"{path} beam {beam} retry {retry} caps {caps}: " +
          "; ".join(f"pass {r['pass']} code {r['code']} N {r['N']} C {r['C']} lds {r['lds_bytes']} "
                    f"lists {'LDS' if r['lists_in_lds'] else 'HBM'} hbits {r['hbits']}" for r in plan))
    if expect is not None:
        expect(plan)
    fo = np.concatenate([[0], np.cumsum([x.shape[0] for x in feats])]).astype(np.int64)
    d_feats = _dev(engine, np.concatenate(feats))
    kw = dict(beam=beam, retry_beam=retry, want_frame_likes=True, **caps)
    if path == "dense":
        ll, ll_off, ll_cols = engine.score(d_feats, fo, g.pdf_list, g.pdf_off_host, g.class_counts)
        res = engine.align(g, ll, ll_off, ll_cols, fo, **kw)
    else:
        res = engine.align_features(g, d_feats, fo, **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}, fo, g, plan


def _equals_oracle(res, fo, u, ref):
    """Utterance ``u`` of ``res`` is the oracle's ``ref``; returns the status."""
    a, b = int(fo[u]), int(fo[u + 1])
    want = helpers.device_status(ref, b - a)
    assert int(res["status"][u]) == want, (u, int(res["status"][u]), want)
    if want in (0, 1):
        assert np.array_equal(res["ali"][a:b], ref["ali"]), u
        nw = int(res["n_words"][u])
        assert np.array_equal(res["words"][a: a + nw], ref["words"]), u
        assert res["like"][u] == np.float32(ref["like"]), (u, res["like"][u], ref["like"])
        assert np.array_equal(res["frame_like"][a:b], ref["per_frame"]), u
    return want


def _same_utterance(res_a, fo_a, ua, res_b, fo_b, ub, what):
    a, b, a2, b2 = int(fo_a[ua]), int(fo_a[ua + 1]), int(fo_b[ub]), int(fo_b[ub + 1])
    assert res_a["status"][ua] == res_b["status"][ub], what
    if int(res_a["status"][ua]) in (0, 1):
        assert res_a["n_words"][ua] == res_b["n_words"][ub] and res_a["like"][ua] == res_b["like"][ub], what
        nw = int(res_a["n_words"][ua])
        assert np.array_equal(res_a["ali"][a:b], res_b["ali"][a2:b2]), what
        assert np.array_equal(res_a["frame_like"][a:b], res_b["frame_like"][a2:b2]), what
        assert np.array_equal(res_a["words"][a: a + nw], res_b["words"][a2: a2 + nw]), what


def _lists_in_hbm(codes, S):
    """Plan check: the launches with these codes keep their token lists in HBM at the full capacity (no shrink)."""
    def expect(plan):
        rows = [r for r in plan if r["code"] in codes]
        assert [r["code"] for r in rows] == list(codes), plan
        assert all(r["lists_in_lds"] == 0 and r["N"] == D.ceil64(S) for r in rows), plan
    return expect


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_hbm_lists_every_utterance_equals_the_oracle(engine, fx, eps, path):
    """One token per state on a batch whose largest graph puts the growth and retry launches' lists in HBM — for every
    utterance of the batch, the small graphs included, which are launched with the large graph's plan."""
    c = D.case("hbm", eps, fx)
    S = max(f.num_states for f in c["fsts"])
    idx = list(range(len(c["fsts"])))
    seen = set()
    for beam, retry in c["beams"]:
        codes = (-2,) if retry == 0.0 else (-2, -1)
        res, fo, g, _ = _decode(engine, c, idx, beam, retry, c["caps"], path, _lists_in_hbm(codes, S))
        assert (g.max_states, tuple(c["caps"].values())) == (S, g.hard_bounds())
        seen |= {_equals_oracle(res, fo, u, ref) for u, ref in enumerate(D.refs("hbm", eps, fx, beam, retry))}
    assert {0, 1} <= seen


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_hbm_lists_small_graphs_decode_as_they_do_alone(engine, fx, eps, path):
    """Batch independence: a small graph gives the same bits in the large graph's batch (HBM lists, the large graph's
    capacities and table) as alone in a batch of its own, where its lists are in LDS."""
    c = D.case("hbm", eps, fx)
    S = max(f.num_states for f in c["fsts"])
    for beam, retry in c["beams"][:2]:
        codes = (-2,) if retry == 0.0 else (-2, -1)
        res, fo, _, _ = _decode(engine, c, list(range(len(c["fsts"]))), beam, retry, c["caps"], path, _lists_in_hbm(codes, S))
        for u in range(1, len(c["fsts"])):
            def in_lds(plan):
                assert all(r["lists_in_lds"] == 1 for r in plan), plan
            alone, fo1, _, _ = _decode(engine, c, [u], beam, retry, D.hard_bounds([c["fsts"][u]]), path, in_lds)
            _same_utterance(res, fo, u, alone, fo1, 0, f"utterance {u}, beam {beam}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_default_capacities_retry_launch_with_lists_in_hbm(engine, fx, eps, path):
    """max_tokens = 1024, 512 back-pointers a frame: the retry launch takes min(4096, max_states) tokens, which a graph of
    about 2 000 states puts in HBM; the large graph needs that launch (status 1)."""
    c = D.case("hbm_default", eps, fx)
    S = max(f.num_states for f in c["fsts"])
    for beam, retry in c["beams"]:
        def expect(plan):
            assert [r["code"] for r in plan] == [0, -2, -1] and plan[1]["lists_in_lds"] == 1, plan
            assert plan[2]["lists_in_lds"] == 0 and plan[2]["N"] == D.ceil64(min(4096, S)), plan
        res, fo, _, _ = _decode(engine, c, list(range(len(c["fsts"]))), beam, retry, c["caps"], path, expect)
        got = [_equals_oracle(res, fo, u, ref) for u, ref in enumerate(D.refs("hbm_default", eps, fx, beam, retry))]
        assert got[0] == 1


@pytest.mark.parametrize("eps", EPS)
def test_hbm_lists_resume_across_the_256_frame_window(engine, fx, eps):
    """The lazy path's list passes decode in windows of K = max(window, 256) frames (align_impl), one launch per window: with
    300 frames the growth launch runs twice, frames 0 … 255 and 256 … 299, and the second launch picks the token lists up
    where the first left them in HBM (the HBM variant parks nothing: it carries the list count, the hash size, the
    back-pointer fill and which of the two lists is current).  Equal to the dense path, which decodes the 300 frames in one
    launch, and to the oracle."""
    c = D.case("resume", eps, fx)
    S = c["fsts"][0].num_states
    assert c["frames"][0].shape[0] == 300
    for beam, retry in c["beams"]:
        lazy, fo, _, _ = _decode(engine, c, [0], beam, retry, c["caps"], "lazy", _lists_in_hbm((-2,), S))
        dense, fo_d, _, _ = _decode(engine, c, [0], beam, retry, c["caps"], "dense", _lists_in_hbm((-2,), S))
        ref = D.refs("resume", eps, fx, beam, retry)[0]
        assert _equals_oracle(lazy, fo, 0, ref) == 0 and _equals_oracle(dense, fo_d, 0, ref) == 0
        for k in KEYS:
            assert np.array_equal(lazy[k], dense[k]), k


def _hashed(plan):
    assert plan[-1]["code"] == -2 and plan[-1]["N"] == 512 and plan[-1]["hbits"] == 11 and plan[-1]["lists_in_lds"] == 1, plan


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_hashed_table_of_2048_buckets_fits_and_overflows(engine, fx, eps, path):
    """512 tokens on a graph of more than 2 048 states: the growth launch's state→slot table is hashed, 2 048 buckets,
    linear probing under hundreds of live tokens.  A beam whose peak fits equals the oracle; one that exceeds 512 tokens
    reports status 3 and nothing else."""
    c = D.case("hashed512", eps, fx)
    (fit, _), (over, _) = c["beams"]
    res, fo, _, _ = _decode(engine, c, [0], fit, 0.0, c["caps"], path, _hashed)
    assert _equals_oracle(res, fo, 0, D.refs("hashed512", eps, fx, fit, 0.0)[0]) == 0
    res, fo, _, _ = _decode(engine, c, [0], over, 0.0, c["caps"], path, _hashed)
    assert res["status"].tolist() == [3]


def _scan(engine, fx, eps, path, which, values, overflow):
    """One capacity scanned at the fitting beam: every result is the overflow status or exactly the oracle's; once a
    capacity succeeds every larger one does; both outcomes occur."""
    c = D.case("hashed512", eps, fx)
    beam = D.HASHED_SCAN_BEAM
    ref = D.refs("hashed512", eps, fx, beam, 0.0)[0]
    ok = []
    for v in values:
        res, fo, _, _ = _decode(engine, c, [0], beam, 0.0, dict(c["caps"], **{which: v}), path)
        if int(res["status"][0]) == overflow:
            ok.append(False)
        else:
            assert _equals_oracle(res, fo, 0, ref) == 0
            ok.append(True)
    print(f"{which} {list(values)}: {['fits' if k else f'status {overflow}' for k in ok]}")
    assert ok == sorted(ok), (values, ok)                     # monotone: no failure above a success
    assert ok[0] is False and ok[-1] is True, (values, ok)    # both outcomes


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_token_capacity_scan_is_status_3_or_the_oracle(engine, fx, eps, path):
    S = D.case("hashed512", eps, fx)["fsts"][0].num_states
    _scan(engine, fx, eps, path, "max_tokens", (64, 128, 256, 512, 1024, S), 3)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_back_pointer_capacity_scan_is_status_4_or_the_oracle(engine, fx, eps, path):
    hard = D.case("hashed512", eps, fx)["caps"]["bp_tokens_per_frame"]
    _scan(engine, fx, eps, path, "bp_tokens_per_frame", (8, 32, 128, 512, 1024, hard), 4)


@pytest.mark.parametrize("eps", EPS)
def test_shrunk_capacity_overflows_with_the_hard_bounds_and_the_ladder_recovers(engine, fx, eps, monkeypatch):
    """From 2 881 states (1 921 with epsilon arcs) even the list-free tables exceed 160 KiB and the plan halves the token
    capacity: ``PackedGraphs.hard_bounds()`` can no longer rule status 3 out (its docstring says so).  The product ladder
    (``engine.redo_capacity``, here behind ``kalpy_api.GmmAligner.align_utterances``) then hands the utterance to the
    general decoder and delivers the oracle's alignment, words and likelihood."""
    from montreal_forced_aligner_amd import kalpy_api as KA

    c = D.case("shrink", eps, fx)
    tm, am, f, x = c["tm"], c["am"], c["fsts"][0], c["frames"][0]
    (beam, retry), = c["beams"]
    ref = D.refs("shrink", eps, fx, beam, retry)[0]
    assert ref["status"] == 0

    def shrunk(plan):
        assert plan[-1]["N"] < D.ceil64(f.num_states) and ref["max_toks"] > plan[-1]["N"], plan
    for path in PATHS:
        res, fo, g, _ = _decode(engine, c, [0], beam, retry, c["caps"], path, shrunk)
        assert tuple(c["caps"].values()) == g.hard_bounds()
        assert res["status"].tolist() == [3]                  # the promise hard_bounds cannot keep at this size
    al = KA.GmmAligner.__new__(KA.GmmAligner)
    al.acoustic_model_path = "mono"; al.transition_model, al.acoustic_model = tm, am
    al.beam, al.retry_beam = beam, retry
    al.transition_scale, al.acoustic_scale, al.self_loop_scale = 1.0, 0.1, 0.1
    al.disambiguation_symbols = []
    al._scaled = np.zeros_like(tm.scaled_log_probs(1.0, 0.1))      # (the graph is given with its weights in place)
    al._loaded = False
    monkeypatch.setattr(KA, "_ENGINE", engine)
    calls = []
    general = engine.align_general

    def counted(*a, **kw):
        calls.append(1)
        return general(*a, **kw)
    monkeypatch.setattr(engine, "align_general", counted)
    out = al.align_utterances([f], [x], ["big"])
    assert len(calls) == 1                                    # the last rung of the ladder: the general decoder
    assert out[0] is not None and out[0].alignment == ref["ali"].tolist() and out[0].words == ref["words"].tolist()
    assert np.float32(out[0].likelihood) == np.float32(ref["like"])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", EPS)
def test_score_rows_wider_than_the_row_cache_and_than_the_speculation_bitmap(engine, fx, eps, path):
    """A model of about 5 000 pdfs in one graph.  More than 512 score columns in an utterance: viterbi_kernel reads scores
    straight from HBM instead of a row staged in LDS; more than 2 048: the lazy path's first tier does not speculate (its
    bitmap of scored columns holds 2 048).  One graph on each side of 2 048, each a batch of its own."""
    c = D.case("wide_rows", eps, fx)
    seen = set()
    for u, (lo, hi) in enumerate(((2048, 1 << 30), (512, 2048))):
        caps = D.hard_bounds([c["fsts"][u]])
        for beam, retry in c["beams"]:
            codes = (-2,) if retry == 0.0 else (-2, -1)
            res, fo, g, _ = _decode(engine, c, [u], beam, retry, caps, path, _lists_in_hbm(codes, c["fsts"][u].num_states))
            cols = np.diff(g.pdf_off_host)
            assert cols.shape == (1,) and lo < int(cols[0]) <= hi, cols
            assert int(cols[0]) == D.column_count(c["fsts"][u], c["tm"])
            seen.add(_equals_oracle(res, fo, 0, D.refs("wide_rows", eps, fx, beam, retry)[u]))
    assert 0 in seen
