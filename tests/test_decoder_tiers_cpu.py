"""The large-graph decoder cases (tests/decoder_tier_cases.py) are what they claim to be — checked with the oracle and the
host-side launch plan alone, so that tests/test_gpu_decoder_tiers.py cannot pass by missing its tier.

For every case and its epsilon twin: the oracle produces the statuses the case needs, its peak live-token counts fall in
the intended ranges, the column counts do, and mfa_debug_viterbi_plan predicts the intended tier from the batch's largest
state and arc counts, its capacities and whether it holds epsilon arcs.  A seed that does not deliver is changed in the
cases module; the assertions here stay.
"""
import numpy as np
import pytest

from tests import decoder_tier_cases as D

EPS = [False, True]


def _plans(c, retry, caps=None, fsts=None):
    """(dense plan, lazy plan) of the case's batch."""
    fsts = c["fsts"] if fsts is None else fsts
    caps = c["caps"] if caps is None else caps
    return [D.batch_plan(fsts, lazy, retry, caps) for lazy in (0, 1)]


def _eps_share(c):
    return [float((f.arcs["ilabel"] == 0).mean()) for f in c["fsts"]]


@pytest.mark.parametrize("eps", EPS)
def test_twins_hold_epsilon_arcs_and_nothing_the_wavefront_decoder_refuses(fx, eps):
    from montreal_forced_aligner_amd.packing import GraphPacking
    from tests import helpers
    for name in D.CASES:
        c = D.case(name, eps, fx)
        assert len(c["fsts"]) <= 5 and len(c["fsts"]) == len(c["frames"])
        assert all(x.shape[0] <= 60 for x in c["frames"]) or name == "resume"
        for f in c["fsts"]:
            assert not GraphPacking.needs_general_decoder(f) and not helpers.has_negative_eps_cycle(f)
        if eps:
            assert D.has_eps(c["fsts"][:1]), name                      # the large graph itself
        else:
            assert not D.has_eps(c["fsts"]), name


@pytest.mark.parametrize("eps", EPS)
def test_hbm_case_runs_growth_and_retry_launches_with_lists_in_hbm(fx, eps):
    c = D.case("hbm", eps, fx)
    S = max(f.num_states for f in c["fsts"])
    assert c["fsts"][0].num_states == S == c["caps"]["max_tokens"] and (eps or S == 2600)
    assert [f.num_states for f in c["fsts"][1:]] == list(D.SMALL) or eps
    seen = set()
    for beam, retry in c["beams"]:
        for plan in _plans(c, retry):
            assert plan[0]["lists_in_lds"] == 1                         # the first tier is small
            for row in plan[1:]:                                        # growth launch, retry launch
                assert row["lists_in_lds"] == 0 and row["N"] == D.ceil64(S), row       # in HBM, and not shrunk
        r = D.refs("hbm", eps, fx, beam, retry)
        seen |= {x["status"] for x in r}
        if retry == 0.0:
            # the wide-beam point: the large graph aligns with more tokens than either first tier holds → growth launch
            assert r[0]["status"] == 0 and r[0]["max_toks"] > 128
        else:
            assert r[0]["status"] == 1                                  # the large graph needs the retry launch
    assert {0, 1} <= seen


@pytest.mark.parametrize("eps", EPS)
def test_hbm_default_case_needs_the_retry_launch_for_the_large_graph(fx, eps):
    c = D.case("hbm_default", eps, fx)
    assert c["caps"] == dict(max_tokens=1024, bp_tokens_per_frame=512)
    S = max(f.num_states for f in c["fsts"])
    for beam, retry in c["beams"]:
        assert retry != 0.0
        for plan in _plans(c, retry):
            assert [row["code"] for row in plan] == [0, -2, -1]
            assert plan[1]["lists_in_lds"] == 1 and plan[1]["N"] == 1024
            assert plan[2]["lists_in_lds"] == 0 and plan[2]["N"] == D.ceil64(min(4096, S))
        r = D.refs("hbm_default", eps, fx, beam, retry)
        assert r[0]["status"] == 1
        for x, feats in zip(r, c["frames"]):
            # the default capacities hold: what the device reports is the oracle's status, not an overflow
            assert x["max_toks"] <= 1024 and x["sum_toks"] <= 512 * feats.shape[0]


@pytest.mark.parametrize("eps", EPS)
def test_hashed512_case_fills_and_overflows_a_2048_bucket_table(fx, eps):
    c = D.case("hashed512", eps, fx)
    assert c["caps"]["max_tokens"] == 512 and c["fsts"][0].num_states >= 2600
    (fit, _), (over, _) = c["beams"]
    for plan in _plans(c, 0.0):
        assert len(plan) == 2 and plan[1]["code"] == -2
        assert plan[1]["N"] == 512 and plan[1]["hbits"] == 11           # the growth launch: 2 048 buckets
    r_fit, r_over = D.refs("hashed512", eps, fx, fit, 0.0)[0], D.refs("hashed512", eps, fx, over, 0.0)[0]
    assert r_fit["status"] == 0 and 128 < r_fit["max_toks"] <= 512
    assert r_over["status"] == 0 and r_over["max_toks"] > 512
    assert D.HASHED_SCAN_BEAM == fit


@pytest.mark.parametrize("eps", EPS)
def test_shrink_case_is_given_fewer_tokens_than_states_and_needs_more(fx, eps):
    c = D.case("shrink", eps, fx)
    S = c["fsts"][0].num_states
    assert S >= 3600 and c["caps"] == D.hard_bounds(c["fsts"]) and c["caps"]["max_tokens"] == S
    (beam, retry), = c["beams"]
    assert beam == 1.0e4 and retry == 0.0
    r = D.refs("shrink", eps, fx, beam, retry)[0]
    assert r["status"] == 0
    for plan in _plans(c, retry):
        assert plan[-1]["N"] < D.ceil64(S) and plan[-1]["lists_in_lds"] == 0
        assert r["max_toks"] > plan[-1]["N"]                            # the oracle's live tokens exceed the shrunk capacity


@pytest.mark.parametrize("eps", EPS)
def test_resume_case_crosses_a_list_pass_window_in_hbm(fx, eps):
    c = D.case("resume", eps, fx)
    S = c["fsts"][0].num_states
    assert c["frames"][0].shape[0] == 300 > 256                          # the list passes' window (align_impl: K = max(window, 256))
    lazy = _plans(c, 0.0)[1]
    assert lazy[1]["code"] == -2 and lazy[1]["lists_in_lds"] == 0 and lazy[1]["N"] == D.ceil64(S)
    for beam, retry in c["beams"]:
        r = D.refs("resume", eps, fx, beam, retry)[0]
        # more tokens than the lazy first tier (64) and the dense one (128) hold: the growth launch decodes all 300 frames
        assert r["status"] == 0 and 128 < r["max_toks"] <= S


@pytest.mark.parametrize("eps", EPS)
def test_wide_rows_case_has_the_column_counts_of_both_branches(fx, eps):
    c = D.case("wide_rows", eps, fx)
    tm = c["tm"]
    assert tm.num_pdfs > 2048 and int(np.diff(c["am"].pdf_offsets).max()) == 1
    wide, mid = (D.column_count(f, tm) for f in c["fsts"])
    assert wide > 2048, wide                                             # no speculation (the scored-column bitmap holds 2 048)
    assert 512 < mid <= 2048, mid                                        # score rows read from HBM, speculation on
    for k, f in enumerate(c["fsts"]):
        caps = D.hard_bounds([f])
        for beam, retry in c["beams"]:
            for plan in _plans(c, retry, caps, [f]):
                assert all(row["lists_in_lds"] == 0 and row["N"] == D.ceil64(f.num_states) for row in plan[1:])
    seen = set()
    for beam, retry in c["beams"]:
        r = D.refs("wide_rows", eps, fx, beam, retry)
        seen |= {x["status"] for x in r}
        assert all(x["status"] in (0, 1) for x in r)
        if retry == 0.0:
            assert all(x["max_toks"] > 128 for x in r)                   # the growth launch decodes both graphs
    assert 0 in seen
