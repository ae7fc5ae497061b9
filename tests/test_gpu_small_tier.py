"""viterbi_small_kernel<3, ·> — the 64-token first tier of ``align_features`` — against the oracle at the edges of its
envelope, bit for bit: 63 / 64 / 65 live tokens (at frame 1, across a window boundary, at the last frame), 64 … 193
candidates a frame with runs across the round boundaries, a 64-arc state, the min_active selection with ties on the 21st
smallest cost, Kaldi's list order with shared hash buckets, probe chains of the 256-entry slot table, the back-pointer
capacity met exactly, first passes that lose every token, every length around the 64-frame window, and the epsilon
instantiation.  The cases are tests/small_tier_cases.py's; tests/test_small_tier_cpu.py holds them to their claims with the
oracle alone, and every test here repeats those claims (``D.assert_claims``) and asks mfa_debug_viterbi_plan for the
batch's launches before it runs anything, so none passes by missing the kernel.

Outputs are compared as tests/test_gpu_decoder_tiers.py compares them: status through ``helpers.device_status``; ``ali``,
``words``, ``n_words``, ``like`` and ``frame_like`` equal to the oracle's.  No tolerances.  The same batch through
``engine.score`` + ``engine.align`` holds the dense path's 128-token tier to the same cases.
"""
import numpy as np
import pytest
import torch

from tests import decoder_tier_cases as T
from tests import small_tier_cases as D
from tests.test_gpu_decoder_tiers import KEYS, _dev, _equals_oracle, _same_utterance

pytestmark = pytest.mark.gpu

LOOKAHEADS = (None, "4", "63")      # MFA_LAZY_LOOKAHEAD: default (K / 2); nearly every window redone; speculation off


def _decode(engine, bt, idx, scale, path):
    """Cases ``idx`` of batch ``bt`` as one device batch through ``align_features`` ("lazy") or ``score`` + ``align``
    ("dense"), after the plan check: the lazy path starts with the 64-token tier and has a growth launch behind it."""
    cases = [bt["cases"][k] for k in idx]
    fsts, feats = [c["fst"] for c in cases], [c["feats"] for c in cases]
    engine.load_gmm(D.model())
    g = engine.pack_graphs(fsts, D.tm())
    assert g.has_eps == bool(bt.get("eps", False)) or len(idx) < len(bt["cases"])
    plan = T.plan(g.max_states, g.max_arcs, g.has_eps, path == "lazy", retry_beam=bt["retry"], **bt["caps"])
    if path == "lazy":
        assert plan[0]["N"] == 64 and plan[0]["code"] == 0 and plan[1]["code"] == -2, plan
    fo = np.concatenate([[0], np.cumsum([x.shape[0] for x in feats])]).astype(np.int64)
    d_feats = _dev(engine, np.concatenate(feats))
    kw = dict(beam=bt["beam"], retry_beam=bt["retry"], acoustic_scale=scale, want_frame_likes=True, **bt["caps"])
    if path == "dense":
        ll, ll_off, ll_cols = engine.score(d_feats, fo, g.pdf_list, g.pdf_off_host, g.class_counts)
        res = engine.align(g, ll, ll_off, ll_cols, fo, **kw)
    else:
        res = engine.align_features(g, d_feats, fo, **kw)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}, fo


def _look(monkeypatch, look):
    if look is None:
        monkeypatch.delenv("MFA_LAZY_LOOKAHEAD", raising=False)
    else:
        monkeypatch.setenv("MFA_LAZY_LOOKAHEAD", look)


def _all_equal_oracle(name, res, fo, scale, what):
    bt = D.batch(name)
    seen = []
    for u, c in enumerate(bt["cases"]):
        try:
            seen.append(_equals_oracle(res, fo, u, D.ref(name, u, scale)))
        except AssertionError as e:
            raise AssertionError(f"{name}/{c['name']} ({what}, scale {scale}): {e}") from e
    return seen


@pytest.mark.parametrize("name", [n for n in D.NAMES if n != "back_pointers"])
def test_family_equals_the_oracle_on_both_paths(engine, monkeypatch, name):
    """Every case of the family, at every acoustic scale of the family: the lazy path (small tier first) and the dense path
    (128-token tier first) give the oracle's status, alignment, words, likelihood and per-frame likelihoods."""
    _look(monkeypatch, None)
    bt = D.batch(name)
    idx = list(range(len(bt["cases"])))
    for scale in bt["scales"]:
        D.assert_claims(name, scale)
        for path in ("lazy", "dense"):
            res, fo = _decode(engine, bt, idx, scale, path)
            seen = _all_equal_oracle(name, res, fo, scale, path)
        if name == "dying_out":
            assert sorted(set(seen)) == [1, 2]
        elif name == "mixed":
            assert sorted(set(seen)) == [0, 1, 2]
        elif name == "random_ties":
            assert set(seen) <= {0, 1} and 0 in seen
        else:
            assert set(seen) == {0}


@pytest.mark.parametrize("name", D.LAG_FAMILIES)
def test_family_gives_the_same_bits_under_every_lookahead(engine, monkeypatch, name):
    """MFA_LAZY_LOOKAHEAD unset, 4 (nearly every window fails its speculation and is redone one window later, window 0
    included) and 63 (no speculation): the oracle's bits under all three."""
    bt = D.batch(name)
    idx = list(range(len(bt["cases"])))
    D.assert_claims(name, 1.0)
    base = None
    for look in LOOKAHEADS:
        _look(monkeypatch, look)
        res, fo = _decode(engine, bt, idx, 1.0, "lazy")
        _all_equal_oracle(name, res, fo, 1.0, f"look-ahead {look}")
        if base is None:
            base = res
        else:
            for k in KEYS:
                assert np.array_equal(base[k], res[k]), (k, look)


def test_back_pointer_capacity_met_exactly_keeps_the_utterance(engine, monkeypatch):
    """T · bp_tokens_per_frame records exactly: the small tier keeps the utterance and the result is the oracle's.  One
    record more: the tier hands over, and the status is 4 or the oracle's result, as in
    test_back_pointer_capacity_scan_is_status_4_or_the_oracle."""
    _look(monkeypatch, None)
    name = "back_pointers"
    bt = D.batch(name)
    D.assert_claims(name, 1.0)
    cap = D.BP_T * bt["caps"]["bp_tokens_per_frame"]
    assert [c["records"] - cap for c in bt["cases"]] == [0, 0, 1, 1]
    for path in ("lazy", "dense"):
        res, fo = _decode(engine, bt, [0, 1, 2, 3], 1.0, path)
        for u in (0, 1):
            assert _equals_oracle(res, fo, u, D.ref(name, u)) == 0, (path, u)
        for u in (2, 3):
            print(f"{path}: {bt['cases'][u]['name']} status {int(res['status'][u])}")
            if int(res["status"][u]) != 4:
                assert _equals_oracle(res, fo, u, D.ref(name, u)) == 0, (path, u)


def test_mixed_batch_utterances_decode_alone_as_in_the_batch(engine, monkeypatch):
    """Utterances that finish, hand over, die and lag in different windows share one batch; each of them decoded alone
    gives the same bits."""
    _look(monkeypatch, None)
    bt = D.batch("mixed")
    D.assert_claims("mixed", 1.0)
    env = D.envelope("mixed")
    assert sum(not e["inside"] for e in env) >= 3 and sum(e["dies"] for e in env) == 3
    res, fo = _decode(engine, bt, list(range(len(bt["cases"]))), 1.0, "lazy")
    for u, c in enumerate(bt["cases"]):
        alone, fo1 = _decode(engine, bt, [u], 1.0, "lazy")
        _same_utterance(res, fo, u, alone, fo1, 0, c["name"])
