"""fMLLR statistics on the device (csrc/fmllr.hip: fmllr_frame_kernel, fmllr_spk_kernel, the transition-id lookup and the
state mfa_fmllr_acc_batch keeps in the context) against the oracle AND against the float64 restatement
(oracle.np_oracle.fmllr_acc), over feature dims 8 – 41, pdfs of 1 – 128 Gaussians, utterance lengths around the 64-frame
chunks, speaker lists of every kind, frame weights, hard posteriors, a 60 000-frame speaker; what holds exactly (symmetry,
zero speakers, the summation order per speaker); the refusals; the statistics through both solvers; and a muted speaker
through CorpusAligner.

The bound.  Device and oracle form a_t and b_t with the same float32 fmaf chains in ascending Gaussian order on the same
float32 log-likelihoods; they differ in the softmax only (tree sum against sequential sum, the device's expf against
libm's).  The unit of error is ε32·S, S the sum of the absolute values of the terms of the same sum (np_oracle.fmllr_acc
returns it).  The oracle's own worst distance from the float64 restatement over every case of this module (the grid of
helpers.fmllr_case_names() and the two fixture cases of test_gpu_parity / test_gpu_alimdl_flow) is measured on the CPU by
tests/test_fmllr_cpu.py::test_oracle_accumulation_against_float64_over_the_device_grid, which prints it and fails when it
moves; the device is allowed four times that: an exponential some 1.5 ulp coarser than libm's and another summation tree over
at most 128 terms are float32 pipelines of the same length as the oracle's.  Against the oracle itself, with which it shares
everything but the softmax, the device is held to a bound derived from those differences (DEVICE_VS_ORACLE below)."""
import functools

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import fmllr as F
from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.engine import AlignmentEngine, fmllr_statistics
from oracle import np_oracle as N
from oracle import oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu

# oracle − float64 in units of ε32·S, worst over the grid: β 3.00, K 219.60, G 148.37, all three at the 300 one-utterance
# speakers of 1 – 11 frames, where nothing averages out (60 000 frames: β 0.05, K 14.6, G 17.1).  Measured on the CPU, kept in
# tests/helpers.py so that the CPU test that measures them needs nothing of the device stack.
ORACLE_BETA, ORACLE_K, ORACLE_G = helpers.FMLLR_ORACLE_BETA, helpers.FMLLR_ORACLE_K, helpers.FMLLR_ORACLE_G
# 1. what the device may be away from the float64 restatement in any case: 4 × that (12.0 / 878.4 / 593.5)
DEVICE_BETA, DEVICE_K, DEVICE_G = 4 * ORACLE_BETA, 4 * ORACLE_K, 4 * ORACLE_G
# 2. K and G of every case are also held to 4 × the oracle's distance IN THAT CASE (computed beside the expectation): the
#    oracle's distance is the float32 rounding of the log-likelihoods, which the device shares bit for bit, so a speaker of
#    60 000 frames is held to 4 × 14.6 / 17.1 and not to the short speakers' 878 / 594.  (Not β: the oracle's β is a sum of
#    float32 counts whose distance from Σw is a random walk of roundings — 0.02 in one case, 0.2 in the next — and says
#    nothing about a second pipeline; β is held by 1 and 3.)
CASE_FACTOR = 4.0
# 3. device − oracle.  Both hold the same float32 log-likelihoods; per frame of n ≤ 128 Gaussians they differ by
#      exp: libm ≤ 1 ulp, device ≤ 2.5 ulp (1.5 coarser)                                     3.5 ε32 on a posterior
#      Σ exp: sequential over n − 1 additions against a 7-level tree, roundings of ½ ulp accumulating as a random walk
#             (√127 + √7) / 2                                                                 7.0
#      1/Σ, · inv, · weight: three roundings of ½ ulp on either side                          3.0
#      a_t, b_t (and the count): two fmaf chains of n terms fed posteriors that differ, each a random walk of ½-ulp
#             roundings relative to the absolute sum: 2 · √128 / 2                            11.3
#    together 24.8 ε32·S for a speaker of one frame at n = 128; over more frames the random parts shrink and the exp bias
#    stays.  25 for β, K and G alike.  A float32 running sum over the frames of a long speaker would drift by the order of
#    √T·ε32·S and more on the one-signed G entries (T = 60 000: hundreds), which this bound does not let through.
DEVICE_VS_ORACLE = 25.0
# end to end (statistics → solve → float32 W), |W − W of the restatement| in ulp of max|W| (ε32·max|W|), worst speaker of
# shape-D{39,40,41}-{one,two}: the oracle chain is 44.69 away (measured on the CPU by test_fmllr_cpu.py::
# test_oracle_chain_through_the_solver; the speakers of ~170 frames at D = 41, whose G_d are poorly conditioned and carry
# the statistics' error into W some tenfold; ~950 frames: 3 – 5); the device chain may be 4 × that plus one ulp for its
# stored result
ORACLE_W = helpers.FMLLR_ORACLE_W
DEVICE_W = 4 * ORACLE_W + 1.0


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


@functools.lru_cache(maxsize=None)
def _grid(name):
    case = helpers.fmllr_case(name)
    return (case,) + helpers.fmllr_expected(case)


def device_statistics(engine, case, load=True):
    if load:
        engine.load_gmm(case["am"])
    return fmllr_statistics(engine, _dev(engine, case["feats"]), case["frame_off"], _dev(engine, case["ali"]), case["tm"],
                            case["utt2spk"], case["sil_phones"], case["silence_weight"], stats_model=case["stats_am"])


def check_statistics(case, got, expected=None, what=""):
    """Device statistics of ``case`` against the float64 restatement (DEVICE_* and CASE_FACTOR) and against the oracle
    (DEVICE_VS_ORACLE); everything that holds exactly.  Returns the worst figures (β, K, G) against the restatement and against the oracle."""
    ids, orc, ref = expected if expected is not None else helpers.fmllr_expected(case)
    d_ids, beta, K, G = got
    assert np.array_equal(d_ids, ids)
    D = case["feats"].shape[1]
    assert beta.shape == (len(ids),) and K.shape == (len(ids), D, D + 1) and G.shape == (len(ids), D, D + 1, D + 1)
    assert np.isfinite(beta).all() and np.isfinite(K).all() and np.isfinite(G).all(), what
    assert np.array_equal(G, np.transpose(G, (0, 1, 3, 2))), f"{what}: G is not bit-symmetric"
    worst, case_fig = np.zeros((2, 3)), np.zeros(3)
    for k in range(len(ids)):
        r, o = ref[k], orc[k]
        if r["S_beta"] == 0:                                  # no weighted frame: exactly nothing
            assert beta[k] == 0 and not K[k].any() and not G[k].any(), (what, ids[k])
        d64 = helpers.fmllr_distance((beta[k], K[k], G[k]), r)
        dor = helpers.fmllr_distance((beta[k], K[k], G[k]), dict(r, beta=o[0], K=o[1], G=o[2]))
        worst = np.maximum(worst, [d64, dor])
        case_fig = np.maximum(case_fig, helpers.fmllr_distance(o, r))
        # the offset column: K[d, D] = Σ_t a_t[d] and G[d, D, D] = Σ_t b_t[d]
        for got_c, ref_c, s_c, lim in ((K[k][:, D], r["K"][:, D], r["SK"][:, D], DEVICE_K),
                                       (G[k][:, D, D], r["G"][:, D, D], r["SG"][:, D, D], DEVICE_G)):
            assert (np.abs(got_c - ref_c) <= lim * helpers.EPS32 * s_c).all(), (what, ids[k])
    name = what or case["name"]
    print(f"{name}: device - float64 in eps32*S: beta {worst[0][0]:.2f} K {worst[0][1]:.2f} G {worst[0][2]:.2f}; "
          f"device - oracle: beta {worst[1][0]:.2f} K {worst[1][1]:.2f} G {worst[1][2]:.2f}; "
          f"oracle - float64 in this case: beta {case_fig[0]:.2f} K {case_fig[1]:.2f} G {case_fig[2]:.2f}")
    assert worst[0][0] <= DEVICE_BETA and worst[0][1] <= DEVICE_K and worst[0][2] <= DEVICE_G, (name, worst)
    assert worst[0][1] <= CASE_FACTOR * case_fig[1] and worst[0][2] <= CASE_FACTOR * case_fig[2], (name, worst, case_fig)
    assert (worst[1] <= DEVICE_VS_ORACLE).all(), (name, worst)
    return worst


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _reordered(case, order):
    """The case with its utterances in another order (or a subset of them)."""
    fo = case["frame_off"]
    rows = np.concatenate([np.arange(fo[u], fo[u + 1]) for u in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    return dict(case, feats=case["feats"][rows], ali=case["ali"][rows], utt2spk=case["utt2spk"][list(order)],
                frame_off=np.concatenate([[0], np.cumsum([fo[u + 1] - fo[u] for u in order])]).astype(np.int64))


# ---- the grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", helpers.fmllr_case_names())
def test_statistics_over_the_grid(engine, name):
    case, ids, orc, ref = _grid(name)
    pdf, w = helpers.fmllr_frame_weights(case)
    if not name.startswith("spk"):          # the second round of the frame kernel (lanes 64 – 127) really is checked
        big = [p for p, n in enumerate(case["sizes"]) if n > 64]
        assert big and all(w[pdf == p].sum() >= 50 for p in big)
    got = device_statistics(engine, case)
    check_statistics(case, got, (ids, orc, ref))
    assert _same(got, device_statistics(engine, case, load=False)), "two runs of the same call differ"
    if name == "spk-mixed":
        assert ids.tolist() == [3, 12, 44, 907, 5000]
        for k in (0, 2):                    # 3: silence and unaligned frames only; 44: utterances without frames
            assert got[1][k] == 0 and not got[2][k].any() and not got[3][k].any()
    if name.startswith("hard"):
        assert all(r["S_beta"] > 100 for r in ref)


@pytest.mark.parametrize("name", ["shape-D41-two", "spk-mixed", "shape-D39-one"])
def test_a_speakers_sums_do_not_depend_on_the_batch_around_it(engine, name):
    """The summation order per speaker is fixed (its utterances in batch order, frames in order): alone, inside the batch, or
    with the other speakers' utterances shuffled around its own, a speaker's β, K and G are the same bits.  Its own
    utterances in another order give another rounding of the same sums."""
    case, ids, orc, ref = _grid(name)
    rng = np.random.default_rng(9)
    _, beta, K, G = device_statistics(engine, case)
    n_utt = len(case["utt2spk"])
    for k, s in enumerate(ids):
        own = np.nonzero(case["utt2spk"] == s)[0]
        alone = device_statistics(engine, _reordered(case, own), load=False)
        assert alone[0].tolist() == [s] and _same((beta[k], K[k], G[k]), (alone[1][0], alone[2][0], alone[3][0])), (name, s)
        others = rng.permutation(np.setdiff1d(np.arange(n_utt), own))
        slots = np.sort(rng.choice(n_utt, size=len(own), replace=False))      # where its own utterances go, in their order
        order = np.zeros(n_utt, np.int64)
        order[slots] = own
        order[np.setdiff1d(np.arange(n_utt), slots)] = others
        mixed = device_statistics(engine, _reordered(case, order), load=False)
        assert _same((beta[k], K[k], G[k]), (mixed[1][k], mixed[2][k], mixed[3][k])), (name, s)
    turned = _reordered(case, np.arange(n_utt)[::-1])
    check_statistics(turned, device_statistics(engine, turned, load=False), (ids, orc, ref), what=f"{name}, utterances reversed")


@pytest.mark.parametrize("sw", ["0.0", "0.5", "1.0"])
def test_ids_without_weight_contribute_nothing(engine, sw):
    """Transition-id 0, negative ids and ids beyond the table are guarded by the lookup (weight 0, pdf −1): replacing them —
    and, at silence_weight 0, the silence frames — by 0 changes no bit.  The largest valid id is in the alignment."""
    case, ids, orc, ref = _grid(f"weights-{sw}")
    tm, ali = case["tm"], case["ali"]
    n_tids = tm.id2pdf.shape[0]
    bad = (ali <= 0) | (ali >= n_tids)
    assert (ali < 0).any() and (ali == 0).any() and (ali == n_tids).any() and (ali > n_tids).any() and (ali == n_tids - 1).any()
    got = device_statistics(engine, case)
    clean = np.where(bad, 0, ali).astype(np.int32)
    if float(sw) == 0.0:
        clean = np.where(~bad & np.isin(tm.id2phone[np.where(bad, 0, ali)], case["sil_phones"]), 0, clean).astype(np.int32)
    assert _same(got, device_statistics(engine, dict(case, ali=clean), load=False))
    # the weights are used: silence frames at weight w count w
    pdf, w = helpers.fmllr_frame_weights(case)
    for k, s in enumerate(ids):
        rows = np.concatenate([np.arange(case["frame_off"][u], case["frame_off"][u + 1]) for u in np.nonzero(case["utt2spk"] == s)[0]])
        assert abs(got[1][k] - float(w[rows].sum())) <= DEVICE_BETA * helpers.EPS32 * float(w[rows].sum())
    assert sorted(set(w.tolist())) == sorted({0.0, float(sw), 1.0})


# ---- state carried in the context ------------------------------------------------------------------------------------------
def _fresh(case):
    e = AlignmentEngine(0)
    try:
        return device_statistics(e, case)
    finally:
        e.close()


def _frames(case, n):
    """The first utterances of a case cut to n frames in all."""
    fo = np.minimum(case["frame_off"], n)
    return dict(case, feats=case["feats"][:n], ali=case["ali"][:n], frame_off=fo)


def test_workspace_regrown_between_calls(engine):
    """200 frames, then 50 000 (the per-frame workspace is freed and grown), then the 200 again."""
    big = _grid("long")[0]
    small, large = _frames(big, 200), _frames(big, 50000)
    first = device_statistics(engine, small)
    second = device_statistics(engine, large, load=False)
    third = device_statistics(engine, small, load=False)
    assert _same(first, third)
    assert _same(second, _fresh(large)) and _same(first, _fresh(small))
    check_statistics(large, second, what="50 000 frames after 200")


def _second_layout_case():
    """40 pdfs whose first 16 have other sizes than FMLLR_SIZES: each the next larger one, so that a row count left over
    from that model would drop Gaussians and never reach beyond a pdf's own rows.  The frames are aligned to those 16."""
    rng = np.random.default_rng(31)
    sizes = list(helpers.FMLLR_SIZES[1:]) + [128] + [int(n) for n in rng.integers(8, 65, size=24)]
    am = helpers.random_gmm(rng, 40, sizes)
    pdfs = rng.permutation(np.repeat(np.arange(16), 40)).astype(np.int32)
    T = len(pdfs)
    return dict(name="second layout", am=am, stats_am=None, tm=helpers.fmllr_tm(len(sizes)), sil_phones=[3], silence_weight=0.0,
                feats=helpers.fmllr_draw(rng, am, pdfs), ali=(2 * pdfs + 1).astype(np.int32), sizes=sizes,
                frame_off=np.array([0, 100, 164, T], np.int64), utt2spk=np.array([1, 0, 1]))


def test_rows_per_pdf_follow_the_loaded_model(engine):
    """The rows-per-pdf table is built on first use and belongs to the loaded model: 16 pdfs, accumulate, 40 pdfs of other
    sizes, accumulate — as a fresh engine does."""
    first, second = _grid("shape-D40-one")[0], _second_layout_case()
    assert len(first["sizes"]) == 16 and all(b > a for a, b in zip(first["sizes"][:15], second["sizes"][:15]))
    a = device_statistics(engine, first)
    b = device_statistics(engine, second)
    check_statistics(second, b)
    assert _same(b, _fresh(second))
    assert _same(a, device_statistics(engine, first))


def test_two_model_form_comes_and_goes(engine):
    """two-model → single-model → two-model on one engine, each as on a fresh engine; and after load_gmm a statistics model
    left over from the previous model is not used."""
    two = _grid("shape-D40-two")[0]
    one = dict(two, stats_am=None)
    other = dict(two, stats_am=helpers.fmllr_second_model(np.random.default_rng(8), two["am"]))
    r2, r1, r3 = device_statistics(engine, two), device_statistics(engine, one, load=False), device_statistics(engine, other, load=False)
    r2b = device_statistics(engine, two, load=False)
    f2, f1, f3 = _fresh(two), _fresh(one), _fresh(other)
    assert _same(r2, f2) and _same(r1, f1) and _same(r3, f3) and _same(r2b, f2)
    assert not _same(r2, r1) and not _same(r2, r3)
    check_statistics(one, r1)
    # (d) the statistics model is set; load_gmm; accumulate through the library without naming a statistics model
    device_statistics(engine, two)
    engine.load_gmm(two["am"])
    tm = two["tm"]
    id2pdf = _dev(engine, np.maximum(tm.id2pdf, 0).astype(np.int32))
    w_tid = np.where(np.isin(tm.id2phone, two["sil_phones"]), 0.0, 1.0).astype(np.float32)
    w_tid[0] = 0.0
    T, D = two["feats"].shape
    spk, inv = np.unique(two["utt2spk"], return_inverse=True)
    feats, ali, fo = _dev(engine, two["feats"]), _dev(engine, two["ali"]), _dev(engine, two["frame_off"])
    d_w, pdf, wgt = _dev(engine, w_tid), torch.empty(T, dtype=torch.int32, device=engine.device), torch.empty(T, dtype=torch.float32, device=engine.device)
    so = _dev(engine, np.concatenate([[0], np.cumsum(np.bincount(inv))]).astype(np.int32))
    su = _dev(engine, np.argsort(inv, kind="stable").astype(np.int32))
    beta = torch.zeros(len(spk), dtype=torch.float64, device=engine.device)
    K = torch.zeros((len(spk), D, D + 1), dtype=torch.float64, device=engine.device)
    G = torch.zeros((len(spk), D, D + 1, D + 1), dtype=torch.float64, device=engine.device)
    rc = engine.lib.mfa_fmllr_acc_ali_batch(engine.ctx, feats.data_ptr(), fo.data_ptr(), len(two["frame_off"]) - 1, T, ali.data_ptr(),
                                             id2pdf.data_ptr(), d_w.data_ptr(), int(id2pdf.shape[0]), pdf.data_ptr(), wgt.data_ptr(),
                                             so.data_ptr(), su.data_ptr(), len(spk), beta.data_ptr(), K.data_ptr(), G.data_ptr())
    assert rc == 0
    assert _same((spk, beta.cpu().numpy(), K.cpu().numpy(), G.cpu().numpy()), f1)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _tiny_case(D, sizes, seed=2):
    rng = np.random.default_rng(seed)
    am = helpers.random_gmm(rng, D, sizes)
    pdfs = rng.integers(0, len(sizes), size=150).astype(np.int32)
    return dict(name=f"tiny D{D}", am=am, stats_am=None, tm=helpers.fmllr_tm(len(sizes)), sil_phones=[], silence_weight=0.0,
                feats=helpers.fmllr_draw(rng, am, pdfs), ali=(2 * pdfs + 1).astype(np.int32), sizes=sizes,
                frame_off=np.array([0, 70, 150], np.int64), utt2spk=np.array([0, 1]))


def test_refusals_name_their_cause_and_leave_the_engine_usable(engine):
    good = _tiny_case(41, [3, 128, 65])
    before = device_statistics(engine, good)
    check_statistics(good, before)

    def still_good():
            assert _same(before, device_statistics(engine, good))

    # nothing to do is no error: no utterance, no speaker, no frame
    none = device_statistics(engine, dict(good, feats=good["feats"][:0], ali=good["ali"][:0], frame_off=np.zeros(1, np.int64),
                                          utt2spk=np.zeros(0, np.int64)))
    assert none[1].shape == (0,) and none[2].shape == (0, 41, 42) and none[3].shape == (0, 41, 42, 42)
    still_good()
    for D in (42, 48):                                        # the speaker kernel tiles (D+1)² ≤ 7·256 entries: D ≤ 41
        with pytest.raises(MfaHipError, match=rf"feature dim {D} > 41"):
            device_statistics(engine, _tiny_case(D, [3, 5]))
        still_good()
    with pytest.raises(MfaHipError, match=r"pdf 1 has more than 128 Gaussians"):
        device_statistics(engine, _tiny_case(40, [3, 129, 5]))
    still_good()
    other_layout = helpers.random_gmm(np.random.default_rng(3), 41, [3, 127, 65])
    with pytest.raises(MfaHipError, match=r"pdf 1 has 127 Gaussians, the loaded \(alignment\) model 128"):
        device_statistics(engine, dict(good, stats_am=other_layout))
    still_good()
    other_dim = helpers.random_gmm(np.random.default_rng(3), 40, [3, 128, 65])
    with pytest.raises(MfaHipError, match=r"3 pdfs of dim 40, loaded model has 3 of dim 41"):
        device_statistics(engine, dict(good, stats_am=other_dim))
    still_good()


# ---- end to end: statistics → solve ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"shape-D{d}-{form}" for d in (39, 40, 41) for form in ("one", "two")])
def test_device_statistics_through_the_solver(engine, name):
    """Device statistics → compute_fmllr and oracle statistics → O.fmllr_solve, both against the float64 restatement's solve
    of its own statistics: the device chain at most DEVICE_W ulp of max|W| away (the oracle chain: ORACLE_W, asserted here
    too — the figure is the CPU's)."""
    case, ids, orc, ref = _grid(name)
    _, beta, K, G = device_statistics(engine, case)
    for k in range(len(ids)):
        W64, impr = N.fmllr_solve(ref[k]["beta"], ref[k]["K"], ref[k]["G"], min_count=100.0)
        Wd, impr_d = F.compute_fmllr(beta[k], K[k], G[k], min_count=100.0)
        Wo, impr_o = O.fmllr_solve(*orc[k], min_count=100.0)
        assert impr > 0 and impr_d > 0 and impr_o > 0
        ulp = helpers.EPS32 * float(np.abs(W64).max())
        dd, do = float(np.abs(Wd - W64).max()) / ulp, float(np.abs(Wo - W64).max()) / ulp
        print(f"{name} speaker {ids[k]}: |W - W64| in ulp of max|W|: device chain {dd:.2f}, oracle chain {do:.2f}")
        assert do <= ORACLE_W and dd <= DEVICE_W


# ---- a muted speaker through CorpusAligner ---------------------------------------------------------------------------------
from tests.test_gpu_corpus_pipeline import setup  # noqa: E402,F401  (the triphone LDA+fMLLR setup, as a fixture here)


def test_a_muted_speaker_costs_its_own_transform_only(engine, setup):
    """One speaker's channel is muted: digital silence, constant MFCCs, constant features after CMVN and LDA, G_d of rank 1.
    Its transcripts are long enough for ≥ fmllr_min_count non-silence frames, so the solver is reached.  The corpus must
    complete, that speaker must keep the transform it came with (identity), be listed in ``fmllr_rejected``, and every other
    speaker's transform (bit for bit), alignments, words and likelihoods must be those of the run without it."""
    from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance

    s = setup
    utts = list(s["utts"][:40])          # ten voiced utterances a speaker (the 41st cannot be aligned: left out)
    prev = s["prev"]
    # digital silence scores far better on the silence pdfs than on any word's, frame after frame: the path through the words
    # falls behind the best token by more than any ordinary retry beam.  The retry beam is opened for both runs (the graphs
    # are a few hundred states; the voiced utterances align with the first beam as before).
    m = s["model"]

    def aligner():
        return CorpusAligner(m.tm, m.am, m.tree, s["world"].lexicon, lda=s["lda"], engine=engine,
                             options=AlignOptions(beam=10.0, retry_beam=1.0e5), silence_phones=s["sil"])

    al = aligner()
    base = al.align(utts, speaker_adapted=True, make_ctm=False, previous_transforms=prev)
    base_W, base_failed = al.transforms.copy(), list(al.failed)
    assert al.fmllr_rejected == [] and base_failed == []
    # estimates, not the transforms the speakers came with: equal bits below mean equal estimates
    assert all(np.abs(base_W[k][:, :40] - prev[k][:, :40]).max() > 1e-3 for k in range(4))
    muted = []
    for i in range(10):
        _pcm, text, _segs, _ = s["world"].utterance(43000 + i, n_words=30, samples=96000, speaker=7)
        muted.append(CorpusUtterance(f"mute-{i}", "mute", np.zeros(96000, np.int16), text))
    prev5 = np.concatenate([prev, np.eye(40, 41, dtype=np.float32)[None]])
    al2 = aligner()
    res = al2.align(utts + muted, speaker_adapted=True, make_ctm=False, previous_transforms=prev5)
    assert al2.failed == [], al2.failure_reasons
    tm = s["model"].tm
    voiced = sum(int((~np.isin(tm.id2phone[r.alignment], s["sil"])).sum()) for r in res[len(utts):])
    assert voiced >= al2.opt.fmllr_min_count, voiced            # the count did not stop the solver: the statistics did
    assert al2.fmllr_rejected == ["mute"]
    W = al2.transforms
    assert np.isfinite(W).all() and np.array_equal(W[4], np.eye(40, 41, dtype=np.float32))
    assert W[:4].tobytes() == base_W.tobytes()
    for k, (a, b) in enumerate(zip(base, res[: len(utts)])):
        assert np.array_equal(a.alignment, b.alignment) and np.array_equal(a.words, b.words), k
        assert np.float32(a.likelihood).tobytes() == np.float32(b.likelihood).tobytes(), k
