"""The inputs of the fine-tuning stage tests (tests/test_gpu_finetune_stages.py) reach every branch of fine-tuning: shown
here on the sequential oracle-only reference (tests/finetune_ref.py), without a GPU.  These are conditions on the inputs,
not measurements of the code under test: were one of them to fail, the GPU tests would still pass but prove less.  The host
pieces of finetune.py (window planning, assembly with the repair loop, labels) are checked against the reference's."""
import numpy as np
import pytest

from montreal_forced_aligner_amd import finetune as FT
from tests import finetune_ref as R


def _alis(out):
    return {k: o.ali for k, o in enumerate(out) if o.ali is not None}


def _same_windows(a, b):
    key = lambda w: (w.utt, w.index, w.feature_begin, w.feature_end, w.begin_offset, w.end_offset, w.prev_phone, w.phone)  # noqa: E731
    return [key(w) for w in a] == [key(w) for w in b]


def _seen(intervals, w):
    return {int(iv.symbol) for iv in intervals[w.utt]}


def test_two_speakers_cannot_be_confused(fx):
    """A wrong speaker index shifts a window's static features by the difference of the speakers' CMVN offsets: in every
    cepstral column that is more than a thousand times the bar the features are held to."""
    batch = R.mono_batch(fx)
    diff = np.abs(np.diff(R.speaker_offsets(batch.spk_stats), axis=0))[0]
    print("speaker CMVN offsets differ by", diff.round(3))
    assert diff.min() > 1000 * R.FEATURE_BAR
    assert sorted(set(batch.utt2spk)) == [0, 1] and list(batch.utt2spk) != sorted(batch.utt2spk)


@pytest.mark.parametrize("snip_edges", [0, 1])
def test_groups_reach_fallback_failure_and_unseen_labels(fx, snip_edges):
    cfg = R.mono_config(fx, "groups40")
    windows, out = R.mono_reference(fx, "groups40", snip_edges)
    assert len(windows) == 86 and _same_windows(windows, FT.plan_windows(cfg["intervals"], [len(x) / R.SR for x in R.mono_batch(fx).pcm]))
    fallback = [k for k, o in enumerate(out) if o.scale == 0.1]
    failed = [k for k, o in enumerate(out) if o.failed and o.rows >= 6]
    unseen = [k for k, (w, o) in enumerate(zip(windows, out)) if not o.failed and o.label not in _seen(cfg["intervals"], w)]
    print(f"snip_edges={snip_edges}: {len(fallback)} windows aligned at 0.1 only, {len(failed)} at neither scale, "
          f"{len(unseen)} tuned phones occur nowhere else in their utterance")
    assert fallback and failed and unseen
    assert any(o.scale == 1.0 for o in out)
    for k in failed:                         # a failed window keeps its boundary and its phone
        iv = cfg["intervals"][windows[k].utt][windows[k].index]
        assert (out[k].boundary, out[k].label) == (iv.begin, int(iv.symbol))
    # the graphs stay small enough for a quick device test, and are the sizes nothing else decodes
    states = {FT.two_phone_graph(fx.mono_gc, cfg["group"](w.prev_phone), cfg["group"](w.phone)).num_states for w in windows[:20]}
    assert 8 <= min(states) and max(states) <= 500, states
    # labels: through the phone table every label is a name; without it an unseen phone stays an id
    named, _ = R.assemble(windows, cfg["intervals"], _alis(out), fx.mono_tm, fx.mono_lex.phone_table)
    bare, _ = R.assemble(windows, cfg["intervals"], _alis(out), fx.mono_tm)
    assert all(isinstance(lab, str) and lab == fx.mono_lex.phone_table.find(p) for ivs in named for _b, _e, lab, p in ivs)
    assert any(isinstance(lab, int) for ivs in bare for _b, _e, lab, _p in ivs)


@pytest.mark.parametrize("snip_edges", [0, 1])
def test_identity_groups_never_fall_back(fx, snip_edges):
    """min_active keeps the 8-state graph alive at any beam: fallbacks need real groups."""
    windows, out = R.mono_reference(fx, "identity", snip_edges)
    assert all(o.scale == 1.0 for o in out)
    moved = sum(o.boundary != R.mono_config(fx, "identity")["intervals"][w.utt][w.index].begin for w, o in zip(windows, out))
    assert moved > len(windows) // 2
    truncated = [k for k, o in enumerate(out) if o.truncated]
    # snip_edges=1: the cut of a boundary 30 ms before the utterance's end has fewer frames than the window's last row
    assert (len(truncated) >= 1) if snip_edges else not truncated
    for k in truncated:
        assert 6 <= out[k].rows < int(round((windows[k].end_offset - windows[k].begin_offset) * 1000))


@pytest.mark.parametrize("snip_edges", [0, 1])
def test_squeezed_intervals_reach_the_repair_loop(fx, snip_edges):
    cfg = R.mono_config(fx, "squeezed")
    windows, out = R.mono_reference(fx, "squeezed", snip_edges)
    ivs, dels = R.assemble(windows, cfg["intervals"], _alis(out), fx.mono_tm, fx.mono_lex.phone_table)
    print(f"snip_edges={snip_edges}: deleted {dels}")
    assert all(len(d) >= 1 for d in dels)
    for u, (a, d) in enumerate(zip(ivs, dels)):
        assert len(a) + len(d) == len(cfg["intervals"][u])
        assert all(x[1] == y[0] for x, y in zip(a[:-1], a[1:])) and all(x[0] < x[1] for x in a)
    if snip_edges:
        assert any(o.truncated for o in out)
    # finetune.assemble (what fine_tune_boundaries ends in) against the restatement, on the same alignments
    got_iv, got_del = FT.assemble(windows, cfg["intervals"], _alis(out), fx.mono_tm, fx.mono_lex.phone_table)
    assert R.as_tuples(got_iv) == ivs and got_del == dels


def test_repair_restatements_agree_on_a_cascade():
    """Deleting an interval opens a gap that empties its neighbour on the next round."""
    m = [dict(id=0, begin=0.0, end=0.1), dict(id=1, begin=0.3, end=0.2), dict(id=2, begin=0.2, end=0.25),
         dict(id=3, begin=0.25, end=0.25), dict(id=4, begin=0.25, end=0.4)]
    a, da = R.repair([dict(x) for x in m])
    b, db = FT.repair_intervals([dict(x) for x in m])
    assert da == db == [1, 3]
    assert [(x["id"], x["begin"], x["end"]) for x in a] == [(x["id"], x["begin"], x["end"]) for x in b] == \
        [(0, 0.0, 0.2), (2, 0.2, 0.25), (4, 0.25, 0.4)]


@pytest.mark.parametrize("snip_edges", [0, 1])
def test_hand_made_intervals(fx, snip_edges):
    hb = R.hand_batch(fx)
    windows, out = R.hand_reference(fx, snip_edges)
    assert _same_windows(windows, FT.plan_windows(hb.intervals, [len(x) / R.SR for x in hb.pcm]))
    by = {(w.utt, w.index): (w, o) for w, o in zip(windows, out)}
    # utterances of one interval and of none have no windows
    assert not any(w.utt in (1, 2) for w in windows)
    # a boundary within 45 ms of time 0: the cut starts at 0 and the rows 15 ms before the boundary
    w, o = by[(0, 1)]
    assert (w.feature_begin, w.begin_offset, w.end_offset) == (0.0, 0.015, 0.045) and not o.failed and o.rows == 30
    # … and within 45 ms of the end: the cut ends with the utterance
    w, o = by[(0, 4)]
    assert w.feature_end == len(hb.pcm[0]) / R.SR == 0.6 and w.feature_begin == 0.53
    if snip_edges:                           # 70 ms cut: 46 frames; the window asks for rows 30 … 60
        assert o.truncated and o.rows == 16 and not o.failed
    else:
        assert not o.truncated and o.rows == 30 and not o.failed
    # fewer than 6 rows: a path through two three-state phones does not fit; both scales fail, the boundary stays
    w, o = by[(3, 1)]
    assert o.rows == 5 and o.failed and o.scale is None and (o.boundary, o.label) == (0.002, int(hb.intervals[3][1].symbol))
    assert not by[(3, 2)][1].failed
    # zero rows
    w, o = by[(4, 1)]
    assert o.rows == 0 and o.failed and (w.begin_offset, w.end_offset) == (0.0, 0.0)
    assert not by[(4, 2)][1].failed
    w, o = by[(5, 2)]                        # 5 ms before the end: rows 30 … 50; snip_edges=1: the 50 ms cut has 26 frames
    assert (o.rows == 0 and o.truncated and o.failed) if snip_edges else (o.rows == 20 and not o.truncated and not o.failed)
    got_iv, got_del = FT.assemble(windows, hb.intervals, _alis(out), fx.mono_tm, fx.mono_lex.phone_table)
    ivs, dels = R.assemble(windows, hb.intervals, _alis(out), fx.mono_tm, fx.mono_lex.phone_table)
    assert R.as_tuples(got_iv) == ivs and got_del == dels
    assert ivs[2] == [] and dels[2] == [] and len(ivs[1]) == 1 and 0 in dels[4]


@pytest.mark.parametrize("snip_edges", [0, 1])
def test_lda_inputs_align_at_the_first_beam(fx, snip_edges):
    s = R.lda_setup(fx)
    windows, out = R.lda_reference(fx, snip_edges)
    assert len(windows) == sum(len(ivs) - 1 for ivs in s.batch.intervals) == 21
    assert all(o.scale == 1.0 and o.status == 0 for o in out)
    states = set()
    for w in windows:
        f = FT.two_phone_graph(s.compiler, s.group(w.prev_phone), s.group(w.phone))
        states.add(f.num_states)
        assert not (f.arcs["ilabel"] == 0).any() and len(s.group(w.phone)) == 2
    print(f"snip_edges={snip_edges}: two-phone graphs of 2 x 2 triphones have {sorted(states)} states")
    assert 14 <= min(states) and max(states) <= 32       # 2 x 2 paths of six HMM states, shared where the tree ties them
    n_gauss = np.diff(s.am.pdf_offsets)
    assert s.am.dim == 40 and s.lda.shape == (40, 91) and (n_gauss > 16).any() and (n_gauss == 1).any()
    diff = np.abs(np.diff(R.speaker_offsets(s.batch.spk_stats), axis=0))[0]
    assert diff.min() > 1000 * R.FEATURE_BAR
    assert np.abs(s.fmllr[0] - s.fmllr[1]).max() > 1000 * R.FEATURE_BAR
