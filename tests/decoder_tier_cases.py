"""The wavefront decoder's large-graph tiers as seeded cases, shared by tests/test_decoder_tiers_cpu.py (the oracle alone:
the cases are what they claim to be) and tests/test_gpu_decoder_tiers.py (the device against the oracle).

align_impl changes tier with the size of the batch's largest graph (csrc/viterbi_plan.hpp; thresholds measured by
tests/native/viterbi_plan_check.cpp for graphs of 3.8 arcs a state and one token per state):

    token lists in HBM      from 1 836 states (1 365 with epsilon arcs)
    capacity shrink         from 2 881 states (1 921 with epsilon arcs)
    hashed table, N = 512   from 2 048 states

Every constructor takes (tm, eps) — eps: the epsilon twin, ``helpers.with_eps`` applied to every graph — and returns
``(fsts, frames, beams, caps)``: graphs, one feature matrix per graph, the (beam, retry beam) points to decode at, and the
capacities as keyword arguments of ``engine.align`` / ``engine.align_features``.  An epsilon twin that is to stay in a
tier between two thresholds starts from a smaller graph (``BIG``): the epsilon states of a 2 600-state graph's twin would
carry it past the shrink threshold, which is another case's business.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd.packing import GraphPacking
from oracle import oracle as O
from tests import helpers, synth
from tests.test_gpu_parity import _random_graph

BIG = {False: 2600, True: 1500}       # the large graph of the HBM-list cases, before with_eps
EPS_FRAC = 0.05                       # share of arcs with_eps splits in the twins that must stay below a threshold
SMALL = (3, 40, 400, 1100)
PLAN_FIELDS = ("pass", "code", "N", "C", "lds_bytes", "lists_in_lds", "hbits")


def ceil64(n: int) -> int:
    return (int(n) + 63) & ~63


def plan(max_states, max_arcs, eps, lazy, retry_beam=40.0, max_tokens=1024, bp_tokens_per_frame=512, beam=10.0, **_):
    """mfa_debug_viterbi_plan as a list of dicts, one per launch (host query: no GPU needed)."""
    o = _lib.AlignOpts(float(beam), float(retry_beam), 0.1, int(max_tokens), int(bp_tokens_per_frame))
    rows = np.zeros((3, 7), dtype=np.int32)
    n = _lib.lib().mfa_debug_viterbi_plan(C.byref(o), int(max_states), int(max_arcs), int(bool(eps)), int(bool(lazy)),
                                          rows.ctypes.data, 3)
    assert 1 <= n <= 3, f"mfa_debug_viterbi_plan returned {n}"
    return [dict(zip(PLAN_FIELDS, (int(v) for v in rows[i]))) for i in range(n)]


def batch_plan(fsts, lazy, retry_beam, caps):
    """The plan of a batch of graphs as pack_graphs sizes it: its largest state and arc counts."""
    return plan(max(f.num_states for f in fsts), max(f.num_arcs for f in fsts), has_eps(fsts), lazy, retry_beam=retry_beam, **caps)


def has_eps(fsts) -> bool:
    return any(bool((f.arcs["ilabel"] == 0).any()) for f in fsts)


def hard_bounds(fsts) -> dict:
    """PackedGraphs.hard_bounds() of the batch these graphs make, as capacities."""
    s = max(1, max(f.num_states for f in fsts))
    return dict(max_tokens=s, bp_tokens_per_frame=s + (s // 2 + 2 if has_eps(fsts) else 0))


def _graph(seed, tm, n_states, eps, frac=0.3):
    """_random_graph from its own seed, or its epsilon twin — drawn again when the twin is one the wavefront decoder does
    not take."""
    rng = np.random.default_rng(seed)
    while True:
        f = _random_graph(rng, tm, n_states)
        if not eps:
            return f
        fe = helpers.with_eps(rng, f, frac)
        if n_states > 3 and not (fe.arcs["ilabel"] == 0).any():
            continue
        if GraphPacking.needs_general_decoder(fe) or helpers.has_negative_eps_cycle(fe):
            continue
        return fe


def _feats(seed, T, dim):
    return np.random.default_rng(seed).normal(0.0, 3.0, size=(T, dim)).astype(np.float32)


def oracle(tm, am, f, x, beam, retry, want_stats=False):
    """The oracle's alignment of features ``x`` on graph ``f``: scores of the graph's own pdfs, then FasterDecoder."""
    emit = f.arcs["ilabel"] > 0
    pl = np.unique(tm.id2pdf[f.arcs["ilabel"][emit]])
    ll = O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl)
    return helpers.oracle_align(tm, f, ll, pl, beam=beam, retry_beam=retry, want_stats=want_stats)


# Seeds.  _random_graph often leaves most of a graph unreachable from its start state; the seeds below were picked with the
# oracle so that each large graph is well connected and the beams give the statuses and token counts the case is about
# (tests/test_decoder_tiers_cpu.py holds them to that).  A graph's features come from its seed + 500.
# ---- token lists in HBM -------------------------------------------------------------------------------------------------
HBM_SEED = {False: 7022, True: 7000}
HBM_SMALL_SEED = 7100
HBM_FRAMES = (48, 5, 30, 60, 44)
HBM_BEAMS = ((60.0, 0.0), (0.5, 30.0), (2.0, 40.0))


def _hbm_graphs(tm, eps):
    fsts = [_graph(HBM_SEED[eps], tm, BIG[eps], eps, EPS_FRAC)]
    fsts += [_graph(HBM_SMALL_SEED + i, tm, s, eps, 0.3 if s <= 400 else EPS_FRAC) for i, s in enumerate(SMALL)]
    seeds = [HBM_SEED[eps] + 500] + [HBM_SMALL_SEED + 500 + i for i in range(len(SMALL))]
    return fsts, [_feats(sd, T, 39) for sd, T in zip(seeds, HBM_FRAMES)]


def hbm(tm, eps=False):
    """One large graph and four small ones, one token per state: the growth launch and the retry launch keep their token
    lists in HBM (viterbi_kernel<false, *>).  A wide beam without retry (the large graph holds hundreds of tokens: the
    growth launch decodes it), two narrow beams with a retry beam (the large graph needs it: status 1)."""
    fsts, frames = _hbm_graphs(tm, eps)
    return fsts, frames, HBM_BEAMS, hard_bounds(fsts)


HBM_DEFAULT_BEAMS = ((0.5, 30.0), (2.0, 40.0))


def hbm_default(tm, eps=False):
    """The same graphs with the default capacities: only the retry launch (N = min(4096, max_states)) has its lists in
    HBM, and the large graph needs it (oracle status 1)."""
    fsts, frames = _hbm_graphs(tm, eps)
    return fsts, frames, HBM_DEFAULT_BEAMS, dict(max_tokens=1024, bp_tokens_per_frame=512)


# ---- hashed state→slot table above the first tier ------------------------------------------------------------------------
HASHED_SEED = {False: 7012, True: 7005}
HASHED_BEAMS = ((60.0, 0.0), (1.0e4, 0.0))    # peak live tokens in (128, 512] / above 512
HASHED_SCAN_BEAM = 60.0
HASHED_T = 40


def hashed512(tm, eps=False):
    """A 2 600-state graph with 512 tokens: the growth launch runs with a hashed table of 2 048 buckets (hbits = 11) and
    linear probing under hundreds of live tokens."""
    fsts = [_graph(HASHED_SEED[eps], tm, 2600, eps)]
    frames = [_feats(HASHED_SEED[eps] + 500, HASHED_T, 39)]
    return fsts, frames, HASHED_BEAMS, dict(max_tokens=512, bp_tokens_per_frame=hard_bounds(fsts)["bp_tokens_per_frame"])


# ---- capacity shrink -----------------------------------------------------------------------------------------------------
SHRINK_SEED = {False: 7000, True: 7000}
SHRINK_BEAMS = ((1.0e4, 0.0),)


def shrink(tm, eps=False):
    """A 3 600-state graph decoded with ``hard_bounds()``: even the list-free tables exceed 160 KiB, the plan halves the
    token capacity, and a beam that keeps the graph alive overflows it."""
    fsts = [_graph(SHRINK_SEED[eps], tm, 3600, eps)]
    frames = [_feats(SHRINK_SEED[eps] + 500, 40, 39)]
    return fsts, frames, SHRINK_BEAMS, hard_bounds(fsts)


# ---- HBM lists across a window boundary ----------------------------------------------------------------------------------
RESUME_SEED = {False: 7003, True: 7004}
RESUME_BEAMS = ((30.0, 0.0), (60.0, 0.0))
RESUME_T = 300


def resume(tm, eps=False):
    """300 frames on a large graph with one token per state: the lazy path's list passes decode in windows of 256 frames,
    so the growth launch's second window picks the lists up where the first left them in HBM."""
    fsts = [_graph(RESUME_SEED[eps], tm, BIG[eps], eps, EPS_FRAC)]
    frames = [_feats(RESUME_SEED[eps] + 500, RESUME_T, 39)]
    return fsts, frames, RESUME_BEAMS, hard_bounds(fsts)


# ---- wide score rows -----------------------------------------------------------------------------------------------------
WIDE_SEED = {False: 7011, True: 7003}
WIDE_MID_SEED = 7004
WIDE_BEAMS = ((8.0, 0.0), (0.5, 30.0))
WIDE_PDFS = 900          # pdfs the second graph's arcs are drawn from
WIDE_T = 50
_TRIPHONE = None


def triphone_model():
    """The synthetic triphone model with single Gaussians (about 5 000 pdfs in 40 dimensions), trained on noise: only its
    size matters here."""
    global _TRIPHONE
    if _TRIPHONE is None:
        rng = np.random.default_rng(0)
        world = synth.SynthWorld.build()
        _TRIPHONE = synth.train_triphone(world, lambda pcm, spk: rng.normal(size=(len(pcm) // 160, 40)).astype(np.float32),
                                         n_train=12, n_gauss=1)
    return _TRIPHONE


def wide_rows(tm=None, eps=False):
    """Two large graphs over the triphone model's transition-ids, each a batch of its own in the tests: random ids spread
    over thousands of pdfs (more than 2 048 score columns: no speculation, rows read from HBM), and the same kind of graph
    with its ids drawn from ``WIDE_PDFS`` pdfs (513 … 2 048 columns: rows read from HBM with speculation still on).
    ``tm`` is ignored: the model is ``triphone_model()``.  Capacities: ``hard_bounds`` of each graph's own batch."""
    tm = triphone_model().tm
    wide = _graph(WIDE_SEED[eps], tm, BIG[eps], eps, EPS_FRAC)
    rng = np.random.default_rng(WIDE_MID_SEED + 1000)
    pdfs = rng.choice(tm.num_pdfs, size=WIDE_PDFS, replace=False)
    tids = np.flatnonzero(np.isin(tm.id2pdf, pdfs) & (np.arange(tm.id2pdf.shape[0]) > 0))
    g = _graph(WIDE_MID_SEED, tm, BIG[eps], eps, EPS_FRAC)
    arcs = g.arcs.copy()
    emit = arcs["ilabel"] > 0
    arcs["ilabel"][emit] = tids[rng.integers(0, len(tids), size=int(emit.sum()))]
    mid = K.Fst(g.start, g.arc_offsets, arcs, g.final)
    frames = [_feats(WIDE_SEED[eps] + 500, WIDE_T, 40), _feats(WIDE_MID_SEED + 500, WIDE_T, 40)]
    return [wide, mid], frames, WIDE_BEAMS, None


def column_count(f, tm, groups=8, span=32) -> int:
    """Score columns pack_graphs gives graph ``f`` (one per pdf and depth cluster; mfa_build_score_plan_grouped, a host
    call), for a model of single Gaussians (every pdf in slot class 5, as the models of these cases are)."""
    lib = _lib.lib()
    na = f.num_arcs
    off = np.ascontiguousarray(f.arc_offsets, dtype=np.int32)
    nxt = np.ascontiguousarray(f.arcs["nextstate"], dtype=np.int32)
    il = f.arcs["ilabel"]
    pdf = np.ascontiguousarray(np.where(il > 0, tm.id2pdf[np.maximum(il, 0)], -1), dtype=np.int32)
    cls = np.full(tm.num_pdfs, 5, dtype=np.int32)
    sd = np.empty((f.num_states, 2), np.int32)
    col, cp, cf, cl = (np.empty(max(na, 1), np.int32) for _ in range(4))
    cc, gc, n = np.zeros(6, np.int32), np.zeros(groups, np.int32), C.c_int32(0)
    rc = lib.mfa_build_score_plan_grouped(f.num_states, off.ctypes.data, nxt.ctypes.data, pdf.ctypes.data, int(f.start),
                                          len(cls), cls.ctypes.data, span, groups, sd.ctypes.data, col.ctypes.data,
                                          cp.ctypes.data, cf.ctypes.data, cl.ctypes.data, cc.ctypes.data, gc.ctypes.data,
                                          C.byref(n))
    assert rc == 0, rc
    return int(n.value)


CASES = dict(hbm=hbm, hbm_default=hbm_default, hashed512=hashed512, shrink=shrink, resume=resume, wide_rows=wide_rows)

_CASE_CACHE: dict = {}
_REF_CACHE: dict = {}


def case(name, eps, fx):
    """The case as dict(tm, am, fsts, frames, beams, caps), built once per process (``fx``: helpers.Fixtures)."""
    key = (name, bool(eps))
    if key not in _CASE_CACHE:
        if name == "wide_rows":
            m = triphone_model()
            tm, am = m.tm, m.am
        else:
            tm, am = fx.mono_tm, fx.mono_am
        fsts, frames, beams, caps = CASES[name](tm, bool(eps))
        _CASE_CACHE[key] = dict(tm=tm, am=am, fsts=fsts, frames=frames, beams=beams, caps=caps)
    return _CASE_CACHE[key]


def refs(name, eps, fx, beam, retry):
    """The oracle's results for every utterance of the case at one (beam, retry beam), with its token counts; computed once
    per process and shared by the tests: treat as read-only."""
    key = (name, bool(eps), float(beam), float(retry))
    if key not in _REF_CACHE:
        c = case(name, eps, fx)
        _REF_CACHE[key] = [oracle(c["tm"], c["am"], f, x, beam, retry, want_stats=True) for f, x in zip(c["fsts"], c["frames"])]
    return _REF_CACHE[key]

