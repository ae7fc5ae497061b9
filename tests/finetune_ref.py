"""Boundary fine-tuning one boundary at a time, on the oracle alone: a sequential restatement of FineTuneFunction._run
(MFA/alignment/multiprocessing.py:1254-1349) that reports what happened to every window, the inputs the fine-tuning tests
share (tests/test_finetune_cpu.py proves on this reference that they reach every branch, tests/test_gpu_finetune_stages.py
runs them on the device), and ``assemble``: intervals and deletions from given per-window alignments.

Where the reference would stop with an error this follows the library, and says so in the outcome: a window whose row
range leaves the cut's frames is cut to them (``truncated``; the reference's FloatSubMatrix asserts), a window that aligns
at neither acoustic scale, or has no rows, keeps its boundary and phone (``failed``; the reference dereferences None)."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from montreal_forced_aligner_amd import ctm as C
from montreal_forced_aligner_amd import finetune as FT
from montreal_forced_aligner_amd import graph as G
from oracle import oracle as O
from tests import helpers

SR = 16000
CUTS = ((0.0, 4.2, "this is the acoustic corpus i'm talking pretty fast here"),
        (4.0, 6.5, "there's nothing going else going on"),
        (23.5, 26.72, "um and that should be all thanks"))
UTT2SPK = (1, 0, 1)              # scrambled: utterances 0 and 2 belong to speaker 1, utterance 1 to speaker 0
FEATURE_BAR = 1e-4               # tests/test_gpu_frontend_options.py: the feature kernels against the oracle chain


@dataclass
class Window:
    utt: int
    index: int
    feature_begin: float
    feature_end: float
    begin_offset: float
    end_offset: float
    prev_phone: int
    phone: int


@dataclass
class Outcome:
    boundary: float              # the interval's begin after tuning (its own when the window failed)
    label: int                   # phone id after tuning
    scale: Optional[float]       # acoustic scale the alignment was found at; None: failed
    failed: bool
    truncated: bool              # fewer rows than the window asked for
    rows: int
    ali: Optional[np.ndarray]
    status: Optional[int] = None  # the oracle decoder's, at ``scale``: 0 first beam, 1 retry beam


def plan(intervals, utt_ends, frame_shift=0.01) -> List[Window]:
    """:1261-1275: ±1.5 frames decoded, ±4.5 frames of audio under the features, both clipped to the utterance and, on
    the right, the decoded range to the interval's own end."""
    out = []
    pad = round(frame_shift * 1.5, 3)
    for u, ivs in enumerate(intervals):
        for i, iv in enumerate(ivs):
            if i == 0:
                continue
            seg_b = max(round(iv.begin - pad, 4), 0)
            feat_b = max(round(iv.begin - 3 * pad, 4), 0)
            seg_e = round(min(iv.begin + pad, iv.end), 3)
            feat_e = min(round(iv.begin + 3 * pad, 4), utt_ends[u])
            out.append(Window(u, i, feat_b, feat_e, round(seg_b - feat_b, 4), round(seg_e - feat_b, 4),
                              int(ivs[i - 1].symbol), int(iv.symbol)))
    return out


def cut_samples(w, sample_rate=SR):
    return int(round(w.feature_begin * sample_rate)), int(round(w.feature_end * sample_rate))


def row_range(w, n_frames):
    """(first row, end row, truncated) of the window inside its cut's ``n_frames`` 1 ms frames (:1300-1304)."""
    a, b = int(round(w.begin_offset * 1000)), int(round(w.end_offset * 1000))
    r0 = min(max(a, 0), n_frames)
    r1 = min(max(b, r0), n_frames)
    return r0, r1, (r1 - r0) < (b - a)


def feature_chain(mfcc, stats, lda=None, fmllr=None, splice_context=3):
    """CMVN → Δ+ΔΔ, or splice + LDA, → fMLLR (:1287-1299), on the oracle."""
    x = O.cmvn_apply(stats, mfcc) if stats is not None else np.asarray(mfcc, np.float32)
    x = O.deltas(x) if lda is None else O.affine(O.splice(x, splice_context, splice_context), lda)
    return x if fmllr is None else O.affine(x, fmllr)


def repair(mapping: List[dict]):
    """:1327-1349.  Every end becomes the next begin; intervals left without length go; again until nothing goes."""
    gone: List[object] = []
    while True:
        for a, b in zip(mapping[:-1], mapping[1:]):
            a["end"] = b["begin"]
        dead = [m["id"] for m in mapping if not m["begin"] < m["end"]]
        gone += dead
        if not dead:
            return mapping, gone
        mapping = [m for m in mapping if m["id"] not in dead]


def assemble(windows, intervals, alis: Dict[int, np.ndarray], tm, phone_table=None):
    """(interval lists as (begin, end, label, phone id) tuples, deletions per utterance) from per-window alignments
    (:1310-1349).  ``alis``: window index → transition-ids; a window without one keeps its boundary and phone.  Labels: the
    phone table's when given; else the label an interval of the same utterance gives that phone id, else the id itself."""
    maps = [[dict(id=0, begin=ivs[0].begin, end=ivs[0].end, phone=int(ivs[0].symbol))] if len(ivs) else [] for ivs in intervals]
    for k, w in enumerate(windows):
        iv = intervals[w.utt][w.index]
        begin, phone = iv.begin, int(iv.symbol)
        if k in alis:
            segs = C.generate_ctm(alis[k], tm, None, FT.NEW_FRAME_SHIFT)
            if len(segs) > 1:
                begin, phone = round(segs[1].begin + w.feature_begin + w.begin_offset, 4), int(segs[1].symbol)
        maps[w.utt].append(dict(id=w.index, begin=begin, end=iv.end, phone=phone))
    out, dels = [], []
    for u, m in enumerate(maps):
        m, gone = repair(m) if m else ([], [])
        seen = {int(iv.symbol): iv.label for iv in intervals[u]}
        name = (lambda p: phone_table.find(p)) if phone_table is not None else (lambda p: seen.get(p, p))
        out.append([(x["begin"], x["end"], name(x["phone"]), x["phone"]) for x in m])
        dels.append(gone)
    return out, dels


def as_tuples(interval_lists):
    return [[(iv.begin, iv.end, iv.label, iv.symbol) for iv in ivs] for ivs in interval_lists]


def fine_tune(pcm, intervals, tm, am, compiler, scaled, stats=None, lda=None, fmllr=None,
              group: Callable[[int], Sequence[int]] = lambda p: [p], beam=100.0, retry_beam=400.0, snip_edges=0,
              splice_context=3, sample_rate=SR):
    """One boundary at a time.  ``stats`` / ``fmllr``: per utterance (its speaker's) or None.  Returns (windows, outcomes)."""
    windows = plan(intervals, [len(x) / sample_rate for x in pcm])
    opts = O.default_mfcc_opts(frame_shift_ms=1.0, snip_edges=snip_edges)
    graphs: dict = {}
    out: List[Outcome] = []
    for w in windows:
        iv = intervals[w.utt][w.index]
        keep = dict(boundary=iv.begin, label=int(iv.symbol), scale=None, failed=True, ali=None)
        a, b = cut_samples(w, sample_rate)
        n_frames = max(O.mfcc_num_frames(b - a, opts), 0)
        r0, r1, truncated = row_range(w, n_frames)
        if r1 == r0:
            out.append(Outcome(truncated=truncated, rows=0, **keep))
            continue
        x = feature_chain(O.mfcc(pcm[w.utt][a:b].astype(np.float32), opts), None if stats is None else stats[w.utt], lda,
                          None if fmllr is None else fmllr[w.utt], splice_context)[r0:r1]
        key = (tuple(group(w.prev_phone)), tuple(group(w.phone)))
        if key not in graphs:
            graphs[key] = G.add_transition_probs(FT.two_phone_graph(compiler, *key), scaled)
        for scale in (1.0, 0.1):
            r = helpers.oracle_align_feats(tm, graphs[key], x, am, scale, beam, retry_beam)
            if r["status"] in (0, 1):
                break
        else:
            out.append(Outcome(truncated=truncated, rows=r1 - r0, **keep))
            continue
        segs = C.generate_ctm(r["ali"], tm, None, FT.NEW_FRAME_SHIFT)
        assert len(segs) == 2, "a path through a two-phone graph has two phones"
        out.append(Outcome(round(segs[1].begin + w.feature_begin + w.begin_offset, 4), int(segs[1].symbol), scale, False,
                           truncated, r1 - r0, r["ali"], int(r["status"])))
    return windows, out


# ---- the shared inputs ----------------------------------------------------------------------------------------------------

@dataclass
class Batch:
    pcm: List[np.ndarray]
    intervals: List[List[C.CtmInterval]]     # first pass at 10 ms, oracle (beam 100 / 400, acoustic scale 0.1)
    utt2spk: tuple
    spk_stats: np.ndarray                    # [2, 2, 14] float64: the speakers' 10 ms CMVN statistics

    @property
    def utt_stats(self):
        return [self.spk_stats[s] for s in self.utt2spk]


@lru_cache(maxsize=None)
def mono_batch(fx) -> Batch:
    """The three fixture cuts, first pass by the oracle on per-utterance CMVN, two speakers in scrambled order."""
    tm, am = fx.mono_tm, fx.mono_am
    pcm = [np.ascontiguousarray(fx.pcm[int(a * SR): int(b * SR)]) for a, b, _ in CUTS]
    mf = [O.mfcc(x.astype(np.float32), O.default_mfcc_opts()) for x in pcm]
    ivs = []
    for x, (_a, _b, text) in zip(pcm, CUTS):
        r = helpers.oracle_align_feats(tm, fx.mono_graph(text), fx.mono_feats(x), am, 0.1, 100.0, 400.0)
        assert r["status"] in (0, 1)
        ivs.append(C.generate_ctm(r["ali"], tm, fx.mono_lex.phone_table, 0.01))
    stats = np.stack([O.cmvn_stats([m for m, s in zip(mf, UTT2SPK) if s == k]) for k in (0, 1)])
    return Batch(pcm, ivs, UTT2SPK, stats)


def speaker_offsets(stats):
    """The CMVN offset (mean) of every speaker, [n_spk, dim]."""
    return stats[:, 0, :-1] / stats[:, 0, -1:]


def mono_phone_classes(fx):
    """(silence phone ids, non-silence phone ids) of the mono model's phone table."""
    sil, other = [], []
    for k, name in fx.mono_lex.phone_table:
        if k == 0 or name.startswith("#"):
            continue
        (sil if name.split("_")[0] in ("sil", "sp", "spn") else other).append(k)
    return sil, other


def seeded_groups(fx, size=40):
    """phone id → its group: the phone and ``size − 1`` seeded other non-silence phones; a silence phone stays alone."""
    sil, other = mono_phone_classes(fx)

    @lru_cache(maxsize=None)
    def group(p):
        if p in sil:
            return (p,)
        rng = np.random.default_rng(p * 1000 + size)
        return tuple(sorted(set(rng.choice(other, size=min(size, len(other)) - 1, replace=False).tolist()) | {p}))
    return group


def squeeze(ivs, seed, share=0.3):
    """The intervals with about ``share`` of them squeezed to 10 ms (their begin moved to 10 ms after the previous one's),
    kept increasing; the last end stays."""
    rng = np.random.default_rng(seed)
    b = [iv.begin for iv in ivs] + [ivs[-1].end]
    nb = list(b)
    for i in range(2, len(b) - 1):
        if rng.random() < share:
            nb[i] = round(nb[i - 1] + 0.01, 2)
    nb = [round(x, 2) for x in nb]
    for i in range(1, len(nb)):
        if nb[i] <= nb[i - 1]:
            nb[i] = round(nb[i - 1] + 0.01, 2)
    nb[-1] = max(nb[-1], b[-1])
    return [C.CtmInterval(nb[i], nb[i + 1], iv.label, iv.symbol) for i, iv in enumerate(ivs)]


SQUEEZE_SEEDS = (0, 0, 0)        # one per utterance; tests/test_finetune_cpu.py checks what they reach
CONFIGS = ("groups40", "identity", "squeezed")


def mono_config(fx, name):
    """dict(intervals, group, beam, retry_beam) of a configuration of the mono batch."""
    batch = mono_batch(fx)
    if name == "groups40":
        return dict(intervals=batch.intervals, group=seeded_groups(fx, 40), beam=1.0, retry_beam=4.0)
    if name == "identity":
        return dict(intervals=batch.intervals, group=lambda p: (p,), beam=100.0, retry_beam=400.0)
    if name == "squeezed":
        return dict(intervals=[squeeze(ivs, s) for ivs, s in zip(batch.intervals, SQUEEZE_SEEDS)], group=lambda p: (p,),
                    beam=100.0, retry_beam=400.0)
    raise ValueError(name)


@lru_cache(maxsize=None)
def mono_reference(fx, name, snip_edges):
    """(windows, outcomes) of the sequential reference on a configuration: computed once, shared, left unchanged."""
    cfg, batch = mono_config(fx, name), mono_batch(fx)
    return fine_tune(batch.pcm, cfg["intervals"], fx.mono_tm, fx.mono_am, fx.mono_gc, fx.mono_tm.scaled_log_probs(1.0, 0.1),
                     stats=batch.utt_stats, group=cfg["group"], beam=cfg["beam"], retry_beam=cfg["retry_beam"],
                     snip_edges=snip_edges)


def hand_intervals(spec, labels=None):
    """[(begin, end, phone id)] → CtmIntervals (label: ``labels[id]`` or "p<id>")."""
    return [C.CtmInterval(b, e, labels[p] if labels else f"p{p}", p) for b, e, p in spec]


HAND_UTT2SPK = (1, 0, 1, 0, 1, 0)


@lru_cache(maxsize=None)
def hand_batch(fx) -> Batch:
    """Hand-made intervals over the start of the recording (phones: the first pass's own, in order).
    0: a boundary within 45 ms of time 0 and two within 45 ms of the end; 1: one interval; 2: none;
    3: a window of 5 rows (two three-state phones need 6); 4: a window of no rows (an empty interval at time 0);
    5: a boundary 5 ms before the end — with snip_edges=1 the cut's 26 frames end before the window's first row, 30."""
    batch = mono_batch(fx)
    first = batch.intervals[0]
    p = [int(iv.symbol) for iv in first]
    labels = {int(iv.symbol): iv.label for iv in first}
    assert all(a != b for a, b in zip(p[:5], p[1:6]))
    spec = [([(0.0, 0.03, p[0]), (0.03, 0.10, p[1]), (0.10, 0.56, p[2]), (0.56, 0.575, p[3]), (0.575, 0.6, p[4])], 0.6),
            ([(0.0, 0.3, p[1])], 0.3),
            ([], 0.2),
            ([(0.0, 0.002, p[0]), (0.002, 0.005, p[1]), (0.005, 0.4, p[2])], 0.4),
            ([(0.0, 0.0, p[0]), (0.0, 0.0, p[1]), (0.0, 0.3, p[2])], 0.3),
            ([(0.0, 0.2, p[1]), (0.2, 0.495, p[2]), (0.495, 0.5, p[3])], 0.5)]
    pcm = [np.ascontiguousarray(fx.pcm[: int(round(end * SR))]) for _ivs, end in spec]
    return Batch(pcm, [hand_intervals(ivs, labels) for ivs, _end in spec], HAND_UTT2SPK, batch.spk_stats)


@lru_cache(maxsize=None)
def hand_reference(fx, snip_edges):
    hb = hand_batch(fx)
    return fine_tune(hb.pcm, hb.intervals, fx.mono_tm, fx.mono_am, fx.mono_gc, fx.mono_tm.scaled_log_probs(1.0, 0.1),
                     stats=hb.utt_stats, snip_edges=snip_edges)


# ---- the LDA + fMLLR model (acoustic_g2p_output_model: 71 phones, triphone tree, mixtures of 1 … 26 Gaussians) ------------

@dataclass
class LdaSetup:
    tm: object
    am: object
    lex: object
    compiler: object
    scaled: np.ndarray
    lda: np.ndarray
    fmllr: np.ndarray                        # [2, 40, 41]: a seeded transform per speaker
    batch: Batch
    group: Callable[[int], Sequence[int]]


@lru_cache(maxsize=None)
def lda_setup(fx) -> LdaSetup:
    """Hand-made intervals of 60 … 140 ms over the model's 71 phones (seeded), on the three cuts; groups of two phones."""
    tm, am = fx.g2p_tm, fx.g2p_am
    lex = G.LexiconCompiler(position_dependent_phones=False, phones=fx.g2p_meta["phones"], silence_phone="sil", oov_phone="spn")
    lex.build_phone_table(["sil", "spn"])
    compiler = G.TrainingGraphCompiler(tm, fx.g2p_tree, lex)
    phones = [k for k, name in lex.phone_table if k > 0 and not name.startswith("#") and name not in ("sil", "spn")]
    assert len(phones) == 71
    rng = np.random.default_rng(71)
    pcm = mono_batch(fx).pcm
    ivs = []
    for n, x in zip((9, 7, 8), pcm):
        t, spec = 0.2, []
        for _ in range(n):
            d = round(float(rng.integers(6, 15)) * 0.01, 2)
            spec.append((round(t, 2), round(t + d, 2), int(rng.choice(phones))))
            t += d
        assert t < len(x) / SR
        ivs.append(hand_intervals(spec, {p: lex.phone_table.find(p) for p in phones}))
    mf = [O.mfcc(x.astype(np.float32), O.default_mfcc_opts()) for x in pcm]
    stats = np.stack([O.cmvn_stats([m for m, s in zip(mf, UTT2SPK) if s == k]) for k in (0, 1)])
    D = am.dim
    fm = np.stack([np.eye(D, D + 1, dtype=np.float32) + 0.1 * helpers.random_affine(rng, D, D + 1) for _ in range(2)])

    def group(p):       # the phone and its neighbour in the table (wrapping round): two phones
        return tuple(sorted({p, phones[(phones.index(p) + 1) % len(phones)]}))
    return LdaSetup(tm, am, lex, compiler, tm.scaled_log_probs(1.0, 0.1), fx.g2p_lda, fm, Batch(pcm, ivs, UTT2SPK, stats), group)


@lru_cache(maxsize=None)
def lda_reference(fx, snip_edges):
    s = lda_setup(fx)
    return fine_tune(s.batch.pcm, s.batch.intervals, s.tm, s.am, s.compiler, s.scaled, stats=s.batch.utt_stats, lda=s.lda,
                     fmllr=[s.fmllr[k] for k in s.batch.utt2spk], group=s.group, beam=100.0, retry_beam=400.0,
                     snip_edges=snip_edges)
