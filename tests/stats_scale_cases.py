"""The training statistics at real key counts and long segments: the cases tests/test_stats_scale_cpu.py (host twins) and
tests/test_gpu_stats_scale.py (device) share.  Builders only, all on the exact tiers of tests/mllt_ref.py, tests/lda_ref.py
and tests/tree_ref.py (integers, or a dyadic grid: any order of summation gives the same bits), so every comparison made on
them is a bit-equality.

Every size is a multiple of one of the library's own constants, which the caller passes in: Cg = mfa_gmm_acc_chunk_frames()
(also the chunk of the MLLT statistics' occupancies and totals), Cm = mfa_mllt_acc_chunk_frames(), the LDA statistics' chunk
and slab, the tree statistics' chunk.  ``units`` restates how the kernels cut a key's frames: ceil(count / chunk) per key.
The tests assert from the references' own counts that a case reaches the path it is there for (tests/test_stats_scale_cpu.py
lists them).

Frame orders.  ``shuffled``: a permutation, as everywhere else in the suite — every run of equal transition-ids has length 1.
``aligned``: the same frames laid out as an alignment is, in runs of one transition-id of 1, 2, 63, 64, 65 and 300 frames
(``alignment_shaped``), which is what the lookup's run compression (csrc/tid_lookup.hpp: one atomic per run inside a
wavefront) and the sort see in production.  The sums expected are those of the shuffled order."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import mle
from montreal_forced_aligner_amd import model as M
from montreal_forced_aligner_amd.model import TransitionModel
from tests import gmm_acc_ref as R
from tests import helpers, lda_ref
from tests import mllt_ref as MR
from tests import tree_ref as TR

KEY_COUNTS = (255, 256, 257, 511, 512, 513, 4960)
RUN_LENGTHS = (1, 2, 63, 64, 65, 300)
ORDERS = ("shuffled", "aligned")


def units(counts, chunk) -> np.ndarray:
    """ceil(count / chunk) per key: the units (chunks, sub-units) a kernel cuts a key's frames into."""
    return (np.asarray(counts, np.int64) + chunk - 1) // chunk


# ---- GMM and MLLT statistics: integer single-Gaussian pdfs ---------------------------------------------------------------------
def key_count_frames(P, Cg, Cm, last=None) -> np.ndarray:
    """Frames per pdf: 0 – 3 on most, 9·Cg + 1 on pdf 0, ``last`` (default 8·Cm: exactly eight units of the MLLT statistics, no
    remainder) on pdf P − 1, Cg on the one in the middle."""
    rng = np.random.default_rng(4100 + P)
    counts = rng.integers(0, 4, size=P)
    counts[0], counts[P // 2], counts[P - 1] = 9 * Cg + 1, Cg, 8 * Cm if last is None else last
    return counts


def sparse_frames(P, total=300) -> np.ndarray:
    """``total`` frames over P ≫ total pdfs: nearly every pdf empty, frames on the first and on the last."""
    rng = np.random.default_rng(4200 + P)
    counts = np.zeros(P, np.int64)
    counts[0], counts[P - 1] = 130, 100
    counts[rng.permutation(np.arange(1, P - 1))[: total - 230]] = 1
    return counts


def occupied_frames(P, occupied) -> np.ndarray:
    """Exactly ``occupied`` pdfs of P hold frames, 1 – 3 each: as many units (and sub-units) as occupied pdfs."""
    rng = np.random.default_rng(4300 + P + occupied)
    counts = np.zeros(P, np.int64)
    counts[rng.permutation(P)[:occupied]] = rng.integers(1, 4, size=occupied)
    return counts


def step_frames(Cg, Cm) -> np.ndarray:
    """The reductions add eight partials a step, then the rest one by one: pdfs of 7, 8 and 9 units of the GMM statistics
    (7·Cg, 8·Cg and 8·Cg + 1 frames) and one of 7 units of the MLLT statistics (7·Cm frames; tests/test_stats_scale_cpu.py's
    other cases hold 8, 9 and 10), with two small pdfs between them."""
    return np.array([7 * Cg, 2, 8 * Cg, 3, 8 * Cg + 1, 7 * Cm])


def _zero_weight_pdf(counts) -> int:
    """A pdf of one to three frames whose second transition-id gets weight 0 (its own frames carry the first)."""
    small = np.flatnonzero((np.asarray(counts) >= 1) & (np.asarray(counts) <= 3))
    return int(small[len(small) // 2])


@lru_cache(maxsize=None)
def _integer_shuffled(dim, counts):
    case = MR.integer_case(dim, list(counts), seed=len(counts))
    z = _zero_weight_pdf(counts)
    case.ali[(case.ali - 1) // 2 == z] = 2 * z + 1
    case.weights[2 * z + 2] = 0.0
    return case, z


def alignment_shaped(case: R.AccCase, z: int) -> R.AccCase:
    """The frames of a shuffled case in which every frame takes part, as runs of one transition-id.

    Each pdf's frames are cut into runs whose lengths cycle through RUN_LENGTHS, alternating between the pdf's two
    transition-ids; the runs are shuffled.  When a pdf holds 1 000 frames or more, its frames also make a fixed head and tail:
      frames 0 – 62     a run of 63
      frames 63 – 127   a run of 65 that starts at lane 63 of the first wavefront
      frames 128 – 427  a run of 300 across the 256-thread block's edge
      then              a run of 300 cut in the middle by one frame of id 0, and a run of 65 cut by one frame of the id of
                        weight 0 (2z + 2) — two frames that take no part, with NaN features
      at the end        a run of 64 that the batch ends in, in a wavefront that is not full (an id-0 frame is inserted before
                        it if the frame count would be a multiple of 64).
    The multiset of (pdf, feature row) is the shuffled case's, so its sums are."""
    rng = np.random.default_rng(4400 + len(case.ali))
    pdf = (case.ali.astype(np.int64) - 1) // 2
    P = case.am.num_pdfs
    counts = np.bincount(pdf, minlength=P)
    by_pdf = np.split(np.argsort(pdf, kind="stable"), np.cumsum(counts)[:-1])
    big = int(np.argmax(counts))
    laid = counts[big] >= 1000 and big != z
    NONE = -1                                                    # a row of NaN features

    def tids(p):
        return (2 * p + 1, 2 * p + 1) if p == z else (2 * p + 1, 2 * p + 2)

    runs, head, tail = [], [], []
    for p in range(P):
        rows, k, i = by_pdf[p], 0, p % len(RUN_LENGTHS) if counts[p] > 3 else 0
        if p == big and laid:
            t1, t2 = tids(p)
            take = lambda n: rows[k: k + n]
            head = [(t1, take(63))]; k += 63
            head += [(t2, take(65))]; k += 65
            head += [(t1, take(300))]; k += 300
            head += [(t2, take(150)), (0, np.array([NONE]))]; k += 150
            head += [(t2, take(150))]; k += 150
            head += [(t1, take(30)), (2 * z + 2, np.array([NONE]))]; k += 30
            head += [(t1, take(35))]; k += 35
            tail = [(t2, take(64))]; k += 64
        while k < len(rows):
            n = min(RUN_LENGTHS[i % len(RUN_LENGTHS)], len(rows) - k)
            runs.append((tids(p)[i % 2], rows[k: k + n]))
            k += n
            i += 1
    body = [runs[j] for j in rng.permutation(len(runs))]
    if laid and (sum(len(r) for _t, r in head + body + tail)) % 64 == 0:
        body.append((0, np.array([NONE])))
    seq = head + body + tail
    rows = np.concatenate([r for _t, r in seq])
    ali = np.concatenate([np.full(len(r), t, np.int32) for t, r in seq])
    feats = np.where((rows == NONE)[:, None], np.float32(np.nan), case.feats[np.maximum(rows, 0)])
    assert sorted(rows[rows >= 0].tolist()) == list(range(len(case.ali)))
    return R.AccCase(case.name + ", aligned", case.am, case.tm, np.ascontiguousarray(feats, np.float32), ali, case.weights)


def run_shape(case: R.AccCase) -> dict:
    """What the runs of equal transition-ids of ``case.ali`` look like: the properties the aligned order is there for."""
    ali = case.ali.astype(np.int64)
    T = len(ali)
    start = np.flatnonzero(np.concatenate([[True], ali[1:] != ali[:-1]]))
    length = np.diff(np.concatenate([start, [T]]))
    end = start + length - 1
    part = (ali > 0) & (case.weights[np.clip(ali, 0, len(case.weights) - 1)] != 0)
    inner = np.arange(1, T - 1)
    cut = inner[(ali[inner - 1] == ali[inner + 1]) & part[inner - 1] & ~part[inner]]
    return dict(frames=T, runs=len(start), lengths=set(length[part[start]].tolist()), longest=int(length.max()),
                starts_at_lane_63=bool(np.any((start % 64 == 63) & (length >= 2) & part[start])),
                crosses_a_block=bool(np.any((start // 256 != end // 256) & part[start])),
                cut_by_id_0=bool(np.any(ali[cut] == 0)), cut_by_weight_0=bool(np.any(ali[cut] > 0)),
                ends_inside_a_run=bool(length[-1] >= 2 and part[-1] and T % 64 != 0 and start[-1] % 64 != 0))


@lru_cache(maxsize=None)
def integer_case(dim, counts, order) -> R.AccCase:
    """Single-Gaussian integer pdfs (tests/mllt_ref.integer_case) with ``counts`` (a tuple) frames per pdf, in ``order``."""
    case, z = _integer_shuffled(dim, tuple(int(c) for c in counts))
    return case if order == "shuffled" else alignment_shaped(case, z)


def frame_counts(case: R.AccCase) -> np.ndarray:
    """Frames that take part per pdf, from the contract's frame tables (not from how the case was built)."""
    pdf, _fw = R.frame_tables(case.tm, case.ali, case.weights)
    return np.bincount(pdf[pdf >= 0], minlength=case.am.num_pdfs)


def gmm_expect(case: R.AccCase, gauss=None):
    """(occ, mean_acc, var_acc, tid_count, tot_count) in float64 numpy, every frame's weight on the Gaussian ``gauss[t]`` (its
    pdf's only one by default): exact whatever the order on the exact tiers."""
    pdf, fw = R.frame_tables(case.tm, case.ali, case.weights)
    took = pdf >= 0
    g = (case.am.pdf_offsets[np.maximum(pdf, 0)] if gauss is None else np.asarray(gauss))[took]
    w = fw[took].astype(np.float64)
    x = case.feats[took].astype(np.float64)
    G, D = case.am.num_gauss, case.am.dim
    occ, mean, var = np.zeros(G), np.zeros((G, D)), np.zeros((G, D))
    np.add.at(occ, g, w)
    np.add.at(mean, g, w[:, None] * x)
    np.add.at(var, g, w[:, None] * x * x)
    assert np.abs(var).max() < 2.0 ** 52
    return occ, mean, var, R.tid_counts(case.ali, pdf, len(case.weights)), float(w.sum())


# ---- mixtures of 1 – 128 Gaussians at many pdfs ---------------------------------------------------------------------------------
MIXED_PDFS = 301


def mixed_sizes():
    return tuple(MR.ONE_HOT_SIZES[i % len(MR.ONE_HOT_SIZES)] for i in range(MIXED_PDFS))


def mixed_frames(Cg, Cm) -> tuple:
    """0 – 3 frames on most pdfs; 7·Cm + 1 (eight units) on a 128-Gaussian pdf, 8·Cm + 1 (nine) on a 5-Gaussian pdf and
    9·Cg + 1 on a 65-Gaussian pdf, each in the middle of the model."""
    sizes = mixed_sizes()
    rng = np.random.default_rng(4500)
    counts = rng.integers(0, 4, size=MIXED_PDFS)
    mid = 7 * (MIXED_PDFS // 14)
    for n, c in ((128, 7 * Cm + 1), (5, 8 * Cm + 1), (65, 9 * Cg + 1)):
        counts[mid + sizes[mid: mid + 7].index(n)] = c
    return tuple(int(c) for c in counts)


def mixed_case(dim, Cg, Cm):
    """(case, gauss) of tests/mllt_ref.one_hot_case over ``mixed_sizes()`` with ``mixed_frames``."""
    return MR.one_hot_case(dim, mixed_frames(Cg, Cm), mixed_sizes())


# ---- LDA statistics -------------------------------------------------------------------------------------------------------------
def lda_case(dim, ctx, lengths, n_classes, long_classes=(), order="shuffled") -> lda_ref.Case:
    """tests/lda_ref.integer_case over ``lengths`` with ``n_classes``: ``long_classes`` = ((class, frames), …) get exactly that
    many frames, at random places and with weights ½, 1 and 2 only (all of them take part); the other frames are spread
    evenly over the other classes.  ``order`` "aligned": the same transition-ids, as many of each, in runs (``in_runs``)."""
    rng = np.random.default_rng(4600 + 7 * dim + n_classes + int(np.sum(lengths)) % 1000)
    T = int(np.sum(lengths))
    named = [c for c, _n in long_classes]
    others = np.array([c for c in range(n_classes) if c not in named])
    cls = others[rng.integers(0, len(others), size=T)]
    spots = rng.permutation(T)
    k = 0
    for c, n in long_classes:
        cls[spots[k: k + n]] = c
        k += n
    case = lda_ref.integer_case(rng, dim, ctx, lengths, n_classes, class_of_frame=cls)
    for c in named:
        case.tid_weight[1 + 4 * c: 5 + 4 * c] = [1.0, 0.5, 1.0, 2.0]
    if order == "aligned":
        case.ali = in_runs(case.ali, rng)
    return case


def in_runs(ali, rng) -> np.ndarray:
    """The transition-ids of ``ali``, as many of each, in runs whose lengths cycle through RUN_LENGTHS, the runs shuffled: what
    the LDA statistics' own run compression (lda_lookup_kernel) sees in production.  Ids of weight 0 cut the runs."""
    ids, counts = np.unique(ali, return_counts=True)
    runs = []
    for i, (t, n) in enumerate(zip(ids, counts)):
        k, j = 0, i % len(RUN_LENGTHS) if n > 3 else 0
        while k < n:
            m = min(RUN_LENGTHS[j % len(RUN_LENGTHS)], n - k)
            runs.append((t, m))
            k, j = k + m, j + 1
    return np.concatenate([np.full(runs[j][1], runs[j][0], np.int32) for j in rng.permutation(len(runs))])


def lda_counts(case: lda_ref.Case) -> np.ndarray:
    cls, _w = lda_ref.frame_tables(case)
    return np.bincount(cls[cls >= 0], minlength=case.n_classes)


# ---- tree statistics ------------------------------------------------------------------------------------------------------------
SPARSE_PHONES = (1, 2, 15, 16, 17, 255, 256, 4095, 4096, 65534, 65535)
SPARSE_ONE_STATE = (2, 16, 4095, 65535)
SPARSE_CI = (1, 65534)                        # one small, one above 2¹⁵
SPARSE_LENGTHS = (0, 1, 65, 129, 700, 3000)
PHONE_COUNTS = (15, 16, 255, 256, 4095, 4096)


def sparse_tm(phones, one_state, classes=(0, 1, 2)) -> TransitionModel:
    """tests/tree_ref.mono_tm over a sparse set of phone ids; ``classes``: the pdf-classes of the three-state entry's states
    (the one-state entry has the first)."""
    bakis = [K.HmmState(c, c, [(i, 0.75), (i + 1, 0.25)]) for i, c in enumerate(classes)] + [K.HmmState(-1, -1, [])]
    single = [K.HmmState(classes[0], classes[0], [(0, 0.5), (1, 0.5)]), K.HmmState(-1, -1, [])]
    ids = np.asarray(sorted(phones), dtype=np.int32)
    phone2idx = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
    for p in ids:
        phone2idx[p] = 1 if int(p) in one_state else 0
    raw_tm, _am, _tree = mle.init_mono(K.HmmTopology(ids, phone2idx, [bakis, single]), 2)
    return TransitionModel(raw_tm)


def _tree_case(tm, utts, dim, ci, seed) -> TR.Case:
    rng = np.random.default_rng(seed)
    fo = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    ali = np.concatenate(list(utts) + [np.zeros(0, np.int32)]).astype(np.int32)
    return TR.Case(tm, rng.integers(-8, 9, size=(len(ali), dim)).astype(np.float32), fo, ali, tuple(ci))


@lru_cache(maxsize=None)
def tree_sparse_case(dim=13) -> TR.Case:
    """Phone ids up to 65 535 in windows of every mix; the 700-frame utterance starts with three one-frame phones 65 535, so the
    largest key there is holds 65 535 in all three fields."""
    tm = sparse_tm(SPARSE_PHONES, SPARSE_ONE_STATE)
    rng = np.random.default_rng(4700)
    utts = [TR.utterance(rng, tm, n, [65535, 65535, 65535, 4096, 65534, 1] if n == 700 else None) for n in SPARSE_LENGTHS]
    return _tree_case(tm, utts, dim, SPARSE_CI, 4701)


@lru_cache(maxsize=None)
def tree_phone_count_case(n_phones, dim=13) -> TR.Case:
    """Three phones of which the largest id is ``n_phones``: the width of the packed sort key follows it."""
    tm = sparse_tm((1, 2, n_phones), (2,))
    rng = np.random.default_rng(4800 + n_phones)
    utts = [TR.utterance(rng, tm, n, [n_phones, n_phones, 2, n_phones]) for n in (1, 65, 129, 300)]
    return _tree_case(tm, utts, dim, (1,), 4801 + n_phones)


@lru_cache(maxsize=None)
def tree_pdf_class_case(dim=13) -> TR.Case:
    """A topology whose states carry pdf-classes 0, 254 and 255."""
    tm = sparse_tm(range(1, 10), TR.ONE_STATE, classes=(0, 254, 255))
    rng = np.random.default_rng(4900)
    return _tree_case(tm, [TR.utterance(rng, tm, n) for n in (65, 129, 300)], dim, TR.CI, 4901)


@lru_cache(maxsize=None)
def tree_long_event_case(chunk, dim=13, integer=True) -> TR.Case:
    """A context-independent three-state phone whose first two states last 8·chunk + 1 and 17·chunk frames: two events of 9
    and 17 chunks; then a few frames of other phones."""
    tm = TR.mono_tm()
    rng = np.random.default_rng(5000)
    ali = np.concatenate([TR.phone_path(tm, 1, [8 * chunk + 1, 17 * chunk, 3]), TR.phone_path(tm, 4, [3, 2, 2]),
                          TR.phone_path(tm, 3, [1]), TR.phone_path(tm, 5, [2, 40, 2])])
    case = _tree_case(tm, [ali], dim, TR.CI, 5001)
    if not integer:
        case.feats = (rng.normal(size=case.feats.shape) * np.linspace(12.0, 1.5, dim) + rng.normal(0, 5.0, size=dim)).astype(np.float32)
    return case


@lru_cache(maxsize=None)
def tree_step_event_case(chunk, dim=13) -> TR.Case:
    """A context-independent three-state phone whose states last 7·chunk + 1, 8·chunk + 1 and 9·chunk + 1 frames: events of
    8, 9 and 10 chunks, so that 7, 8 and 9 partials are added to an event's first (eight a step, then the rest)."""
    tm = TR.mono_tm()
    ali = np.concatenate([TR.phone_path(tm, 1, [7 * chunk + 1, 8 * chunk + 1, 9 * chunk + 1]), TR.phone_path(tm, 4, [3, 2, 2]),
                          TR.phone_path(tm, 3, [1])])
    return _tree_case(tm, [ali], dim, TR.CI, 5002)


def de_bruijn(k, n=3):
    """The de Bruijn sequence B(k, n) over 0 … k − 1 (the standard Lyndon-word construction): kⁿ symbols."""
    seq, a = [], [0] * (k * n)

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def small_event_phones(cus) -> int:
    """The smallest k with k³ above the 4 · 8 · CUs wavefronts of the short events' kernel."""
    k = 2
    while k ** 3 <= 32 * cus:
        k += 1
    return k


@lru_cache(maxsize=None)
def tree_every_frame_case(k, dim=13) -> TR.Case:
    """One utterance of one-frame phones in de Bruijn order over k one-state phones: every frame is an event of its own."""
    tm = TR.mono_tm(k, tuple(range(1, k + 1)))
    first = {p: TR.phone_path(tm, p, [1])[0] for p in range(1, k + 1)}
    ali = np.array([first[s + 1] for s in de_bruijn(k)], dtype=np.int32)
    assert len(ali) == k ** 3
    return _tree_case(tm, [ali], dim, (), 5100 + k)


@lru_cache(maxsize=None)
def tree_one_event_case(chunk, cus) -> TR.Case:
    """One context-independent one-state phone over eight utterances of more than chunk · 4 · 8 · CUs frames together, at dim 1:
    one event of more units than the long events' kernel has wavefronts."""
    tm = TR.mono_tm()
    forward, loop = TR.phone_path(tm, 3, [2])
    need = chunk * 32 * cus + 1
    lens = [need // 8 + 1 + 37 * u for u in range(8)]
    utts = []
    for n in lens:
        u = np.full(n, loop, np.int32)
        u[0] = forward
        utts.append(u)
    return _tree_case(tm, utts, 1, (3,), 5200)


# ---- real features: one long segment per kernel ----------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def soft_long_case(dim, long_frames) -> R.AccCase:
    """Overlapping mixtures of 2, 1, 5 and 17 Gaussians with real frames drawn from them; the first pdf holds ``long_frames``,
    weights 1, 0.5 and 0.3, some frames that take no part."""
    rng = np.random.default_rng(5300 + dim + long_frames % 97)
    sizes = [2, 1, 5, 17]
    gconsts, mi, iv, offs = [], [], [], [0]
    for n in sizes:                      # tests/mllt_ref.grouped_soft_case's model: means √(3 / dim) apart, neighbours overlap
        w = rng.dirichlet(np.ones(n)) if n > 1 else np.ones(1)
        mean = rng.normal(0, np.sqrt(3.0 / dim), size=(n, dim))
        var = rng.uniform(0.5, 4.0, size=(n, dim))
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean / var).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean / var).astype(np.float32)); iv.append((1.0 / var).astype(np.float32))
        offs.append(offs[-1] + n)
    am = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    P = len(sizes)
    pdfs = rng.permutation(np.repeat(np.arange(P), [long_frames + 40, 300, 150, 200]))
    feats = helpers.fmllr_draw(rng, am, pdfs)
    weights = rng.choice(np.array([1.0, 0.5, 0.3], np.float32), size=2 * P + 1).astype(np.float32)
    ali = (2 * pdfs + 1 + rng.integers(0, 2, size=len(pdfs))).astype(np.int32)
    first = np.flatnonzero(pdfs == 0)
    ali[first[:20]] = 0
    ali[first[20:40]] = 2 * P + 1 + rng.integers(0, 5, size=20)
    return R.AccCase(f"soft long dim {dim}", am, helpers.fmllr_tm(P), feats, ali, weights)
