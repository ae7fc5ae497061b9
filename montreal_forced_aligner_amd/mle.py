"""Maximum-likelihood re-estimation of an acoustic model from GMM statistics, mixing up, and the flat-start model: the
host half of the reference's training stages (``AmDiagGmm.mle_update(gmm_accs, mixup=, power=)``,
MFA/acoustic_modeling/base.py:788-790; ``gmm_init_mono``, MFA/acoustic_modeling/monophone.py:324).

The accumulation is the device's (``engine.gmm_statistics``); everything here is float64 numpy on ``kaldi_io.RawAmDiagGmm``,
in the manner of ``adapt``.  The rules are Kaldi's (MleDiagGmmUpdate, GetSplitTargets, DiagGmm::Split, gmm-init-mono),
restated from their descriptions (parity unpinned: DESIGN §2).
"""
from __future__ import annotations

import copy
import heapq
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import kaldi_io
from .adapt import MIN_GAUSSIAN_OCCUPANCY, MIN_GAUSSIAN_WEIGHT, _check, gconsts, pdf_offsets
from .engine import GmmStats

MIN_VARIANCE = 1.0e-3
MAX_GAUSSIANS_PER_PDF = 128        # mfa_gmm_acc_batch's limit
MAX_DIM = 48


def mle_update(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats, flags: str = "mvw",
               min_gaussian_occupancy: float = MIN_GAUSSIAN_OCCUPANCY, min_gaussian_weight: float = MIN_GAUSSIAN_WEIGHT,
               min_variance: float = MIN_VARIANCE, remove_low_count_gaussians: bool = True):
    """MleDiagGmmUpdate over every pdf.  In a pdf with Σocc > 0, Gaussian i is re-estimated iff occ_i > min_gaussian_occupancy
    and occ_i / Σocc > min_gaussian_weight:
      "m"  μ = mean_acc / occ rounded to float32;
      "v"  σ² = var_acc / occ − μ² (without "m": var_acc / occ − 2·μ_old·mean_acc / occ + μ_old², about the mean that stays),
           every element floored at min_variance, inv_var = 1 / σ² rounded to float32;
      "w"  w = occ_i / Σocc;
    means_invvars = μ·inv_var in float32.  Every other Gaussian is removed — in index order, and only while the pdf would
    keep at least one Gaussian besides those already marked: the last Gaussian of a pdf is never removed — or, with
    ``remove_low_count_gaussians=False``, kept as it is.  The weights of a pdf are renormalised (in float64, then rounded)
    when "w" is set or a Gaussian was removed, and left bit for bit otherwise; the gconsts of every pdf with statistics are
    recomputed (``adapt.gconsts``), and one that is not finite raises.  A pdf without statistics is kept as it is.
    Returns (new model, Gaussians updated, Gaussians removed, variance elements floored)."""
    if set(flags) - set("mvw"):
        raise ValueError(f"mle_update: update flags {flags!r} (any of 'm', 'v', 'w')")
    offs = _check(raw_am, stats)
    new = kaldi_io.RawAmDiagGmm(raw_am.dim, [], [], [], [])
    updated = removed = floored = 0
    for p in range(raw_am.num_pdfs):
        a, b = int(offs[p]), int(offs[p + 1])
        occ = stats.occ[a:b]
        occ_sum = float(occ.sum())
        w_old = raw_am.weights[p].astype(np.float32)
        iv = raw_am.inv_vars[p].astype(np.float32).copy()
        mi = raw_am.means_invvars[p].astype(np.float32).copy()
        if not occ_sum > 0:
            new.gconsts.append(raw_am.gconsts[p].copy()); new.weights.append(w_old.copy())
            new.means_invvars.append(mi); new.inv_vars.append(iv)
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            share = occ / occ_sum
            mean_ml = stats.mean_acc[a:b] / occ[:, None]
            x2 = stats.var_acc[a:b] / occ[:, None]
        take = (occ > min_gaussian_occupancy) & (share > min_gaussian_weight)
        mu_old = mi / iv                                          # float32: the model's own means
        mu = mu_old.copy()
        if "m" in flags:
            mu[take] = mean_ml[take].astype(np.float32)
        if "v" in flags:
            if "m" in flags:
                var = x2 - mean_ml * mean_ml
            else:
                m0 = mu_old.astype(np.float64)
                var = x2 - 2.0 * m0 * mean_ml + m0 * m0
            low = take[:, None] & ~(var >= min_variance)          # (a NaN is floored too, and then caught by its gconst)
            floored += int(low.sum())
            var = np.where(low, min_variance, var)
            iv[take] = (1.0 / var[take]).astype(np.float32)
        mi[take] = mu[take] * iv[take]
        w = w_old.astype(np.float64)
        if "w" in flags:
            w[take] = share[take]
        keep = np.ones(b - a, dtype=bool)
        if remove_low_count_gaussians:
            marked = 0
            for i in np.flatnonzero(~take):
                if marked < (b - a) - 1:
                    keep[i] = False
                    marked += 1
        if "w" in flags or not keep.all():
            w = w[keep]
            w32 = (w / w.sum()).astype(np.float32)
        else:
            w32 = w_old.copy()
        mi, iv = mi[keep], iv[keep]
        gc = gconsts(w32, mi, iv)
        if not np.isfinite(gc).all():
            raise ValueError(f"mle_update: pdf {p} has a gconst that is not finite (a zero weight, variance or a bad statistic)")
        new.gconsts.append(gc); new.weights.append(w32); new.means_invvars.append(mi); new.inv_vars.append(iv)
        updated += int((take & keep).sum())
        removed += int((~keep).sum())
    return new, updated, removed, floored


def split_targets(pdf_occ: Sequence[float], num_comp: Sequence[int], target_total: int, power: float = 0.25,
                  min_count: float = 20.0) -> np.ndarray:
    """GetSplitTargets: Gaussians per pdf for a total of ``target_total``.  A priority queue on occ^power / components; the
    pdf on top gains a component unless (components + 1)·min_count >= occ, in which case it is retired; until the total is
    reached or every pdf is retired.  Equal priorities: the lower pdf index first, so the result is a function of the input.
    No pdf ever loses a component."""
    occ = np.asarray(pdf_occ, dtype=np.float64)
    n = np.asarray(num_comp, dtype=np.int64).copy()
    if occ.shape != n.shape:
        raise ValueError("split_targets: one occupancy and one component count per pdf")
    total = int(n.sum())
    scaled = np.power(np.maximum(occ, 0.0), power)
    heap = [(-scaled[p] / n[p], p) for p in range(len(n)) if n[p] > 0]
    heapq.heapify(heap)
    while total < target_total and heap:
        _prio, p = heapq.heappop(heap)
        if (n[p] + 1) * min_count >= occ[p]:
            continue                               # retired
        n[p] += 1
        total += 1
        heapq.heappush(heap, (-scaled[p] / n[p], p))
    return n


def mix_up(raw_am: kaldi_io.RawAmDiagGmm, pdf_occ: Sequence[float], target_total: int, power: float = 0.25,
           min_count: float = 20.0, perturb_factor: float = 0.01,
           rng: Optional[np.random.Generator] = None,
           max_per_pdf: Optional[int] = MAX_GAUSSIANS_PER_PDF) -> Tuple[kaldi_io.RawAmDiagGmm, np.ndarray]:
    """AmDiagGmm::SplitByCount: every pdf is split up to its ``split_targets`` count.  One split: the component of largest
    weight (the first on ties) gives half its weight to a copy appended to the pdf; with z ~ N(0, 1) per dimension from
    ``rng`` the copy's mean is μ + perturb_factor·√σ²·z and the original's μ − perturb_factor·√σ²·z; variances are copied
    and the gconsts recomputed.  A target beyond ``max_per_pdf`` Gaussians in a pdf is refused: by default 128, the limit of
    the statistics kernel over alignments; the diagonal UBM, one mixture of up to 2048 (``ubm.split``), passes its own.
    Returns (new model, Gaussians per pdf)."""
    rng = np.random.default_rng(0) if rng is None else rng
    targets = split_targets(pdf_occ, [w.shape[0] for w in raw_am.weights], target_total, power, min_count)
    if max_per_pdf is not None and len(targets) and int(targets.max()) > max_per_pdf:
        raise ValueError(f"mix_up: pdf {int(targets.argmax())} would get {int(targets.max())} Gaussians; the statistics "
                         f"kernel takes at most {max_per_pdf} per pdf")
    new = kaldi_io.RawAmDiagGmm(raw_am.dim, [], [], [], [])
    for p in range(raw_am.num_pdfs):
        w = raw_am.weights[p].astype(np.float32)
        iv = raw_am.inv_vars[p].astype(np.float32)
        mi = raw_am.means_invvars[p].astype(np.float32)
        if targets[p] == w.shape[0]:
            new.gconsts.append(raw_am.gconsts[p].copy()); new.weights.append(w.copy())
            new.means_invvars.append(mi.copy()); new.inv_vars.append(iv.copy())
            continue
        ws, ivs = list(w), [row.copy() for row in iv]
        mus = [row for row in mi.astype(np.float64) / iv.astype(np.float64)]
        while len(ws) < targets[p]:
            i = int(np.argmax(np.asarray(ws)))
            half = np.float32(ws[i] * np.float32(0.5))
            step = perturb_factor * np.sqrt(1.0 / ivs[i].astype(np.float64)) * rng.standard_normal(raw_am.dim)
            ws[i] = half
            ws.append(half); mus.append(mus[i] + step); ivs.append(ivs[i].copy())
            mus[i] = mus[i] - step
        w32, iv2 = np.asarray(ws, dtype=np.float32), np.stack(ivs)
        mi2 = np.stack(mus).astype(np.float32) * iv2
        gc = gconsts(w32, mi2, iv2)
        if not np.isfinite(gc).all():
            raise ValueError(f"mix_up: pdf {p} has a gconst that is not finite")
        new.gconsts.append(gc); new.weights.append(w32); new.means_invvars.append(mi2); new.inv_vars.append(iv2)
    return new, targets


def phone_sets(topology: kaldi_io.HmmTopology, shared_phones: Optional[Sequence[Sequence[int]]] = None) -> List[List[int]]:
    """The phone sets of ``gmm_init_mono``: those given, then every phone of the topology in none of them on its own,
    ordered by their smallest phone."""
    phones = sorted(int(p) for p in topology.phones)
    sets = [sorted(int(p) for p in s) for s in (shared_phones or []) if len(s)]
    seen = [p for s in sets for p in s]
    if len(set(seen)) != len(seen) or set(seen) - set(phones):
        raise ValueError("init_mono: shared phone sets overlap or name phones outside the topology")
    sets += [[p] for p in phones if p not in set(seen)]
    return sorted(sets, key=lambda s: s[0])


def init_mono(topology: kaldi_io.HmmTopology, dim: int, shared_phones: Optional[Sequence[Sequence[int]]] = None):
    """gmm-init-mono: (RawTransitionModel, RawAmDiagGmm, ContextDependency) of a flat-start monophone system.  One pdf per
    (phone set, pdf-class) — the phones of a set share their pdfs and must share a topology entry's pdf-classes —, numbered
    by set, then by pdf-class; one Gaussian each at mean 0, variance 1.  Tree: context width 1, position 0, a table over the
    phone to a table over the pdf-class.  Transition log-probabilities are the topology's."""
    dim = int(dim)
    if dim <= 0 or dim > MAX_DIM:
        raise ValueError(f"init_mono: feature dimension {dim}; the statistics kernel takes 1 to {MAX_DIM}")
    topo = copy.deepcopy(topology)
    n_phone_ids = int(max(topo.phones))
    table: List[Optional[kaldi_io.EventMap]] = [None] * (n_phone_ids + 1)
    pdf_of = {}
    n_pdfs = 0
    for s in phone_sets(topo, shared_phones):
        classes = None
        for ph in s:
            entry = topo.entry_for_phone(ph)
            cl = sorted({c for st in entry for c in (st.forward_pdf_class, st.self_loop_pdf_class) if c >= 0})
            if classes is not None and cl != classes:
                raise ValueError(f"init_mono: phones {s} share pdfs but not their topology's pdf-classes")
            classes = cl
        leaves = {c: n_pdfs + k for k, c in enumerate(classes)}
        n_pdfs += len(classes)
        per_class: List[Optional[kaldi_io.EventMap]] = [None] * (max(classes) + 1 if classes else 0)
        for c, leaf in leaves.items():
            per_class[c] = kaldi_io.EventMap("CE", answer=leaf)
        node = kaldi_io.EventMap("TE", key=-1, table=per_class)
        for ph in s:
            table[ph] = node
            for c, leaf in leaves.items():
                pdf_of[(ph, c)] = leaf
    tree = kaldi_io.ContextDependency(1, 0, kaldi_io.EventMap("TE", key=0, table=table))
    tuples, log_probs = [], [np.float32(0.0)]
    for ph in sorted(int(p) for p in topo.phones):
        for hs, st in enumerate(topo.entry_for_phone(ph)):
            if not st.transitions:
                continue
            tuples.append((ph, hs, pdf_of[(ph, st.forward_pdf_class)], pdf_of[(ph, st.self_loop_pdf_class)]))
            for _dst, prob in st.transitions:
                log_probs.append(np.log(np.float32(prob)))
    raw_tm = kaldi_io.RawTransitionModel(topo, np.asarray(tuples, dtype=np.int32).reshape(-1, 4), np.asarray(log_probs, dtype=np.float32))
    one, zero, unit = np.ones(1, np.float32), np.zeros((1, dim), np.float32), np.ones((1, dim), np.float32)
    gc = gconsts(one, zero, unit)
    raw_am = kaldi_io.RawAmDiagGmm(dim, [gc.copy() for _ in range(n_pdfs)], [one.copy() for _ in range(n_pdfs)],
                                   [zero.copy() for _ in range(n_pdfs)], [unit.copy() for _ in range(n_pdfs)])
    return raw_tm, raw_am, tree


def pdf_occupancies(raw_am: kaldi_io.RawAmDiagGmm, stats: GmmStats) -> np.ndarray:
    """Σ occ per pdf: what ``split_targets`` ranks the pdfs by."""
    offs = pdf_offsets(raw_am)
    return np.add.reduceat(np.concatenate([stats.occ, [0.0]]), offs[:-1]) if raw_am.num_pdfs else np.zeros(0)
