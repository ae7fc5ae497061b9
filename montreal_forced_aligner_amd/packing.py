"""Decoding graphs in the device layout: ``PackedGraphs`` (what the decoders and the lazy scorer read) and
``GraphPacking``, the packing methods of ``AlignmentEngine``.

``GraphPacking`` uses of the engine: ``lib``, ``ctx``, ``stream``, ``_dev``, ``next_staging`` and ``slot_class`` (the loaded
model's slot classes, set by ``load_gmm``).
"""
from __future__ import annotations

import os
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, hostcpu
from ._lib import GraphBatch, ScorePlan, check
from .kaldi_io import Fst
from .model import TransitionModel
from .ragged import RaggedView, max_len, offsets
from .staging import StagingPool


def _flatten_fsts(fsts: Sequence[Fst]):
    """A list of graphs end to end: (state_off [n + 1], arc_base [n + 1], arc_off int32 [ΣS + n], final float32 [ΣS], arcs)."""
    arc_off = np.concatenate([f.arc_offsets.astype(np.int32) for f in fsts]) if len(fsts) else np.zeros(0, np.int32)
    final = np.concatenate([f.final for f in fsts]).astype(np.float32)
    return (offsets([f.num_states for f in fsts]), offsets([f.num_arcs for f in fsts]), arc_off, final,
            np.concatenate([f.arcs for f in fsts]))


@dataclass
class PackedGraphs:
    """Graphs of a batch in the device layout mfa_align_batch consumes (see mfa_graph_batch)."""

    n_utt: int
    max_states: int
    max_arcs: int
    total_arcs: int
    tensors: Dict[str, torch.Tensor]
    pdf_list: torch.Tensor      # int32 [ΣP_u] (slot-sorted per utterance)
    pdf_off: torch.Tensor       # int64 [n_utt+1]
    class_counts: torch.Tensor  # int32 [n_utt,6]
    pdf_off_host: np.ndarray
    pdf_lists_host: Sequence[np.ndarray]                  # per-utterance views of the host copy of pdf_list
    pdf_first_frame: Optional[torch.Tensor] = None        # int32 [ΣP_u]: first frame a pdf can be asked for
    pdf_first_frame_host: Optional[List[np.ndarray]] = None
    # lazy (windowed) scoring keys — mfa_score_plan: running max inside each class of the longest-path depth of a pdf's
    # source states, and {BFS depth, longest-path depth} of every graph state
    pdf_last_depth: Optional[torch.Tensor] = None         # int32 [ΣP_u]
    state_depth: Optional[torch.Tensor] = None            # int32 [ΣS_u, 2]
    # class-0 columns laid out in `groups` runs (pdf id mod groups), one per XCD of the scoring kernel: columns per run
    groups: int = 1
    group_counts: Optional[torch.Tensor] = None           # int32 [n_utt, groups]

    def plan(self) -> ScorePlan:
        if self.pdf_last_depth is None or self.state_depth is None or self.pdf_first_frame is None:
            raise _lib.MfaHipError("these graphs were packed without depth keys (lazy scoring needs them)")
        return ScorePlan(self.pdf_list.data_ptr(), self.pdf_off.data_ptr(), self.class_counts.data_ptr(),
                         self.pdf_first_frame.data_ptr(), self.pdf_last_depth.data_ptr(), self.state_depth.data_ptr(),
                         max_len(self.pdf_off_host), int(self.groups),
                         self.group_counts.data_ptr() if self.group_counts is not None else None)

    @property
    def has_eps(self) -> bool:
        """Some graph of the batch has epsilon input arcs (the decoder then runs ProcessNonemitting after every frame)."""
        return self.tensors.get("state_nemit") is not None

    def hard_bounds(self) -> Tuple[int, int]:
        """(max_tokens, bp_tokens_per_frame) that the decoder's capacity statuses cannot occur with: one token per graph state
        — and, for graphs with epsilon arcs, room behind the back-pointer trail for the path the traceback writes there
        (T + E arc indices, E ≤ T·S in the worst case: half a record per frame and state).

        The exception: the back-pointer bound always holds, the token bound only while the decoder's tables for one token
        per state fit its 160 KiB of LDS.  Beyond that the launch plan (csrc/viterbi_plan.hpp) halves the token capacity
        until they fit, and an utterance that keeps more tokens alive than that comes back with status 3 all the same.
        For graphs of about 3.8 arcs a state this starts at 2 881 states, at 1 921 when the batch holds epsilon arcs
        (tests/native/viterbi_plan_check.cpp measures it; ``mfa_debug_viterbi_plan`` answers for a given batch: N below
        ``max_states`` rounded up to 64).  ``engine.redo_capacity`` therefore sends what still reports a capacity status
        after this step to the general decoder, which has no such limit."""
        s = max(1, int(self.max_states))
        return s, s + (s // 2 + 2 if self.has_eps else 0)

    def struct(self) -> GraphBatch:
        t = self.tensors
        nemit = t.get("state_nemit")
        return GraphBatch(self.n_utt, t["state_off"].data_ptr(), t["arc_base"].data_ptr(), t["start"].data_ptr(),
                          t["arc_off"].data_ptr(), t["final"].data_ptr(), t["arc_next"].data_ptr(),
                          t["arc_weight"].data_ptr(), t["arc_col"].data_ptr(), t["arc_ilabel"].data_ptr(),
                          t["arc_olabel"].data_ptr(), nemit.data_ptr() if nemit is not None else None)


class GraphPacking:
    """Host graphs → ``PackedGraphs``, and the host-side graph queries that go with it."""

    def sort_pdf_list(self, pdfs: np.ndarray, first_frame: Optional[np.ndarray] = None):
        """Order a pdf list by slot class as the scoring kernels require; returns (sorted, counts[6]) or, with
        ``first_frame`` keys, (sorted, counts[6], sorted keys) with ascending keys inside each class
        (mfa_gmm_sort_pdf_list / mfa_gmm_sort_pdf_list_keyed)."""
        pdfs = np.ascontiguousarray(pdfs, dtype=np.int32).copy()
        counts = np.zeros(6, dtype=np.int32)
        if first_frame is None:
            check(self.ctx, self.lib.mfa_gmm_sort_pdf_list(self.ctx, pdfs.ctypes.data, len(pdfs), counts.ctypes.data),
                  "mfa_gmm_sort_pdf_list")
            return pdfs, counts
        keys = np.ascontiguousarray(first_frame, dtype=np.int32).copy()
        check(self.ctx, self.lib.mfa_gmm_sort_pdf_list_keyed(self.ctx, pdfs.ctypes.data, keys.ctypes.data, len(pdfs),
                                                             counts.ctypes.data), "mfa_gmm_sort_pdf_list_keyed")
        return pdfs, counts, keys

    def state_first_frames(self, fst: Fst) -> np.ndarray:
        """depth[s] = fewest arcs from the start state to s = first frame a token can sit on s (mfa_fst_first_frames)."""
        arc_off = np.ascontiguousarray(fst.arc_offsets, dtype=np.int32)
        nxt = np.ascontiguousarray(fst.arcs["nextstate"], dtype=np.int32)
        depth = np.empty(fst.num_states, dtype=np.int32)
        if self.lib.mfa_fst_first_frames(fst.num_states, arc_off.ctypes.data, nxt.ctypes.data, int(fst.start),
                                         depth.ctypes.data) != 0:
            raise _lib.MfaHipError("mfa_fst_first_frames: malformed graph")
        return depth

    def state_last_depths(self, fst: Fst, bfs_depth: Optional[np.ndarray] = None) -> np.ndarray:
        """m[s] = smallest BFS depth among the states reachable from s (mfa_fst_last_depths): non-decreasing along every
        arc — the lower bound of the lazy-scoring band."""
        arc_off = np.ascontiguousarray(fst.arc_offsets, dtype=np.int32)
        nxt = np.ascontiguousarray(fst.arcs["nextstate"], dtype=np.int32)
        bfs = np.ascontiguousarray(self.state_first_frames(fst) if bfs_depth is None else bfs_depth, dtype=np.int32)
        depth = np.zeros(fst.num_states, dtype=np.int32)
        if self.lib.mfa_fst_last_depths(fst.num_states, arc_off.ctypes.data, nxt.ctypes.data, int(fst.start), bfs.ctypes.data,
                                        depth.ctypes.data) < 0:
            raise _lib.MfaHipError("mfa_fst_last_depths: malformed graph")
        return depth

    @staticmethod
    def needs_general_decoder(fst: Fst) -> bool:
        """True for graphs the wavefront-parallel decoder does not take: a state with more than 64 emitting (or more than 64
        epsilon) arcs.  Epsilon input arcs as such are fine: ``pack_graphs`` stores every state's arcs [emitting | epsilon]
        and the decoder runs ProcessNonemitting after every frame."""
        if not fst.num_arcs:
            return False
        eps = fst.arcs["ilabel"] == 0
        deg = np.diff(fst.arc_offsets)
        if not eps.any():
            return bool(int(deg.max()) > 64)
        src = np.repeat(np.arange(fst.num_states), deg)
        n_eps = np.bincount(src[eps], minlength=fst.num_states)
        return bool(int(n_eps.max()) > 64 or int((deg - n_eps).max()) > 64)

    def _arc_tensors(self, state_off, arc_base, starts, arc_off, final, arcs, arc_col: torch.Tensor) -> Dict[str, torch.Tensor]:
        """mfa_graph_batch's arrays on the device from host arc records, one plain upload per column (``arc_col``: uploaded
        by the caller, whose staging differs)."""
        return dict(
            state_off=self._dev(state_off), arc_base=self._dev(arc_base), start=self._dev(starts),
            arc_off=self._dev(arc_off), final=self._dev(final),
            arc_next=self._dev(arcs["nextstate"].astype(np.int32)), arc_weight=self._dev(arcs["weight"].astype(np.float32)),
            arc_col=arc_col, arc_ilabel=self._dev(arcs["ilabel"].astype(np.int32)),
            arc_olabel=self._dev(arcs["olabel"].astype(np.int32)),
        )

    def pack_graphs_general(self, fsts: Sequence[Fst], tm: TransitionModel) -> PackedGraphs:
        """Device layout for the general-graph decoder (mfa_align_general_batch): graphs may hold epsilon input arcs
        (ilabel 0) and states of any out-degree.  One score column per pdf, no depth keys (scores are computed densely)."""
        n = len(fsts)
        state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
        if np.any(arcs["ilabel"] < 0) or np.any(arcs["ilabel"] > tm.num_transition_ids):
            raise _lib.MfaHipError("a graph arc carries an input label outside the model's transition-ids")
        pdf_of_arc = tm.id2pdf[arcs["ilabel"]]            # -1 for epsilon arcs
        cols = np.zeros(arcs.shape[0], dtype=np.int32)
        pdf_lists, counts = [], []
        lut = np.full(tm.num_pdfs, -1, dtype=np.int32)
        for u in range(n):
            a0, a1 = int(arc_base[u]), int(arc_base[u + 1])
            pa = pdf_of_arc[a0:a1]
            emit = pa >= 0
            pl, cc = self.sort_pdf_list(np.unique(pa[emit])) if emit.any() else (np.zeros(0, np.int32), np.zeros(6, np.int32))
            lut[pl] = np.arange(pl.shape[0], dtype=np.int32)
            cols[a0:a1] = np.where(emit, lut[np.maximum(pa, 0)], 0)
            pdf_lists.append(pl)
            counts.append(cc)
        pdf_off = offsets([len(p) for p in pdf_lists])
        t = self._arc_tensors(state_off, arc_base, np.array([f.start for f in fsts], dtype=np.int32), arc_off, final, arcs,
                              self._dev(cols))
        return PackedGraphs(n, max_len(state_off), max_len(arc_base), int(arc_base[-1]), t,
                            self._dev(np.concatenate(pdf_lists).astype(np.int32) if n else np.zeros(0, np.int32)),
                            self._dev(pdf_off), self._dev(np.stack(counts).astype(np.int32)), pdf_off, pdf_lists)

    def pack_graphs(self, fsts: Sequence[Fst], tm: TransitionModel, cluster_gap: Optional[int] = 32,
                    groups: Optional[int] = None, pool: Optional[StagingPool] = None) -> PackedGraphs:
        """Concatenate per-utterance graphs (with transition probabilities already applied) into the device layout.

        Score columns: one per (pdf, depth cluster) of the utterance.  A pdf whose arcs leave states far apart in the graph
        (the same phone in two words) gets one column per cluster of occurrences — occurrences whose BFS depths differ by
        more than ``cluster_gap``, or lie in different ``cluster_gap``-wide depth ranges, start a new column — so that the
        lazy-scoring band, which is a range of graph depths, does not have to keep the pdf alive for everything in
        between (optional silence after every word would otherwise chain into one column spanning the utterance).
        ``cluster_gap=None``: one column per pdf.

        ``groups`` (default 8, env MFA_PLAN_GROUPS): the single-block pdfs' columns are laid out in that many runs — pdf id
        mod groups — so that the lazy scoring kernel can give each run to one XCD (mfa_build_score_plan_grouped)."""
        if groups is None:
            groups = int(os.environ.get("MFA_PLAN_GROUPS", "8"))
        if cluster_gap == 32 and os.environ.get("MFA_PLAN_SPAN"):          # (diagnostics: tools/band_study.py)
            cluster_gap = int(os.environ["MFA_PLAN_SPAN"])
        n = len(fsts)
        whole = getattr(fsts, "arcs", None) is not None and len(getattr(fsts, "state_off", ())) == n + 1
        columns = whole and getattr(fsts, "arc_pdf", None) is not None and getattr(fsts, "arc_next", None) is not None \
            and getattr(fsts, "arc_off32", None) is not None
        if whole:
            # a batch from the native compiler (graph_native.FstBatch): its elements are views of these arrays
            state_off, arc_base = np.ascontiguousarray(fsts.state_off, dtype=np.int64), np.ascontiguousarray(fsts.arc_base, dtype=np.int64)
            arc_off = fsts.arc_off32 if columns else fsts.arc_off.astype(np.int32)
            final, arcs = np.ascontiguousarray(fsts.final, dtype=np.float32), fsts.arcs
        else:
            state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
        if self.slot_class is None:
            raise _lib.MfaHipError("pack_graphs needs the acoustic model's slot classes: call load_gmm first")
        nemit = None          # emitting arcs per state, for graphs with epsilon input arcs
        if columns:
            # (the compiler produced next-state and pdf columns; an input label outside the model was refused there)
            nxt, pdf_of_arc = fsts.arc_next, fsts.arc_pdf
            if arcs.shape[0] and (fsts.min_ilabel <= 0 if getattr(fsts, "min_ilabel", None) is not None else int(pdf_of_arc.min()) < 0):
                raise _lib.MfaHipError("a natively compiled batch cannot hold epsilon input arcs")
        else:
            il = arcs["ilabel"]
            if np.any(il < 0) or np.any(il > tm.num_transition_ids):
                raise _lib.MfaHipError("a graph arc carries an input label outside the model's transition-ids")
            is_eps = il == 0
            if is_eps.any():
                # epsilon input arcs (kalpy / Kaldi-compiled graphs): every state's arcs stored [emitting | epsilon], each
                # kind in its original order — FasterDecoder's two loops never see the interleaving (include/mfa_hip.h)
                deg = np.concatenate([np.diff(f.arc_offsets) for f in fsts]).astype(np.int64)
                src = np.repeat(np.arange(deg.shape[0], dtype=np.int64), deg)
                perm = np.argsort(src * 2 + is_eps, kind="stable")
                arcs = arcs[perm]
                is_eps = is_eps[perm]
                n_eps = np.bincount(src[perm][is_eps], minlength=deg.shape[0])
                nemit = (deg - n_eps).astype(np.int32)
                if int(n_eps.max()) > 64 or int(nemit.max()) > 64:
                    raise _lib.MfaHipError("a graph state has more than 64 arcs of a kind; the device decoder supports at most 64 "
                                           "emitting and 64 epsilon arcs per state (needs_general_decoder)")
            pdf_of_arc = np.ascontiguousarray(np.where(il[perm] > 0, tm.id2pdf[np.maximum(il[perm], 0)], -1) if nemit is not None
                                              else tm.id2pdf[il], dtype=np.int32)
            nxt = np.ascontiguousarray(arcs["nextstate"], dtype=np.int32)
        # (the concatenated offsets restart at every utterance: those steps are <= 0 and do not disturb the maximum)
        if columns and getattr(fsts, "max_degree", None) is not None:
            max_deg = int(fsts.max_degree)
        else:
            max_deg = max_len(arc_off)
        if max_deg > 64 and nemit is None:
            raise _lib.MfaHipError(f"a graph state has {max_deg} arcs; the device decoder supports at most 64")
        span = 0 if cluster_gap is None else int(cluster_gap)
        pdf_class = np.ascontiguousarray(self.slot_class, dtype=np.int32)
        # columns (pdf, depth cluster) in kernel order, their depth keys, and every arc's column: one host call for the batch,
        # utterances spread over the host's threads (mfa_build_score_plans_batch); outputs land in reused pinned staging
        # buffers and travel to the device asynchronously
        total_s, total_a = int(state_off[-1]), int(arc_base[-1])
        starts = np.zeros(n, dtype=np.int32) if whole else np.array([f.start for f in fsts], dtype=np.int32)
        # ``pool``: the staging buffers of this batch (the ones a native-compiled batch already lives in, when the caller
        # compiled it with ``alloc=pool.get``); default: the engine's next set
        in_pool = pool is not None and getattr(fsts, "staging", None) is pool
        pool = pool or self.next_staging()
        sd_all = pool.get("sd", max(total_s, 1) * 2, np.int32).reshape(-1, 2)
        cols = pool.get("cols", max(total_a, 1), np.int32)
        cp, cf, cl = (pool.get(k, max(total_a, 1), np.int32) for k in ("cp", "cf", "cl"))
        cc_all = np.zeros((max(n, 1), 6), dtype=np.int32)
        gc_all = np.zeros((max(n, 1), max(groups, 1)), dtype=np.int32)
        n_cols = np.zeros(max(n, 1), dtype=np.int32)
        bad = C.c_int32(-1)
        rc = self.lib.mfa_build_score_plans_batch(n, state_off.ctypes.data, arc_base.ctypes.data, arc_off.ctypes.data,
                                                  nxt.ctypes.data, pdf_of_arc.ctypes.data, starts.ctypes.data,
                                                  int(pdf_class.shape[0]), pdf_class.ctypes.data, span, groups,
                                                  hostcpu.threads(), sd_all.ctypes.data, cols.ctypes.data, cp.ctypes.data,
                                                  cf.ctypes.data, cl.ctypes.data, cc_all.ctypes.data, gc_all.ctypes.data,
                                                  n_cols.ctypes.data, C.byref(bad)) if n else 0
        if rc != 0:
            raise _lib.MfaHipError(f"mfa_build_score_plan: utterance {int(bad.value)}: " +
                                   ("a pdf id outside the loaded model" if rc == -2 else
                                    "unsupported number of plan groups" if rc == -3 else "malformed graph"))
        cols = cols[:total_a]
        n_cols = n_cols[:n].astype(np.int64)
        pdf_off = offsets(n_cols)
        # utterance u's columns sit at [arc_base[u], arc_base[u] + n_cols[u]) of the column arrays: compact them
        take = np.repeat(arc_base[:-1] - pdf_off[:-1], n_cols) + np.arange(int(pdf_off[-1]), dtype=np.int64)
        pdf_all, first_all, last_all = cp[take], cf[take], cl[take]
        pdf_lists = RaggedView(pdf_all, pdf_off)
        first_frames = RaggedView(first_all, pdf_off)
        counts, group_counts = cc_all[:n], gc_all[:n]
        up = lambda a: pool.to_device(a, self.stream)       # noqa: E731  (pinned staging → device, asynchronous)
        if columns:
            # the 16-byte arc records travel once; their four columns are split on the device (strided device copies)
            flat = arcs.view(np.int32).reshape(-1)
            if not in_pool:
                stage = pool.get("arcs_copy", max(total_a, 1) * 4, np.int32)[: total_a * 4]
                stage[:] = flat
                flat = stage
            rec = up(flat).view(-1, 4)
            t = dict(
                state_off=self._dev(state_off), arc_base=self._dev(arc_base), start=self._dev(starts),
                arc_off=up(arc_off) if in_pool else self._dev(arc_off), final=up(final) if in_pool else self._dev(final),
                arc_next=rec[:, 3].contiguous(), arc_weight=rec[:, 2].contiguous().view(torch.float32),
                arc_col=up(cols), arc_ilabel=rec[:, 0].contiguous(), arc_olabel=rec[:, 1].contiguous(),
            )
            del rec
        else:
            t = self._arc_tensors(state_off, arc_base, starts, arc_off, final, arcs, up(cols))
        if nemit is not None:
            t["state_nemit"] = self._dev(nemit)
        sd_dev = up(sd_all[:total_s].reshape(-1)).view(-1, 2)
        return PackedGraphs(n, max_len(state_off), max_len(arc_base), total_a, t, self._dev(pdf_all),
                            self._dev(pdf_off), self._dev(counts), pdf_off, pdf_lists,
                            self._dev(first_all), first_frames, self._dev(last_all),
                            sd_dev, groups,
                            self._dev(group_counts) if groups > 1 else None)
