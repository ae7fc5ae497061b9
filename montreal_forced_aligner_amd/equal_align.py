"""Equal alignment: the first alignment of flat-start training (the reference's ``gmm_align_equal``,
MFA/acoustic_modeling/monophone.py:108) — device call and host twin.  The contract is in include/mfa_hip.h ("Equal
alignment"): a random path through the utterance's graph, its frames spread evenly over the path's self-loops, random numbers
a function of (seed, utterance key, draw index) alone.  Functions of an engine, as in ``stats``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, check
from .kaldi_io import Fst
from .packing import PackedGraphs, _flatten_fsts
from .ragged import max_len

STATUS_OK, STATUS_FAILED = 0, 2


def _keys(keys, n: int) -> np.ndarray:
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    if k.shape != (n,):
        raise ValueError(f"{k.shape[0] if k.ndim == 1 else k.shape} utterance keys for {n} utterances")
    return k


def equal_align(engine, graphs: PackedGraphs, frame_off: np.ndarray, keys, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """mfa_align_equal_batch on packed graphs: (ali int32 [ΣT] transition-ids, status int32 [n]: 0 ok, 2 failed) on the
    device, enqueued on the engine's stream.  ``keys``: one uint32 per utterance, its position in the corpus."""
    n = graphs.n_utt
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    if frame_off.shape != (n + 1,):
        raise ValueError(f"{frame_off.shape[0]} frame offsets for {n} utterances (+ 1)")
    total = int(frame_off[-1]) if n else 0
    ali = torch.zeros(total, dtype=torch.int32, device=engine.device)
    status = torch.full((n,), -1, dtype=torch.int32, device=engine.device)
    gs = graphs.struct()
    d_keys, d_fo = engine._dev(_keys(keys, n)), engine._dev(frame_off)
    check(engine.ctx, engine.lib.mfa_align_equal_batch(engine.ctx, C.byref(gs), _ptr(d_fo), total,
                                                        int(graphs.tensors["final"].shape[0]), _ptr(d_keys),
                                                        int(seed) & 0xFFFFFFFF, _ptr(ali), _ptr(status)), "mfa_align_equal_batch")
    return ali, status


def pack_bare(engine, fsts: Sequence[Fst]) -> PackedGraphs:
    """Graphs in the device layout with no acoustic model involved: the arrays the equal alignment reads, arcs in the order
    the graphs hold them (score columns all 0: not for the decoders)."""
    if not len(fsts):
        raise ValueError("pack_bare: no graphs")
    state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
    t = engine._arc_tensors(state_off, arc_base, np.array([f.start for f in fsts], dtype=np.int32), arc_off, final, arcs,
                            engine._dev(np.zeros(arcs.shape[0], dtype=np.int32)))
    empty = torch.zeros(0, dtype=torch.int32, device=engine.device)
    return PackedGraphs(len(fsts), max_len(state_off), max_len(arc_base), int(arc_base[-1]), t, empty, empty, empty,
                        np.zeros(len(fsts) + 1, dtype=np.int64), [])


def equal_align_host_arrays(state_off, arc_base, start, arc_off, final, arc_next, arc_ilabel, frame_off, keys,
                            seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The host twin (mfa_debug_align_equal_host) on a batch's arrays in mfa_graph_batch's layout: the specification the
    device is held to, bit for bit.  Returns (ali int32 [ΣT], status int32 [n])."""
    lib = _lib.lib()
    state_off, arc_base, frame_off = (np.ascontiguousarray(a, dtype=np.int64) for a in (state_off, arc_base, frame_off))
    start, arc_off, arc_next, arc_ilabel = (np.ascontiguousarray(a, dtype=np.int32) for a in (start, arc_off, arc_next, arc_ilabel))
    final = np.ascontiguousarray(final, dtype=np.float32)
    n = int(state_off.shape[0]) - 1
    keys = _keys(keys, n)
    ali = np.zeros(int(frame_off[-1]) if n else 0, dtype=np.int32)
    status = np.full(n, -1, dtype=np.int32)
    rc = lib.mfa_debug_align_equal_host(n, state_off.ctypes.data, arc_base.ctypes.data, start.ctypes.data, arc_off.ctypes.data,
                                        final.ctypes.data, arc_next.ctypes.data, arc_ilabel.ctypes.data, frame_off.ctypes.data,
                                        keys.ctypes.data, int(seed) & 0xFFFFFFFF, ali.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise _lib.MfaHipError("mfa_debug_align_equal_host: " + ("2^31 frames or more" if rc == -2 else "bad arguments"))
    return ali, status


def equal_align_host(fsts: Sequence[Fst], frame_off: np.ndarray, keys, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The host twin on a list of graphs, arcs in the order the graphs hold them."""
    if not len(fsts):
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    state_off, arc_base, arc_off, final, arcs = _flatten_fsts(fsts)
    return equal_align_host_arrays(state_off, arc_base, np.array([f.start for f in fsts], dtype=np.int32), arc_off, final,
                                   arcs["nextstate"], arcs["ilabel"], frame_off, keys, seed)


def equal_align_host_packed(graphs: PackedGraphs, frame_off: np.ndarray, keys, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The host twin on the arrays a ``PackedGraphs`` holds on the device (arcs in the packed order)."""
    t = {k: graphs.tensors[k].cpu().numpy() for k in ("state_off", "arc_base", "start", "arc_off", "final", "arc_next", "arc_ilabel")}
    return equal_align_host_arrays(t["state_off"], t["arc_base"], t["start"], t["arc_off"], t["final"], t["arc_next"],
                                   t["arc_ilabel"], frame_off, keys, seed)


def path_words(fst: Fst, ali) -> Optional[List[int]]:
    """The output labels (0 dropped) along a path of ``fst`` that spells the transition-ids ``ali`` and ends in a final
    state, or None when there is none: sets of states per consumed label, epsilon input arcs closed, one predecessor kept."""
    off, arcs = fst.arc_offsets, fst.arcs
    nxt, il, ol = arcs["nextstate"], arcs["ilabel"], arcs["olabel"]
    pred = [dict() for _ in range(len(ali) + 1)]

    def close(t):
        stack = list(pred[t])
        while stack:
            s = stack.pop()
            for a in range(int(off[s]), int(off[s + 1])):
                d = int(nxt[a])
                if il[a] == 0 and d != s and d not in pred[t]:
                    pred[t][d] = (t, s, int(ol[a]))
                    stack.append(d)

    pred[0][int(fst.start)] = None
    close(0)
    for t, lab in enumerate(ali):
        for s in list(pred[t]):
            for a in range(int(off[s]), int(off[s + 1])):
                d = int(nxt[a])
                if il[a] == lab and d not in pred[t + 1]:
                    pred[t + 1][d] = (t, s, int(ol[a]))
        close(t + 1)
        if not pred[t + 1]:
            return None
    ends = [s for s in pred[len(ali)] if np.isfinite(fst.final[s])]
    if not ends:
        return None
    words, t, s = [], len(ali), ends[0]
    while pred[t][s] is not None:
        t, s, w = pred[t][s]
        if w:
            words.append(w)
    return words[::-1]
