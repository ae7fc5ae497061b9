"""What the stages' wrappers share on the torch and numpy side; the ctypes side (``check``, ``twin_check``, ``_ptr``, ``_np_ptr``) is
in ``_lib``."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


def device_model(engine, model, arrays):
    """The arrays ``arrays()`` yields for ``model`` as device tensors, computed and uploaded once per model object and device: kept
    on the model, one device at a time."""
    cache = model.__dict__.setdefault("_device_arrays", {})
    key = str(engine.device)
    if key not in cache:
        cache.clear()
        cache[key] = tuple(torch.from_numpy(a).to(engine.device) for a in arrays())
    return cache[key]


def check_device_frames(what: str, feats, ali) -> None:
    if feats.dtype != torch.float32 or not feats.is_cuda or not ali.is_cuda:
        raise _lib.MfaHipError(f"{what}: features must be float32 and, like the alignments, on the device")


def frame_pdf_weight(ali: np.ndarray, id2pdf: np.ndarray, w: np.ndarray):
    """Every frame's pdf (int32; −1 for a transition-id outside the table) and weight (float32; 0 there) from its alignment, as the
    twins of the alignment statistics take them."""
    ok = (ali > 0) & (ali < id2pdf.shape[0])
    safe = np.where(ok, ali, 0)
    return np.where(ok, id2pdf[safe], -1).astype(np.int32), np.where(ok, w[safe], np.float32(0)).astype(np.float32)


def accumulators(st, dev=None, tid_count: bool = False):
    """A ``GmmStats`` as the accumulators a call adds to — (occ, mean, var, tot = [tot_like, tot_count]), with ``tid_count`` also the
    transition-id counts — as tensors on ``dev``, or for the host twins (``dev`` None) as contiguous numpy arrays."""
    acc = [np.ascontiguousarray(a, dtype=np.float64) for a in (st.occ, st.mean_acc, st.var_acc, [st.tot_like, st.tot_count])]
    if tid_count:
        acc.append(np.ascontiguousarray(st.tid_count, dtype=np.int64))
    return acc if dev is None else [torch.from_numpy(a).to(dev) for a in acc]


def store_accumulators(st, acc) -> None:
    """The accumulators of either kind back into the ``GmmStats`` as numpy arrays and floats."""
    occ, mean, var, tot, *cnt = (a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in acc)
    st.occ, st.mean_acc, st.var_acc = occ, mean, var
    st.tot_like, st.tot_count = float(tot[0]), float(tot[1])
    if cnt:
        st.tid_count = cnt[0]
