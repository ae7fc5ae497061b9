"""Host staging memory on the way to and from the device: ``StagingPool`` (named, reused, pinned buffers) and
``StagingRing`` (n pools handed out in turn).  torch is used for pinned allocation, copies and events only.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch


class StagingPool:
    """Named host staging buffers in pinned memory, reused from batch to batch (a fresh 200 MB numpy array costs more in page
    faults than the copy it is for).  ``get`` hands out a numpy view; ``to_device`` starts an asynchronous H2D copy of a view
    and remembers it: ``wait`` blocks until every copy started since the last ``wait`` has left the buffers — call it before
    writing into them again."""

    def __init__(self, device: torch.device, pinned: bool = True):
        self.device = device
        self.pinned = pinned
        self._buf: Dict[str, torch.Tensor] = {}
        self._event: Optional[torch.cuda.Event] = None

    def get(self, name: str, count: int, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        need = max(1, int(count)) * dtype.itemsize
        t = self._buf.get(name)
        if t is None or t.numel() < need:
            size = int(need * 1.25) + 64
            t = None
            if self.pinned:
                try:
                    t = torch.empty(size, dtype=torch.uint8, pin_memory=True)
                except RuntimeError:      # pinned allocation refused (constrained container): pageable still works
                    self.pinned = False
            if t is None:
                t = torch.empty(size, dtype=torch.uint8)
            self._buf[name] = t
        return t.numpy()[: int(count) * dtype.itemsize].view(dtype)

    def to_device(self, view: np.ndarray, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        src = torch.from_numpy(view)
        with torch.cuda.device(self.device):
            out = src.to(self.device, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(self.device) if stream is None else stream)
        return out

    def wait(self) -> None:
        if self._event is not None:
            self._event.synchronize()
            self._event = None


class StagingRing:
    """``n`` staging pools handed out round robin: ``next()`` is the pool to fill next, returned once the copies last started
    from it are done — so whatever was staged in a pool may be read until the n-th ``next()`` after the one that gave it."""

    def __init__(self, device: torch.device, n: int, pinned: bool = True):
        self.pools = [StagingPool(device, pinned) for _ in range(n)]
        self._turn = 0

    def next(self) -> StagingPool:
        self._turn = (self._turn + 1) % len(self.pools)
        pool = self.pools[self._turn]
        pool.wait()
        return pool
