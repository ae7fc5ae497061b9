"""Ragged arrays on the host: pieces laid end to end and the offsets that say where each starts.

numpy only — no torch, no device: ``kalpy_api`` and ``finetune`` import this at module top without pulling torch in.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def offsets(lengths, dtype=np.int64) -> np.ndarray:
    """Lengths of n pieces laid end to end → where each starts, and the total last: [0, l0, l0 + l1, …], ``dtype`` [n + 1]."""
    return np.concatenate([[0], np.cumsum(lengths)]).astype(dtype)


def max_len(off) -> int:
    """The longest piece of an offsets array [n + 1]; 0 when there are no pieces."""
    return int(np.diff(off).max()) if len(off) > 1 else 0


def _rows_by_group(rows: np.ndarray, n_groups: int) -> Tuple[np.ndarray, np.ndarray]:
    """Utterances listed group by group (stable) and each group's range in that list, as the per-speaker kernels take them:
    int32 [n], int32 [n_groups + 1].  A group may be empty."""
    return np.argsort(rows, kind="stable").astype(np.int32), offsets(np.bincount(rows, minlength=n_groups), np.int32)


def _speaker_groups(utt2spk) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Speaker labels of any kind → (sorted distinct labels, each utterance's row among them, ``_rows_by_group`` of the rows)."""
    spk_ids, inv = np.unique(np.asarray(utt2spk), return_inverse=True)
    return (spk_ids, inv) + _rows_by_group(inv, len(spk_ids))


class RaggedView:
    """``np.split(flat, offsets[1:-1])`` without making the pieces up front: piece u is ``flat[offsets[u]: offsets[u + 1]]``."""

    def __init__(self, flat: np.ndarray, offsets: np.ndarray):
        self.flat, self.offsets = flat, offsets

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, u):
        if isinstance(u, slice):
            return [self[k] for k in range(*u.indices(len(self)))]
        if u < 0:
            u += len(self)
        return self.flat[int(self.offsets[u]): int(self.offsets[u + 1])]

    def __iter__(self):
        for u in range(len(self)):
            yield self[u]
