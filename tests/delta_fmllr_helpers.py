"""Inputs shared by tests/test_gpu_delta_fmllr.py, tests/test_gpu_delta_sat_flow.py and tools/frontend_fuzz.py: the Δ+ΔΔ
feature path with per-speaker fMLLR (CMVN → deltas → transform, no LDA)."""
from __future__ import annotations

import copy
import functools

import numpy as np

from oracle import oracle as O
from tests import helpers

# Frames per utterance: every clamp combination of the ±4 halo (an utterance shorter than the halo on one or both sides), and
# one frame below, at and above the 64-frame tile of the generic kernel and the 128-frame tile of the register-row LDA
# kernel; 300 spans several blocks of either.
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 127, 128, 129, 300)
DIMS = (8, 12, 13, 16)
N_SPK = 3


@functools.lru_cache(maxsize=None)
def kernel_case(dim):
    """One batch per base dimension: (matrices, frame_off, utt2spk = u % 3, W [3, 3·dim, 3·dim+1], per-speaker CMVN
    statistics [3, 2, dim+1] float64 from the oracle).  Computed once; callers must not write to it."""
    rng = np.random.default_rng(7100 + dim)
    mats = [helpers.mfcc_like(rng, T, dim) for T in LENGTHS]
    u2s = (np.arange(len(mats)) % N_SPK).astype(np.int32)
    W = np.stack([helpers.random_affine(rng, 3 * dim, 3 * dim + 1) for _ in range(N_SPK)])
    stats = np.stack([O.cmvn_stats([m for m, s in zip(mats, u2s) if s == k]) for k in range(N_SPK)])
    fo = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    for a in (W, stats, fo, u2s, *mats):
        a.setflags(write=False)
    return mats, fo, u2s, W, stats


@functools.lru_cache(maxsize=None)
def oracle_chain(dim, cmvn):
    """The oracle's whole chain on ``kernel_case(dim)``: per utterance (Δ+ΔΔ of the CMVN-applied matrix, the same through
    the speaker's transform)."""
    mats, _fo, u2s, W, stats = kernel_case(dim)
    out = []
    for m, s in zip(mats, u2s):
        d = O.deltas(O.cmvn_apply(stats[s], m) if cmvn else m)
        out.append((d, O.affine(d, W[s])))
    return out


def seeded_delta_fmllr(n_spk, dim=39, seed=20240):
    """Seeded [n_spk, dim, dim+1] transforms near identity (identity + 0.05·N(0,1), offsets 0.1·N(0,1)): synth.seeded_fmllr
    for the Δ+ΔΔ dimension."""
    rng = np.random.default_rng(seed + 13)
    a = np.eye(dim)[None] + 0.05 * rng.normal(size=(n_spk, dim, dim))
    b = 0.1 * rng.normal(size=(n_spk, dim, 1))
    return np.concatenate([a, b], axis=2).astype(np.float32)


def second_model(rng, am):
    """A perturbed copy of ``am`` with the same layout (the alignment model of the two-model form), gconsts rebuilt so that
    it is a proper GMM."""
    st = copy.copy(am)
    inv = (am.inv_vars * rng.uniform(0.8, 1.25, size=am.inv_vars.shape)).astype(np.float32)
    mean = (am.means_invvars / am.inv_vars) * (1.0 + 0.05 * rng.normal(size=am.means_invvars.shape))
    old = -0.5 * ((am.means_invvars.astype(np.float64) ** 2 / am.inv_vars).sum(axis=1) - np.log(am.inv_vars.astype(np.float64)).sum(axis=1))
    new = -0.5 * ((mean * mean * inv).sum(axis=1) - np.log(inv.astype(np.float64)).sum(axis=1))
    st.inv_vars = inv
    st.means_invvars = (mean * inv).astype(np.float32)
    st.gconsts = (am.gconsts + (new - old)).astype(np.float32)
    return st


class CountingLib:
    """Stands in for ``engine.lib``: counts the feature launches that reach the library."""

    def __init__(self, lib):
        self._lib, self.feats_calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "mfa_feats_batch":
            return fn

        def counted(*a):
            self.feats_calls += 1
            return fn(*a)
        return counted
