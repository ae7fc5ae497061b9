"""Host-side model tables: transition model (derived ids) and the diagonal-GMM acoustic model in SoA form.

Mirrors what the reference obtains from kalpy — ``read_gmm_model`` / ``read_transition_model``
(MFA/alignment/base.py:339, MFA/models.py:481-491) and the model half of
``GmmAligner.__init__`` / ``.boost_silence`` (MFA/alignment/multiprocessing.py:814-815).  The derived-table rules
are Kaldi's ``TransitionModel::ComputeDerived``; the scaling rule is ``AddTransitionProbs``
(Appendix A.8).  These run once per model on the host; the device receives flat arrays.
"""
from __future__ import annotations

import ctypes
import ctypes.util
from dataclasses import dataclass
from typing import Iterable, List, Optional

import numpy as np

from . import kaldi_io

# Kaldi's Exp()/Log() on BaseFloat are the C library's expf/logf; numpy's float32 exp/log are separate SIMD
# implementations that differ in the last bit now and then, so bind libm directly for the model tables.
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def _expf(x) -> np.float32:
    return np.float32(_libm.expf(float(x)))


def _logf(x) -> np.float32:
    return np.float32(_libm.logf(float(x)))


class TransitionModel:
    """Transition-id tables.  transition-ids and transition-states are 1-based as in Kaldi."""

    def __init__(self, raw: kaldi_io.RawTransitionModel):
        self.raw = raw
        self.topo = raw.topo
        self.tuples = raw.tuples
        self.log_probs = raw.log_probs.astype(np.float32)
        n = self.tuples.shape[0]
        state2id = np.zeros(n + 2, dtype=np.int32)
        cur = 1
        for ts in range(1, n + 2):
            state2id[ts] = cur
            if ts <= n:
                phone, hs = int(self.tuples[ts - 1, 0]), int(self.tuples[ts - 1, 1])
                cur += len(self.topo.entry_for_phone(phone)[hs].transitions)
        self.state2id = state2id
        self.num_transition_ids = cur - 1
        nt = cur
        self.id2state = np.zeros(nt, dtype=np.int32)
        self.id2pdf = np.full(nt, -1, dtype=np.int32)
        self.is_self_loop = np.zeros(nt, dtype=np.int32)
        self.is_final = np.zeros(nt, dtype=np.int32)
        self.id2phone = np.zeros(nt, dtype=np.int32)
        self.self_loop_of = np.zeros(n + 1, dtype=np.int32)  # per transition-state, 0 = none
        for ts in range(1, n + 1):
            phone, hs, fwd, slf = (int(x) for x in self.tuples[ts - 1])
            entry = self.topo.entry_for_phone(phone)
            for k, (dst, _p) in enumerate(entry[hs].transitions):
                tid = state2id[ts] + k
                self.id2state[tid] = ts
                self.id2phone[tid] = phone
                self.is_self_loop[tid] = int(dst == hs)
                self.is_final[tid] = int(len(entry[dst].transitions) == 0)
                self.id2pdf[tid] = slf if dst == hs else fwd
                if dst == hs:
                    self.self_loop_of[ts] = tid
        self.num_pdfs = int(max(self.tuples[:, 2].max(), self.tuples[:, 3].max())) + 1
        if self.log_probs.shape[0] != nt:
            raise kaldi_io.KaldiFormatError(
                f"final.mdl: {self.log_probs.shape[0]} log-probs for {nt - 1} transition-ids"
            )

    # Kaldi TransitionModel::GetNonSelfLoopLogProb
    def non_self_loop_log_prob(self, ts: int) -> np.float32:
        sl = int(self.self_loop_of[ts])
        if sl == 0:
            return np.float32(0.0)
        p = np.float32(1.0) - _expf(self.log_probs[sl])
        if p <= 0:
            p = np.float32(1.0e-10)
        return _logf(p)

    def scaled_log_probs(self, transition_scale: float, self_loop_scale: float) -> np.ndarray:
        """``GetScaledTransitionLogProb`` for every transition-id (index 0 = 0)."""
        ts_, sl_ = np.float32(transition_scale), np.float32(self_loop_scale)
        out = np.zeros(self.num_transition_ids + 1, dtype=np.float32)
        for tid in range(1, self.num_transition_ids + 1):
            lp = self.log_probs[tid]
            if ts_ == sl_:
                out[tid] = lp * ts_
            elif self.is_self_loop[tid]:
                out[tid] = sl_ * lp
            else:
                nsl = self.non_self_loop_log_prob(int(self.id2state[tid]))
                out[tid] = np.float32(sl_ * nsl) + np.float32(ts_ * np.float32(lp - nsl))
        return out

    def transition_id(self, ts: int, index: int) -> int:
        return int(self.state2id[ts]) + index

    def mle_update(self, transition_accs):
        """kalpy's ``transition_model.mle_update(transition_accs)``: new transition probabilities from the counts
        (``adapt.transition_update``), in place.  Returns (log-likelihood improvement, count) over the states updated."""
        from . import adapt

        cnt = np.asarray(transition_accs, dtype=np.float64)
        new = adapt.transition_update(self.raw, cnt)
        moved = new.log_probs != self.log_probs
        states = np.unique(self.id2state[moved])
        touched = np.isin(self.id2state, states[states > 0])
        impr = float(np.sum(cnt[touched] * (new.log_probs[touched].astype(np.float64) - self.log_probs[touched])))
        self.raw = new
        self.log_probs = new.log_probs.astype(np.float32)
        return impr, float(cnt[touched].sum())

    def flat_topology(self):
        """Flattened topology arrays in the layout the oracle's orc_tm_derive takes (tests use this)."""
        phone2entry = self.topo.phone2idx.astype(np.int32)
        entry_off = [0]
        trans_off = [0]
        trans_dst: List[int] = []
        for e in self.topo.entries:
            for s in e:
                for dst, _ in s.transitions:
                    trans_dst.append(dst)
                trans_off.append(len(trans_dst))
            entry_off.append(len(trans_off) - 1)
        return (
            phone2entry,
            np.asarray(entry_off, dtype=np.int32),
            np.asarray(trans_off, dtype=np.int32),
            np.asarray(trans_dst, dtype=np.int32),
        )


@dataclass
class DiagGmmModel:
    """All Gaussians of an AmDiagGmm, concatenated (struct of arrays).

    gconsts [G], means_invvars [G, D], inv_vars [G, D], pdf_offsets [P+1] (Gaussian range per pdf); weights [G] (optional:
    the mixture weights, already folded into the gconsts — kept for model adaptation, which writes models back).
    """

    dim: int
    gconsts: np.ndarray
    means_invvars: np.ndarray
    inv_vars: np.ndarray
    pdf_offsets: np.ndarray
    weights: Optional[np.ndarray] = None

    @property
    def num_pdfs(self) -> int:
        return int(self.pdf_offsets.shape[0] - 1)

    @property
    def num_gauss(self) -> int:
        return int(self.gconsts.shape[0])

    @classmethod
    def from_raw(cls, am: kaldi_io.RawAmDiagGmm) -> "DiagGmmModel":
        offs = np.zeros(am.num_pdfs + 1, dtype=np.int32)
        for i, g in enumerate(am.gconsts):
            offs[i + 1] = offs[i] + g.shape[0]
        return cls(
            am.dim,
            np.concatenate(am.gconsts).astype(np.float32),
            np.concatenate(am.means_invvars, axis=0).astype(np.float32),
            np.concatenate(am.inv_vars, axis=0).astype(np.float32),
            offs,
            np.concatenate(am.weights).astype(np.float32),
        )

    def mle_update(self, gmm_accs, update_flags_str: Optional[str] = None, remove_low_count_gaussians: Optional[bool] = None,
                   mixup: Optional[int] = None, power: float = 0.25, min_gaussian_occupancy: Optional[float] = None,
                   perturb_factor: float = 0.01, rng=None):
        """kalpy's ``acoustic_model.mle_update``, in place, in the two forms the reference calls.

        ``mle_update(gmm_accs, update_flags_str="m", remove_low_count_gaussians=False)`` (MFA/alignment/adapting.py; also what
        a call with ``gmm_accs`` alone gives): the mean update of ``adapt.map_update``; no other form without ``mixup``.  Returns (auxiliary-function
        improvement, count): Σ_i Σ_k inv_var·[(μ' − μ)·mean_acc − ½·occ·(μ'² − μ²)] and Σ occ.

        ``mle_update(gmm_accs, mixup=, power=[, min_gaussian_occupancy=])`` (MFA/acoustic_modeling/monophone.py:280-285,
        base.py:788-790): ``mle.mle_update`` — means, variances and weights, low-count Gaussians removed unless told otherwise
        — then ``mle.mix_up`` to ``mixup`` Gaussians.  Returns (auxiliary-function improvement of the update, before mixing
        up, over the pdfs that kept all their Gaussians; Σ occ)."""
        from . import adapt

        if mixup is not None:
            return self._mle_update_training(gmm_accs, update_flags_str or "mvw",
                                             True if remove_low_count_gaussians is None else bool(remove_low_count_gaussians),
                                             mixup, power, 10.0 if min_gaussian_occupancy is None else float(min_gaussian_occupancy),
                                             perturb_factor, rng)
        if update_flags_str not in (None, "m") or remove_low_count_gaussians or min_gaussian_occupancy is not None:
            raise NotImplementedError("mle_update without mixup=: only update_flags_str='m' with remove_low_count_gaussians=False "
                                      "(means only); the training form is mle_update(gmm_accs, mixup=, power=)")
        stats = getattr(gmm_accs, "stats", gmm_accs)
        raw = adapt.raw_from_soa(self)
        new, _updated, _kept = adapt.map_update(raw, stats)
        iv = self.inv_vars.astype(np.float64)
        mu0 = self.means_invvars.astype(np.float64) / iv
        mi1 = np.concatenate(new.means_invvars)
        mu1 = mi1.astype(np.float64) / iv
        impr = float(np.sum(iv * ((mu1 - mu0) * stats.mean_acc - 0.5 * stats.occ[:, None] * (mu1 * mu1 - mu0 * mu0))))
        self.means_invvars = mi1
        self.gconsts = np.concatenate(new.gconsts)
        self.weights = np.concatenate(new.weights)
        return impr, float(stats.occ.sum())

    def _mle_update_training(self, gmm_accs, flags, remove, mixup, power, min_occ, perturb_factor, rng):
        from . import adapt, mle

        stats = getattr(gmm_accs, "stats", gmm_accs)
        raw = adapt.raw_from_soa(self)
        new, _updated, _removed, _floored = mle.mle_update(raw, stats, flags=flags, min_gaussian_occupancy=min_occ,
                                                           remove_low_count_gaussians=remove)

        def aux(am, p, a, b):          # Σ_g occ·gconst + means_invvars·mean_acc − ½·inv_vars·var_acc over one pdf
            return float(np.sum(stats.occ[a:b] * am.gconsts[p].astype(np.float64))
                         + np.sum(am.means_invvars[p].astype(np.float64) * stats.mean_acc[a:b])
                         - 0.5 * np.sum(am.inv_vars[p].astype(np.float64) * stats.var_acc[a:b]))

        impr = 0.0
        for p in range(raw.num_pdfs):
            a, b = int(self.pdf_offsets[p]), int(self.pdf_offsets[p + 1])
            if new.weights[p].shape[0] == b - a:
                impr += aux(new, p, a, b) - aux(raw, p, a, b)
        if mixup is not None and int(mixup) > sum(w.shape[0] for w in new.weights):
            new, _targets = mle.mix_up(new, mle.pdf_occupancies(raw, stats), int(mixup), power, perturb_factor=perturb_factor, rng=rng)
        soa = DiagGmmModel.from_raw(new)
        self.gconsts, self.means_invvars, self.inv_vars = soa.gconsts, soa.means_invvars, soa.inv_vars
        self.pdf_offsets, self.weights = soa.pdf_offsets, soa.weights
        return impr, float(stats.occ.sum())

    def boost_silence(self, factor: float, pdf_ids: Iterable[int]) -> None:
        """Scale the weights of the given pdfs by ``factor`` without renormalising ⇒ gconst += ln(factor).

        Reference: ``aligner.boost_silence(boost, silence_phone_ids)`` (MFA/alignment/multiprocessing.py:803-815);
        Kaldi ``AmDiagGmm`` weight scaling + ``ComputeGconsts``.
        """
        if factor == 1.0:
            return
        lf = _logf(np.float32(factor))
        for p in sorted(set(int(x) for x in pdf_ids)):
            a, b = int(self.pdf_offsets[p]), int(self.pdf_offsets[p + 1])
            self.gconsts[a:b] += lf


# kalpy PitchComputer option → (key of meta.json's "features", the reference's default)
_PITCH_META = {"frame_shift": ("frame_shift", 10), "frame_length": ("frame_length", 25), "min_f0": ("min_f0", 50),
               "max_f0": ("max_f0", 800), "sample_frequency": ("sample_frequency", 16000), "penalty_factor": ("penalty_factor", 0.1),
               "delta_pitch": ("delta_pitch", 0.005), "snip_edges": ("snip_edges", True)}


def pitch_options(meta: dict) -> dict:
    """kalpy PitchComputer options of an acoustic model's ``meta.json`` (a dict with a ``features`` entry) — the mapping of
    the reference's AcousticModel.pitch_options (MFA/models.py:551-576): ``use_pitch`` adds the normalised log-pitch, or the
    raw one when ``normalize_pitch`` is off; ``use_voicing`` adds the POV feature; ``use_delta_pitch`` the delta-pitch."""
    feats = meta.get("features", {})
    pitch, normalize = bool(feats.get("use_pitch", False)), feats.get("normalize_pitch", True)
    options = {name: feats.get(key, default) for name, (key, default) in _PITCH_META.items()}
    options.update(add_pov_feature=feats.get("use_voicing", False), add_normalized_log_pitch=normalize if pitch else False,
                   add_delta_pitch=feats.get("use_delta_pitch", False))
    if pitch:                       # (the reference names this flag only for a use_pitch model)
        options["add_raw_log_pitch"] = not normalize
    return options


def pdfs_of_phones(tm: TransitionModel, phones: Iterable[int]) -> List[int]:
    """Kaldi ``GetPdfsForPhones``: every pdf reachable from the given phone ids."""
    ph = set(int(p) for p in phones)
    out = set()
    for row in tm.tuples:
        if int(row[0]) in ph:
            out.add(int(row[2]))
            out.add(int(row[3]))
    return sorted(out)


def load_model_bytes(data: bytes):
    raw_tm, raw_am = kaldi_io.read_model(data)
    return TransitionModel(raw_tm), DiagGmmModel.from_raw(raw_am)
