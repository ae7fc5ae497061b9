"""What bench.py reports about a ``Pipeline``: the work one step does in flops and bytes, and a roofline per stage —
``PipelineReport``, methods of ``Pipeline``.

Uses of the pipeline: ``e`` (the engine: ``device``, ``gmm``), ``step``, the shape fields (``frame_off``, ``ll_off``, ``n_utt``,
``num_ceps``, ``feat_dim``), ``pcm``, ``graphs``, ``loglikes``, ``lazy`` / ``window`` / ``reachability``, ``gmm_flops``; it owns
``cells_scored``, ``cells_scored_fraction``, ``scored_flops`` and ``_states_times_frames``.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch


def _split_passes(mono: bool, gauss_per_pdf: int) -> Tuple[bool, bool]:
    """(split-operand scoring at all, its f16x2 pass) for a model, as MFA_GMM_BF16 / MFA_GMM_F16 say right now (tests and the
    benchmark flip them inside one process, so nothing is cached)."""
    split = os.environ.get("MFA_GMM_BF16", "1") != "0" and not mono and gauss_per_pdf != 1
    return split, split and os.environ.get("MFA_GMM_F16", "1") != "0"


class PipelineReport:
    _states_times_frames: Optional[float] = None
    # measure_scored_cells (bench.py hands one pipeline's figures to the others of the same shape)
    cells_scored = cells_scored_fraction = scored_flops = None

    def scores_string(self) -> str:
        if self.lazy:
            return (f"lazy: per {self.window}-frame window, only the pdfs arcs within {self.window} arcs of the live tokens "
                    "can emit (a superset of what Kaldi's lazy decodable evaluates)")
        return "reachable cells only (pdf j from its first possible frame on)" if self.reachability else "dense T x P"

    def dtype_string(self, mono: bool, gauss_per_pdf: int) -> str:
        split, f16 = _split_passes(mono, gauss_per_pdf)
        if f16:
            return "f32 scores from 2-way f16-split products (3*2^-22 per term worst case), f64 path costs"
        if split:
            return "f32 scores from 3-way bf16-split products (2^-24 per term), f64 path costs"
        return "f32 (scores), f64 (path costs)"

    def algorithmic_bytes(self, score_cells_read: Optional[float] = None) -> Dict[str, float]:
        """SURVEY §8(d) staged-pipeline bytes of one step, per stage (each tensor written once and read once).  The score
        matrix counts for what is actually moved: the scoring stage writes the cells it computes, the decoder reads
        ``score_cells_read`` cells (counted by the oracle's lazy decodable on a sample — the device decoder asks for exactly
        the same cells) or, without that count, at most the cells written."""
        T = np.diff(self.frame_off).astype(np.float64)
        P = np.diff(self.graphs.pdf_off_host).astype(np.float64)
        n_samples = float(self.pcm.numel())
        A = float(self.graphs.total_arcs)
        S = float(self.graphs.tensors["final"].numel())
        D = float(self.feat_dim)
        tot = float(T.sum())
        written = self.cells_scored if self.lazy else None
        if written is None:
            written = float((P * T).sum())
        if score_cells_read is not None:
            read, how = float(score_cells_read), "4 B x cells the decoder read (oracle's lazy-decodable count on the CPU sample, scaled to the batch)"
        else:
            read, how = written, "4 B x cells the scoring stage wrote (upper bound of the cells the decoder read)"
        if self._states_times_frames is None:
            self._states_times_frames = float((T * np.diff(self.graphs.tensors["state_off"].cpu().numpy())).sum())
        return {
            "mfcc": 2.0 * n_samples + 4.0 * self.num_ceps * tot,
            "feats": 4.0 * self.num_ceps * tot + 4.0 * D * tot,
            "gmm": 4.0 * D * tot + 4.0 * written,                  # model slice cache-resident (SURVEY's 6.0 MB variant)
            "viterbi": 4.0 * read + 16.0 * A + 2.0 * self._states_times_frames + 6.0 * tot,
            "viterbi_score_bytes_how": how,
            "states": S,
        }

    def measure_scored_cells(self) -> Dict[str, float]:
        """One step on a zero-filled score scratch: which cells did the scoring kernels write?  Returns the count, the
        fraction of the T x P matrix, and the flops those cells cost (4*D*g per cell, g = Gaussians of the cell's pdf) —
        the work the scoring stage EXECUTES, which is what bench.py's roofline prices."""
        self.loglikes.zero_()
        self.step()
        torch.cuda.synchronize(self.e.device)
        g_of_pdf = torch.from_numpy(np.diff(self.e.gmm.pdf_offsets).astype(np.float64)).to(self.e.device)
        pdf_list = self.graphs.pdf_list.long()
        T = np.diff(self.frame_off)
        cells = torch.zeros((), dtype=torch.float64, device=self.e.device)
        weighted = torch.zeros((), dtype=torch.float64, device=self.e.device)
        po = self.graphs.pdf_off_host
        for u in range(self.n_utt):
            a, b = int(self.ll_off[u]), int(self.ll_off[u + 1])
            if b == a:
                continue
            per_col = (self.loglikes[a:b].view(int(T[u]), -1) != 0).sum(dim=0).to(torch.float64)
            cells += per_col.sum()
            weighted += (per_col * g_of_pdf[pdf_list[int(po[u]): int(po[u + 1])]]).sum()
        self.cells_scored = float(cells.item())
        self.cells_scored_fraction = self.cells_scored / max(1, self.loglikes.numel())
        self.scored_flops = 4.0 * self.e.gmm.dim * float(weighted.item())
        return {"cells": self.cells_scored, "fraction": self.cells_scored_fraction, "flops": self.scored_flops}

    def roofline(self, dominant: str, ktimes: Dict[str, Dict[str, float]], steps: int, mono: bool, gauss_per_pdf: int,
                 score_cells_read: Optional[float] = None) -> Dict:
        """Roofline object for a stage of the step (bench.py): per-step stage time from the HIP-event timers.  Everything
        priced here is work the kernels EXECUTE: scoring = the cells the lazy path wrote (``measure_scored_cells``), the
        decoder's score bytes = the cells it read (``score_cells_read`` when the oracle counted them on a sample, else the
        cells written — an upper bound)."""
        ms = ktimes[dominant]["ms"] / max(1, steps)
        launches = ktimes[dominant]["launches"] / max(1, steps)
        lazy_measured = self.lazy and self.scored_flops is not None
        if dominant == "gmm":
            split, f16 = _split_passes(mono, gauss_per_pdf)
            mult = 3.0 if f16 else (6.0 if split else 1.0)
            peak = 2500.0 if split else 157.3
            flops = self.scored_flops if lazy_measured else self.gmm_flops
            ach = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            equiv = self.gmm_flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            return {"kernel": "diagonal-GMM scoring (" + ("f16x2" if f16 else "bf16x3" if split else "f32") + " MFMA)",
                    "kernel_key": "gmm", "bound": "mfma", "achieved": round(ach, 3), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(ach / peak, 4), "traffic": None,
                    "executed_flops_per_step": flops, "mfma_flops_per_algorithmic_flop": int(mult),
                    "executed_mfma_tflops": round(mult * ach, 3), "executed_mfma_frac_of_peak": round(mult * ach / peak, 4),
                    "cells_scored_fraction": self.cells_scored_fraction,
                    "algorithmic_equivalent_tflops": round(equiv, 3), "ms_per_step": round(ms, 4), "launches_per_step": launches,
                    "note": "achieved = 4*D*g flops of the (frame, pdf) cells the scoring kernels actually computed / stage time; "
                            "executed_mfma_* = the same times the split-operand products per term; algorithmic_equivalent_tflops "
                            "prices every cell of the reachability-bounded matrix (what a dense scorer would do) and is NOT work done"}
        by = self.algorithmic_bytes(score_cells_read)
        b = by.get(dominant, 0.0)
        gbs = b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        names = {"viterbi": "viterbi kernels (beam Viterbi, one wavefront per utterance)", "mfcc": "mfcc_kernel",
                 "feats": "feats_rows_kernel / feats_kernel", "cmvn": "cmvn kernels"}
        out = {"kernel": names.get(dominant, dominant), "kernel_key": dominant, "bound": "hbm", "achieved": round(gbs, 2),
               "peak": 8000.0, "unit": "GB/s", "frac": round(gbs / 8000.0, 5), "traffic": None,
               "algorithmic_bytes_per_step": b, "ms_per_step": round(ms, 4), "launches_per_step": launches,
               "note": "algorithmic bytes = SURVEY 8(d) staged-pipeline bytes of this stage (each tensor written once, read once)"}
        if dominant == "viterbi":
            out["score_bytes"] = by["viterbi_score_bytes_how"]
        return out
