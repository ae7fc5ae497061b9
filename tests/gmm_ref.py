"""Acoustic scoring off the tuned shapes: a model generator shaped like a trained model, the float64 reference, a derived
per-cell error bound, and the cases the GPU tests of tests/test_gpu_gmm_shapes.py run (tests/test_gmm_ref_cpu.py checks the
bound on every one of them against the C++ oracle, without a GPU).

The bound.  A score is LL(t, j) = log Σ_g exp(ll_g), ll_g = gconst_g + Σ_k w_gk · x̃_tk over the 2·dim operand columns
(w = [means·inv_vars, −½ inv_vars], x̃ = [x, x²]).  With M(t, j) = max_g (|gconst_g| + Σ_k |w_gk · x̃_tk|), formed in float64,

    B(t, j) = (3·2⁻²² + (2·dim + 1)·2⁻²⁴) · M(t, j) + G_j·2⁻²³ + 2⁻²⁰ + spacing(float32(ref))

  3·2⁻²²            the per-term worst case include/mfa_hip.h documents for the f16×2 operand split (bf16×3 is finer, the
                    float32 pipe exact);
  (2·dim + 1)·2⁻²⁴  float32 accumulation of 2·dim + 1 addends in any order;
  G·2⁻²³            rounding of a sum of G exponentials, each at most 1 (the sum is at least 1, and log is 1-Lipschitz
                    there), together with the components Kaldi's cutoff drops: each is below ε = 2⁻²³ relative;
  2⁻²⁰              the hardware exp2 and log2 (csrc/gmm_common.hpp puts `finish` at ≲ 4e-7);
  spacing           the final rounding of the score to float32.
The log-sum-exp itself is 1-Lipschitz in the max norm, so a per-Gaussian error of at most e moves the score by at most e.
Nothing here is measured on the code under test."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List

import numpy as np

from montreal_forced_aligner_amd import model as M
from oracle import np_oracle as NP
from tests import helpers


@dataclass
class SkewedGmm:
    am: M.DiagGmmModel
    means: np.ndarray      # [G, dim] float64
    devs: np.ndarray       # [G, dim] float64
    weights: np.ndarray    # [G] float64
    forced: np.ndarray     # [G] bool: the components whose weight was forced to 1e-12
    dup: np.ndarray        # [n, 2] Gaussian indices of the exactly duplicated pairs


def skewed_gmm(rng, dim, sizes) -> SkewedGmm:
    """A seeded diagonal GMM with the spread of a trained one: every column has its own scale (standard deviation
    log-uniform in [1e-2, 1e2]) and an offset of several deviations; every Gaussian's deviation is that scale jittered by a
    factor in [0.5, 2]; mixture weights are Dirichlet(0.1) (floored at 1e-30: float64 Dirichlet draws underflow to 0); a pdf
    of 3 or more Gaussians has one weight forced to 1e-12 (under Kaldi's ln ε cutoff wherever it is not the closest
    component), a pdf of 4 or more has one exactly duplicated component (a tie in the maximum)."""
    col_dev = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=dim))
    col_mean = rng.normal(0.0, 4.0, size=dim) * col_dev
    gconsts, mi, iv, offs = [], [], [], [0]
    means, devs, weights, forced, dup = [], [], [], [], []
    for g in sizes:
        w = rng.dirichlet(np.full(g, 0.1)) if g > 1 else np.ones(1)
        w = np.maximum(w, 1e-30)
        w /= w.sum()
        mean = col_mean[None, :] + rng.normal(0.0, 2.0, size=(g, dim)) * col_dev[None, :]
        dev = col_dev[None, :] * np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=(g, dim)))
        f = np.zeros(g, bool)
        if g >= 4:
            mean[g - 1], dev[g - 1], w[g - 1] = mean[g - 2], dev[g - 2], w[g - 2]
            dup.append((offs[-1] + g - 2, offs[-1] + g - 1))
        if g >= 3:
            w[0] = 1e-12
            f[0] = True
        var = dev * dev
        inv = 1.0 / var
        gc = np.log(w) - 0.5 * (dim * np.log(2 * np.pi) + np.log(var).sum(axis=1) + (mean * mean * inv).sum(axis=1))
        gconsts.append(gc.astype(np.float32)); mi.append((mean * inv).astype(np.float32)); iv.append(inv.astype(np.float32))
        means.append(mean); devs.append(dev); weights.append(w); forced.append(f)
        offs.append(offs[-1] + g)
    am = M.DiagGmmModel(dim, np.concatenate(gconsts), np.concatenate(mi), np.concatenate(iv), np.asarray(offs, np.int32))
    return SkewedGmm(am, np.concatenate(means), np.concatenate(devs), np.concatenate(weights), np.concatenate(forced),
                     np.asarray(dup, np.int64).reshape(-1, 2))


def sample_frames(rng, sk: SkewedGmm, n_frames) -> np.ndarray:
    """Frames drawn from the model's own Gaussians (a component picked uniformly, then N(mean, dev²)); about 5 % of them carry
    one coordinate 8 deviations off its mean."""
    g = rng.integers(0, sk.means.shape[0], size=n_frames)
    x = sk.means[g] + sk.devs[g] * rng.normal(size=(n_frames, sk.means.shape[1]))
    far = np.flatnonzero(rng.random(n_frames) < 0.05)
    k = rng.integers(0, sk.means.shape[1], size=far.size)
    x[far, k] = sk.means[g[far], k] + 8.0 * sk.devs[g[far], k] * rng.choice([-1.0, 1.0], size=far.size)
    return x.astype(np.float32)


def ref64(feats, am, pdf_list) -> np.ndarray:
    """float64 log-likelihoods [T, len(pdf_list)], plain log-sum-exp without the cutoff (oracle.np_oracle.gmm_loglikes)."""
    return NP.gmm_loglikes(feats, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pdf_list)


def bound(feats, am, pdf_list, ref) -> np.ndarray:
    """B(t, j) of the module docstring for every cell of ``ref`` = ref64(feats, am, pdf_list)."""
    x = np.asarray(feats, np.float64)
    dim = am.dim
    mag = np.abs(am.gconsts.astype(np.float64))[None, :] + np.abs(x) @ np.abs(am.means_invvars.astype(np.float64)).T \
        + 0.5 * (x * x) @ np.abs(am.inv_vars.astype(np.float64)).T
    out = np.zeros((x.shape[0], len(pdf_list)))
    per_term = 3.0 * 2.0 ** -22 + (2 * dim + 1) * 2.0 ** -24
    for j, p in enumerate(pdf_list):
        a, b = int(am.pdf_offsets[p]), int(am.pdf_offsets[p + 1])
        out[:, j] = per_term * mag[:, a:b].max(axis=1) + (b - a) * 2.0 ** -23 + 2.0 ** -20
    return out + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def f32_rule(orc) -> float:
    """The project's bound on the float32 kernels' mixture scores against the C++ oracle (test_gmm_real_mixture_model): four
    float32 spacings of the utterance's largest score."""
    return 4.0 * float(np.spacing(np.float32(np.abs(orc).max())))


# ---- the cases of tests/test_gpu_gmm_shapes.py: (generator, dim, sizes, seed) → model, utterances, pdf lists

@dataclass
class Case:
    name: str
    am: M.DiagGmmModel
    feats: List[np.ndarray]
    lists: List[np.ndarray]
    skewed: bool = False
    sk: SkewedGmm = None


SIZES_EDGE = [1, 1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 70]
FRAMES_EDGE = (1, 63, 64, 65, 257)
DIMS_EDGE = (3, 8, 13, 16, 24, 36, 41, 47, 48)
DIMS_PLAIN = (49, 52, 64)
DIMS_NAIVE = (39, 45)
SIZES_SKEWED = [1, 2, 4, 5, 8, 12, 16, 17, 32, 33, 70, 128]
FRAMES_SKEWED = (65, 300)
DIMS_SKEWED = (39, 40, 45)
SIZES_HUGE = [1025, 1500, 33, 32, 1]
SIZES_REPEATS = [1, 4, 17, 40, 2]
REPEAT_DIMS = (52, 39)
SIZES_RANGE = [32] * 6 + [17, 20, 31, 29] + [1, 4, 8, 16] + [33, 70]
N_MANY, MANY_ALONE = 700, 20


def _lists(rng, n_pdfs, counts):
    return [rng.permutation(n_pdfs)[:n].astype(np.int32) for n in counts]


@lru_cache(maxsize=None)
def edge_case(dim) -> Case:
    """a / b: random_gmm at narrow, edge and wide dimensions; frame counts around the 64-frame tile and past one 256-frame item."""
    rng = np.random.default_rng(7000 + dim)
    am = helpers.random_gmm(rng, dim, SIZES_EDGE)
    feats = [rng.normal(0, 3, size=(t, dim)).astype(np.float32) for t in FRAMES_EDGE]
    return Case(f"random dim {dim}", am, feats, _lists(rng, am.num_pdfs, (12, 12, 5, 1, 9)))


@lru_cache(maxsize=None)
def repeats_case(dim) -> Case:
    """c: 5 pdfs, the longest utterance carries a 12-entry list with repeats — T_u · P_u > max_frames · num_pdfs."""
    rng = np.random.default_rng(7100 + dim)
    am = helpers.random_gmm(rng, dim, SIZES_REPEATS)
    feats = [rng.normal(0, 3, size=(t, dim)).astype(np.float32) for t in (20, 70, 33)]
    lists = [np.array([3, 0, 4], np.int32), np.array([0, 1, 2, 3, 4, 2, 2, 0, 3, 1, 4, 3], np.int32),
             np.array([4, 3, 2, 1, 0], np.int32)]
    return Case(f"repeats dim {dim}", am, feats, lists)


@lru_cache(maxsize=None)
def skewed_case(dim) -> Case:
    """e: a skewed model, frames from its own Gaussians."""
    rng = np.random.default_rng(7200 + dim)
    sk = skewed_gmm(rng, dim, SIZES_SKEWED)
    feats = [sample_frames(rng, sk, t) for t in FRAMES_SKEWED]
    return Case(f"skewed dim {dim}", sk.am, feats, _lists(rng, sk.am.num_pdfs, (12, 12)), True, sk)


@lru_cache(maxsize=None)
def huge_case() -> Case:
    """f: pdfs of more than 1 024 Gaussians (more than 32 blocks: the block count no longer fits the column's row word)."""
    rng = np.random.default_rng(7300)
    am = helpers.random_gmm(rng, 39, SIZES_HUGE)
    feats = [rng.normal(0, 3, size=(t, 39)).astype(np.float32) for t in (65, 130)]
    return Case("huge pdfs dim 39", am, feats, [np.arange(5, dtype=np.int32), np.array([1, 4, 0], np.int32)])


@lru_cache(maxsize=None)
def range_case() -> Case:
    """g: a 700-frame utterance (three 256-frame items) and a short one; the tests move one value of frame 300."""
    rng = np.random.default_rng(7400)
    am = helpers.random_gmm(rng, 40, SIZES_RANGE)
    feats = [rng.normal(0, 3, size=(t, 40)).astype(np.float32) for t in (700, 65)]
    return Case("f16 range dim 40", am, feats, [np.arange(am.num_pdfs, dtype=np.int32), _lists(rng, am.num_pdfs, (7,))[0]])


# g: (name, operand column k, scaled target, tile declined by the f16 pass) — one plain column and one squared column, each
# just under and just over the f16 pass's decline threshold of 65 000.  A plain column cannot be the first to get there: the
# packer balances operand k and weight column k at 2^13 each for the model's reach |μ| + 10σ (S·wmax_k·xmax_k ≤ 2^26), so
# a plain operand at 65 000 is a feature ≥ 7.9 reaches out, its square ≥ 63 reaches, and the squared column's scale is
# never below the plain one's by that much (wmax_k / (wmax_{dim+k}·reach) ≤ 2: both maxima carry the same inv_var).
# Those two variants therefore pin that the tile IS declined on either side of the plain operand's own threshold;
# test_gmm_ref_cpu.py evaluates the kernels' range test on the host to confirm each expectation.
RANGE_VARIANTS = [("plain under", 3, 64990.0, True), ("plain over", 3, 65010.0, True), ("square under", 40 + 5, 64990.0, False),
                  ("square over", 40 + 5, 65010.0, True)]


def range_feats(case: Case, fscale, k, target) -> List[np.ndarray]:
    """The case's features with frame 300 of the long utterance set so that operand column k, scaled, comes to ``target``."""
    dim = case.am.dim
    feats = [f.copy() for f in case.feats]
    v = target / float(fscale[k])
    feats[0][300, k % dim] = np.float32(v if k < dim else np.sqrt(v))
    return feats


@lru_cache(maxsize=None)
def many_case() -> Case:
    """h: 700 short utterances — more (utterance, tile) items than a launch has workgroups."""
    rng = np.random.default_rng(7500)
    am = helpers.random_gmm(rng, 39, [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 70, 1])
    T = rng.integers(1, 41, size=N_MANY)
    feats = [rng.normal(0, 3, size=(int(t), 39)).astype(np.float32) for t in T]
    lists = [rng.choice(am.num_pdfs, size=int(rng.integers(1, 7)), replace=False).astype(np.int32) for _ in range(N_MANY)]
    return Case("many utterances dim 39", am, feats, lists)


def wide_models(num_pdfs):
    """d: dim-52 models over a transition model's pdfs — single Gaussians, then mixtures."""
    rng = np.random.default_rng(7600)
    single = helpers.random_gmm(rng, 52, [1] * num_pdfs)
    sizes = [int(x) for x in rng.choice([1, 2, 4, 5, 9, 17, 33], size=num_pdfs)]
    return single, helpers.random_gmm(rng, 52, sizes)


def sorted_lists(am, lists):
    """numpy copy of mfa_gmm_sort_pdf_list's order (classes {17–32, > 32, 9–16, 5–8, 2–4, 1 Gaussians}, stable), so that the
    CPU check scores the columns the GPU tests score."""
    g = np.diff(am.pdf_offsets)
    cls = np.array([0 if 16 < x <= 32 else 1 if x > 32 else 2 if x > 8 else 3 if x > 4 else 4 if x > 1 else 5 for x in g])
    return [np.asarray(l, np.int32)[np.argsort(cls[l], kind="stable")] for l in lists]


def all_cases() -> List[Case]:
    """Every (generator, dim, sizes, seed) the GPU tests use but the two that need fixtures (d: wide_models; g: the moved
    frames), for the CPU check of the bound."""
    cases = [edge_case(d) for d in DIMS_EDGE + DIMS_PLAIN + DIMS_NAIVE]
    cases += [repeats_case(d) for d in REPEAT_DIMS] + [skewed_case(d) for d in DIMS_SKEWED]
    cases += [huge_case(), range_case(), many_case()]
    return cases
