"""The PLDA scoring formula in its direct form and the transform, restated in ``numpy.longdouble`` (64-bit significand on
x86: 2⁻⁶⁴ against float64's 2⁻⁵³), with the cases and the error bound that tests/test_plda_cpu.py and tests/test_gpu_plda.py
share.  Nothing here imports the package: the inputs are plain arrays.

The bound.  The device (and its host twin) computes  score_ij = c_j + Σ_k (p_ik·p_ik)·A_jk + Σ_k p_ik·B_jk  in float64.
With u = 2⁻⁵³ and γ_m = m·u / (1 − m·u), counting roundings (include/mfa_hip.h "PLDA", csrc/plda_math.hpp):

  prepare   a = nψ/(nψ+1): 3;  v = 1 + ψ/(nψ+1): 4 (sums of positive numbers keep the relative error);
            A = −½·ψa/(v(1+ψ)): ψa 4, 1+ψ 1, v(1+ψ) 6, the quotient 11;  B = (a g)/v: a g 4, the quotient 9
  products  p·p: 1, (p p)·A: 1 more → 13 on a term p²A;  p·B: 1 → 10 on a term pB
  sum       the accumulator starts from c_j and takes 2·Dpad ≤ 2(D + 3) additions → every term, c_j included, carries at
            most 2(D + 3) more, whatever the order inside one matrix instruction is
  c_j       = ½(Σ_k log1p(ψa/v) − Σ_k (a g)²/v): a term log1p(ψa/v) carries 9 (its argument; the function's condition
            number is at most 1) + 8 (an implementation within 4 ulp) = 17, a term (a g)²/v 14; D − 1 additions; the
            difference 1 → γ_(D+18) relative to  cmag_j = ½(Σ log1p + Σ (a g)²/v),  not to |c_j|: the two sums may cancel.
            The issue's bracket |c_j| + Σ|p²A| + Σ|pB| covers cmag_j only through its other two terms: termwise
            ½·log1p(ψa/v) ≤ ½·ψa/v = p²|A|·(1 + ψ)/p² and ½·(a g)²/v = |pB|·a|g|/(2|p|), so a test element far enough from 0
            covers both.  ``random_case`` therefore keeps every test element at least ¾ of its standard deviation from 0
            (p² ≥ 0.5625 (1 + ψ): the first ratio is below 1.78; the second exceeds 4 only for a train element past 6
            deviations), and ``check_case`` asserts  cmag_j ≤ 4·(|c_j| + Σ|p²A| + Σ|pB|)  for every pair from the inputs
            alone, on the CPU — which turns c_j's error into 4(D + 18) roundings on the bracket.  (A test vector at 0
            against a column whose two sums cancel has no bound of this form in float64: c_j itself is ill-conditioned
            there.  Zeros are the exact tier's business.)

  m = 4(D + 18) + 13 + 2(D + 3) + 1 = 6 D + 92,   |err_ij| ≤ γ_m · (|c_j| + Σ_k |p_ik² A_jk| + Σ_k |p_ik B_jk|),

the bracket evaluated in longdouble from the inputs.  Nothing in it comes from the output under test.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


def bound_m(D: int) -> int:
    return 6 * D + 92


def llr(psi, train, n, test):
    """[test, train] log-likelihood ratios, the direct form (the specification), longdouble."""
    psi, train, test = LD(np.asarray(psi))[None, :], LD(np.asarray(train)), LD(np.asarray(test))
    n = LD(np.broadcast_to(np.asarray(n, dtype=np.float64), (train.shape[0],)))[:, None]
    mean = n * psi / (n * psi + 1) * train                       # [Ns, D]
    var = 1 + psi / (n * psi + 1)
    D = train.shape[1]
    log2pi = LD("1.8378770664093454835606594728112353")
    out = np.empty((test.shape[0], train.shape[0]), dtype=LD)
    for i in range(test.shape[0]):
        t = test[i][None, :]
        given = -(np.log(var).sum(axis=1) + D * log2pi + ((t - mean) ** 2 / var).sum(axis=1)) / 2
        without = -(np.log(1 + psi).sum() + D * log2pi + (t ** 2 / (1 + psi)).sum()) / 2
        out[i] = given - without
    return out


def bracket(psi, train, n, test):
    """(|c_j| + Σ|p²A| + Σ|pB| as [test, train], cmag [train]) in longdouble, from the inputs."""
    psi, train, test = LD(np.asarray(psi))[None, :], LD(np.asarray(train)), LD(np.asarray(test))
    n = LD(np.broadcast_to(np.asarray(n, dtype=np.float64), (train.shape[0],)))[:, None]
    a = n * psi / (n * psi + 1)
    v = 1 + psi / (n * psi + 1)
    A = -(1 / v - 1 / (1 + psi)) / 2
    B = a * train / v
    logr, quad = (np.log(1 + psi) - np.log(v)).sum(axis=1), ((a * train) ** 2 / v).sum(axis=1)
    c = (logr - quad) / 2
    br = np.abs(c)[None, :] + (test ** 2) @ np.abs(A).T + np.abs(test) @ np.abs(B).T
    return br, (logr + quad) / 2


def error_bound(psi, train, n, test):
    """[test, train] float64: γ_m times the bracket."""
    br, _ = bracket(psi, train, n, test)
    return np.asarray(br * gamma(bound_m(np.shape(train)[1])), dtype=np.float64)


def direct_form_error(psi, train, n, test):
    """[test, train] float64: what the direct form evaluated in float64 (``PldaModel.log_likelihood_ratio``: numpy, plain
    sums) may itself be off by — every term of its two brackets carries at most 8 roundings (mean 4, var 4 or 1 + ψ 1, the
    difference, the square, the quotient, log within an ulp) and the sums D + 2 additions, D·log 2π included on both sides:
    γ_(D+10)·½(Σ|log var| + Σ log(1+ψ) + 2 D log 2π + Σ (t − m)²/var + Σ t²/(1+ψ))."""
    psi, train, test = LD(np.asarray(psi))[None, :], LD(np.asarray(train)), LD(np.asarray(test))
    n = LD(np.broadcast_to(np.asarray(n, dtype=np.float64), (train.shape[0],)))[:, None]
    mean, var = n * psi / (n * psi + 1) * train, 1 + psi / (n * psi + 1)
    D = train.shape[1]
    fixed = np.abs(np.log(var)).sum(axis=1)[None, :] + np.log(1 + psi).sum() + 2 * D * LD("1.8378770664093454835606594728112353")
    quad = np.stack([((t[None, :] - mean) ** 2 / var).sum(axis=1) for t in test]) + (test ** 2 / (1 + psi)).sum(axis=1)[:, None]
    return np.asarray(gamma(D + 10) * (fixed + quad) / 2, dtype=np.float64)


def check_case(psi, train, n, test) -> None:
    """The premise of the bound's treatment of c_j, from the inputs alone."""
    br, cmag = bracket(psi, train, n, test)
    assert (cmag[None, :] <= 4 * br).all(), float((cmag[None, :] / br).max())


def transform(mean, T, psi, x, num_examples, norm):
    """The transform with its length normalisation in longdouble: norm 0 none, 1 simple, 2 the model's."""
    mean, T, psi, x = LD(np.asarray(mean)), LD(np.asarray(T)), LD(np.asarray(psi)), LD(np.atleast_2d(x))
    u = x @ T.T - (T @ mean)[None, :]
    if norm == 0:
        return u
    D = x.shape[1]
    if norm == 1:
        s = (u * u).sum(axis=1, keepdims=True)
    else:
        n = LD(np.broadcast_to(np.asarray(num_examples, dtype=np.float64), (x.shape[0],)))[:, None]
        s = (u * u / (psi[None, :] + 1 / n)).sum(axis=1, keepdims=True)
    return u * np.sqrt(D / s)


# ---- cases -----------------------------------------------------------------------------------------------------------------
TRAIN_N = (1, 2, 7, 1000)


def random_case(D: int, nt: int, ns: int, seed: int):
    """psi [D] descending in [0.05, 8]; train vectors as means of n examples of their class (variance ψ + 1/n), test vectors as
    single examples (deviation √(ψ + 1)) with every element pushed ¾ of a deviation away from 0 (the module docstring says why).
    train_n cycles through {1, 2, 7, 1000}."""
    rng = np.random.default_rng(seed)
    psi = np.sort(np.exp(rng.uniform(np.log(0.05), np.log(8.0), D)))[::-1].copy()
    n = np.array([TRAIN_N[(j + seed) % 4] for j in range(ns)], dtype=np.int32)
    train = rng.standard_normal((ns, D)) * np.sqrt(psi[None, :] + 1.0 / n[:, None])
    z = rng.standard_normal((nt, D))
    test = np.where(z < 0, -1.0, 1.0) * (0.75 + np.abs(z)) * np.sqrt(psi[None, :] + 1.0)
    return psi, train, n, test


def exact_case(D: int, nt: int, ns: int, seed: int):
    """Operands for the sweep's debug entry on which every product and sum is exact in float64: p small integers, A and B
    multiples of 1/4, c multiples of 1/8; few distinct values, so equal scores are common (the tie rule).  Sums stay below
    2^20 with at most 5 fractional bits."""
    rng = np.random.default_rng(seed)
    test = rng.integers(-3, 4, (nt, D)).astype(np.float64)
    A = -rng.integers(0, 3, (ns, D)).astype(np.float64) / 4
    B = rng.integers(-2, 3, (ns, D)).astype(np.float64) / 4
    c = rng.integers(-8, 9, ns).astype(np.float64) / 8
    if ns > 2:                                           # two identical columns: a tie in every row
        A[ns - 1], B[ns - 1], c[ns - 1] = A[0], B[0], c[0]
    return test, A, B, c


def exact_scores(test, A, B, c):
    """The exact tier's matrix in longdouble (exact there too)."""
    return LD(c)[None, :] + (LD(test) ** 2) @ LD(A).T + LD(test) @ LD(B).T


def stable_topk(scores, k: int, exclude_diagonal: bool = False):
    """(indices [rows, k], scores [rows, k]) of the finite entries, larger first, ties to the lower index; −1 / −inf padding."""
    s = np.array(scores, dtype=np.float64)
    nt, ns = s.shape
    idx, val = np.full((nt, k), -1, dtype=np.int32), np.full((nt, k), -np.inf)
    for i in range(nt):
        row = s[i].copy()
        ok = np.isfinite(row)
        if exclude_diagonal and i < ns:
            ok[i] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(-row[cand], kind="stable")][:k]
        idx[i, : order.size], val[i, : order.size] = order, row[order]
    return idx, val


def clear_rows(ref, bound, k: int, exclude_diagonal: bool = False):
    """(rows whose first min(k, candidates) ranks in the restatement ``ref`` are separated from one another and from the next
    rank by more than twice the row's largest bound, the restatement's order [rows, columns], the ranks compared).  Only on
    those rows can indices be compared with the restatement's."""
    masked = np.array(ref, dtype=np.float64)
    nt, ns = masked.shape
    if exclude_diagonal:
        d = np.arange(min(nt, ns))
        masked[d, d] = -np.inf
    order = np.argsort(-masked, axis=1, kind="stable")
    srt = np.take_along_axis(masked, order, axis=1)
    kk = min(k, ns - (1 if exclude_diagonal else 0))
    clear = np.ones(nt, bool)
    if kk < 1:
        return clear, order, 0
    rowb = np.asarray(bound).max(axis=1)
    if srt.shape[1] > kk:
        clear &= (srt[:, kk - 1] - srt[:, kk]) > 2 * rowb
    if kk > 1:
        clear &= (srt[:, : kk - 1] - srt[:, 1: kk]).min(axis=1) > 2 * rowb
    return clear, order, kk
