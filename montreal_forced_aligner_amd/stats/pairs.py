"""Statistics over pairs of vectors: the PLDA transform, the sweep of every test vector over every train vector for any metric
and its consumers (scores, best, k-NN, neighbour bits), DBSCAN on the bits, HDBSCAN's pair form, core scores and spanning
tree, and the silhouette coefficients; device call and host twin each.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib
from .._lib import twin_call
from ._common import device_model


# ---- PLDA: the transform, the score matrix and its row-wise consumers (include/mfa_hip.h "PLDA") ---------------------------------
_PLDA_TWIN_CODES = {-2: "dimension outside [1, 1024]", -3: "list length outside [1, 64]", -4: "a psi entry that is not positive and finite",
                    -5: "2^31 vectors or more", -6: "a number of examples below 1", -7: "every output is off"}
PLDA_BLOCK_BYTES = 256 << 20        # device bytes of one row block of ``plda_scores``
PLDA_MATRIX_BYTES = 4 << 30         # the largest full matrix ``plda_scores`` hands out


def _plda_arrays(model):
    return tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (model.transform, model.offset, model.psi))


def _plda_device_model(engine, model):
    """A ``plda.PldaModel`` as the device tensors (transform, offset, psi)."""
    return device_model(engine, model, lambda: _plda_arrays(model))


def _device_f64(engine, x) -> torch.Tensor:
    """A numpy array or a tensor as a contiguous float64 tensor on the device."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return t.to(device=engine.device, dtype=torch.float64).contiguous()


def _plda_vectors(engine, x, D: int, what: str) -> torch.Tensor:
    """Rows of float64 [n, D] on the device, from a numpy array or a tensor."""
    t = x if isinstance(x, torch.Tensor) else np.atleast_2d(x)
    if t.ndim != 2 or (t.shape[0] and t.shape[1] != D):
        raise _lib.MfaHipError(f"{what}: vectors {tuple(t.shape)} for a model of dimension {D}")
    return _device_f64(engine, t)


def _plda_counts(engine, n, rows: int, what: str):
    if n is None:
        return None
    t = n if isinstance(n, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32))
    if tuple(t.shape) != (rows,):
        raise _lib.MfaHipError(f"{what}: one number of examples per vector ({tuple(t.shape)} for {rows})")
    return t.to(device=engine.device, dtype=torch.int32).contiguous()


def _plda_norm(normalize_length: bool, simple_length_norm: bool) -> int:
    return 0 if not normalize_length else (1 if simple_length_norm else 2)


def plda_transform(engine, model, x, num_examples=None, normalize_length: bool = True, simple_length_norm: bool = False) -> torch.Tensor:
    """``model.transform_ivector`` of every row of ``x`` ([n, D], numpy or a tensor) on the device (mfa_plda_transform_batch):
    float64 [n, D] on the device, where the scoring calls take it.  ``num_examples``: int32 [n], default 1."""
    x = _plda_vectors(engine, x, model.dim, "plda_transform")
    out = torch.empty_like(x)
    engine._launch_plda_transform(x, _plda_device_model(engine, model), _plda_counts(engine, num_examples, x.shape[0], "plda_transform"),
                                  _plda_norm(normalize_length, simple_length_norm), out)
    return out


def plda_transform_host(model, x, num_examples=None, normalize_length: bool = True, simple_length_norm: bool = False) -> np.ndarray:
    """``plda_transform`` on the host twin (plain loops): numpy in and out."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    if x.shape[0] and x.shape[1] != model.dim:
        raise _lib.MfaHipError(f"plda_transform_host: vectors {x.shape} for a model of dimension {model.dim}")
    n = None if num_examples is None else np.ascontiguousarray(num_examples, dtype=np.int32)
    if n is not None and n.shape != (x.shape[0],):
        raise _lib.MfaHipError("plda_transform_host: one number of examples per vector")
    out = np.empty_like(x)
    twin_call("mfa_debug_plda_transform_host", _PLDA_TWIN_CODES, x, int(x.shape[0]), model.dim, *_plda_arrays(model), n,
              _plda_norm(normalize_length, simple_length_norm), out)
    return out


class _SweepFamily(NamedTuple):
    """The callers of one pair of sweep entry points: their label in messages, the engine's launch, the host twins for train vectors and
    for ready operands, how the twin's message about vectors of the wrong shape ends, and whether the entries take a metric and a
    threshold and write neighbour bits."""
    label: str
    launch: str
    host: str
    host_operands: str
    mismatch: str
    bits: bool


_PLDA_SWEEP = _SweepFamily("PLDA scoring", "_launch_plda_score", "mfa_debug_plda_score_host", "mfa_debug_plda_sweep_host",
                           "for a model of dimension {}", False)
_METRIC_SWEEP = _SweepFamily("neighbour sweep", "_launch_neighbor_bits", "mfa_debug_neighbor_bits_host", "mfa_debug_neighbor_sweep_host",
                             "do not go together", True)


def _device_sweep(engine, family: _SweepFamily, code: int, D: int, unit: bool, test, train, threshold, model, train_n, exclude_diagonal, k,
                  want_scores, want_best, want_knn, want_bits, operands):
    """One sweep on the device through ``family``'s launch: the inputs as float64 device tensors of dimension ``D`` (``unit``: made
    unit length first), the outputs asked for allocated once.  ``code`` is the library's metric; ``model`` and ``train_n`` count for
    0 (plda) alone.  ``operands``: the debug entry's (A, B, c) in place of ``train``.  Returns (scores, best, knn, bits)."""
    dev, label = engine.device, family.label
    test = _plda_vectors(engine, test, D, label)
    if operands is None:
        train = _plda_vectors(engine, train, D, label)
        if unit:
            test, train = _unit_rows(test), _unit_rows(train)
        ns = int(train.shape[0])
        train_n = _plda_counts(engine, train_n, ns, label) if code == 0 else None
        psi = _plda_device_model(engine, model)[2] if code == 0 else None
    else:
        operands = tuple(a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
                         for a in operands)
        train, train_n, psi, ns = None, None, None, int(operands[2].shape[0])
    nt = int(test.shape[0])
    if want_bits and threshold is None:
        raise _lib.MfaHipError(f"{label}: the bits need a threshold")
    scores = torch.empty((nt, ns), dtype=torch.float64, device=dev) if want_scores else None
    best = (torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.float64, device=dev)) if want_best else None
    knn = (torch.empty((nt, k), dtype=torch.int32, device=dev), torch.empty((nt, k), dtype=torch.float64, device=dev)) if want_knn else None
    bits = torch.empty((nt, (ns + 63) // 64), dtype=torch.int64, device=dev) if want_bits else None
    launch = getattr(engine, family.launch)
    if not family.bits:
        launch(test, train, train_n, psi, exclude_diagonal, k, scores, best, knn, operands)
    elif ns == 0 and not (want_scores or want_best or want_knn):
        return None, None, None, bits                  # no train vectors: rows of no words, nothing to ask the library for
    else:
        launch(test, train, code, train_n, psi, exclude_diagonal, int(k), 0.0 if threshold is None else float(threshold), scores, best, knn,
               bits, operands)
    return scores, best, knn, bits


def _host_sweep(family: _SweepFamily, code: int, model_dim: int, unit: bool, test, train, threshold, model, train_n, exclude_diagonal, k,
                want_scores, want_best, want_knn, want_bits, operands):
    """``_device_sweep`` on ``family``'s host twins: numpy in and out, ``bits`` uint64.  ``model_dim``: the dimension the test
    vectors must have."""
    label = family.label
    test = np.ascontiguousarray(np.atleast_2d(test), dtype=np.float64)
    nt, D = int(test.shape[0]), int(test.shape[1])
    if operands is None:
        train = np.ascontiguousarray(np.atleast_2d(train), dtype=np.float64)
        if model_dim != D or (train.shape[0] and train.shape[1] != D):
            raise _lib.MfaHipError(f"{label}: vectors {test.shape} and {train.shape} {family.mismatch.format(model_dim)}")
        if unit:
            test, train = np.ascontiguousarray(_unit_rows(test)), np.ascontiguousarray(_unit_rows(train))
        ns = int(train.shape[0])
        n = None if train_n is None or code != 0 else np.ascontiguousarray(train_n, dtype=np.int32)
        if n is not None and n.shape != (ns,):
            raise _lib.MfaHipError(f"{label}: one number of examples per train vector")
        psi = np.ascontiguousarray(model.psi, dtype=np.float64) if code == 0 else None
        entry, head = family.host, (test, nt, train, ns, D, *((code,) if family.bits else ()), n, psi)
    else:
        A, B, c = (np.ascontiguousarray(a, dtype=np.float64) for a in operands)
        ns = int(c.shape[0])
        entry, head = family.host_operands, (test, nt, D, A, B, c, ns)
    if want_bits and threshold is None:
        raise _lib.MfaHipError(f"{label}: the bits need a threshold")
    scores = np.empty((nt, ns)) if want_scores else None
    bi, bs = (np.empty(nt, np.int32), np.empty(nt)) if want_best else (None, None)
    ki, ks = (np.empty((nt, k), np.int32), np.empty((nt, k))) if want_knn else (None, None)
    bits = np.zeros((nt, (ns + 63) // 64), dtype=np.uint64) if want_bits else None
    if family.bits and ns == 0 and not (want_scores or want_best or want_knn):
        return None, None, None, bits
    outs = (scores, bi, bs, ki, ks)
    tail = (0.0 if threshold is None else float(threshold), *outs, bits) if family.bits else outs
    twin_call(entry, _PLDA_TWIN_CODES, *head, int(bool(exclude_diagonal)), int(k), *tail)
    return scores, (bi, bs) if want_best else None, (ki, ks) if want_knn else None, bits


def _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, k, want_scores, want_best, want_knn, operands=None):
    """One scoring call: (scores or None, (best index, best score) or None, (k-NN indices, scores) or None), on the device."""
    D = model.dim if operands is None else int(np.shape(operands[0])[1])
    return _device_sweep(engine, _PLDA_SWEEP, 0, D, False, test, train, None, model, train_n, exclude_diagonal, k, want_scores, want_best,
                         want_knn, False, operands)[:3]


def plda_scores(engine, model, test, train, train_n=None, block_bytes: int = PLDA_BLOCK_BYTES,
                max_bytes: int = PLDA_MATRIX_BYTES) -> np.ndarray:
    """The matrix [test, train] of log-likelihood ratios (mfa_plda_score_batch), vectors in the model's space (``plda_transform``),
    ``train_n`` the examples behind each train vector.  The device writes row blocks of at most ``block_bytes``; the matrix
    is handed out as a numpy array.  One larger than ``max_bytes`` is refused: the consumers that need no stored matrix are
    ``plda_classify`` and ``plda_knn``."""
    test = _plda_vectors(engine, test, model.dim, "plda_scores")
    train = _plda_vectors(engine, train, model.dim, "plda_scores")
    nt, ns = int(test.shape[0]), int(train.shape[0])
    if nt * ns * 8 > max_bytes:
        raise _lib.MfaHipError(f"plda_scores: a matrix of {nt} x {ns} scores ({nt * ns * 8} bytes) exceeds {max_bytes} bytes: "
                               "use plda_knn or plda_classify, which keep no matrix")
    train_n = _plda_counts(engine, train_n, ns, "plda_scores")
    out = np.empty((nt, ns))
    rows = max(1, int(block_bytes) // max(ns * 8, 1))
    for r0 in range(0, nt, rows):
        out[r0: r0 + rows] = _plda_score_call(engine, model, test[r0: r0 + rows], train, train_n, False, 1, True, False, False)[0].cpu().numpy()
    return out


def plda_classify(engine, model, test, train, train_n=None, exclude_diagonal: bool = False):
    """Every test vector's best train vector: (index int32 [n_test], score float64 [n_test]) on the device; −1 and −inf for a
    row without a finite score.  Ties go to the lower index.  No matrix is stored."""
    return _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, 1, False, True, False)[1]


def plda_knn(engine, model, test, train, k: int, train_n=None, exclude_diagonal: bool = False):
    """Every test vector's ``k`` (1 to 64) best train vectors, best first: (indices int32 [n_test, k], scores float64 [n_test, k])
    on the device, padded with −1 and −inf.  ``exclude_diagonal``: test and train are the same vectors, skip j == i."""
    return _plda_score_call(engine, model, test, train, train_n, exclude_diagonal, int(k), False, False, True)[2]


def plda_sweep(engine, test, A, B, c, exclude_diagonal: bool = False, k: int = 1, want_scores=True, want_best=True, want_knn=True):
    """The sweep alone over the caller's operands (mfa_debug_plda_sweep_batch; tests)."""
    return _plda_score_call(engine, None, test, None, None, exclude_diagonal, int(k), want_scores, want_best, want_knn, operands=(A, B, c))


def plda_prepare_host(model, train, train_n=None):
    """(A [n, D], B [n, D], c [n]) of the train vectors on the host twin (mfa_debug_plda_prepare_host)."""
    train = np.ascontiguousarray(np.atleast_2d(train), dtype=np.float64)
    n = None if train_n is None else np.ascontiguousarray(train_n, dtype=np.int32)
    psi = np.ascontiguousarray(model.psi, dtype=np.float64)
    A, B, c = np.empty_like(train), np.empty_like(train), np.empty(train.shape[0])
    twin_call("mfa_debug_plda_prepare_host", _PLDA_TWIN_CODES, train, int(train.shape[0]), int(train.shape[1]), n, psi, A, B, c)
    return A, B, c


def _plda_host_call(model, test, train, train_n, exclude_diagonal, k, want_scores, want_best, want_knn, operands=None):
    return _host_sweep(_PLDA_SWEEP, 0, None if operands is not None else model.dim, False, test, train, None, model, train_n, exclude_diagonal,
                       k, want_scores, want_best, want_knn, False, operands)[:3]


def plda_scores_host(model, test, train, train_n=None) -> np.ndarray:
    """``plda_scores`` on the host twin (the expanded form in plain loops): numpy in and out."""
    return _plda_host_call(model, test, train, train_n, False, 1, True, False, False)[0]


def plda_classify_host(model, test, train, train_n=None, exclude_diagonal: bool = False):
    return _plda_host_call(model, test, train, train_n, exclude_diagonal, 1, False, True, False)[1]


def plda_knn_host(model, test, train, k: int, train_n=None, exclude_diagonal: bool = False):
    return _plda_host_call(model, test, train, train_n, exclude_diagonal, int(k), False, False, True)[2]


def plda_sweep_host(test, A, B, c, exclude_diagonal: bool = False, k: int = 1, want_scores=True, want_best=True, want_knn=True):
    """``plda_sweep`` on the host twin (mfa_debug_plda_sweep_host)."""
    return _plda_host_call(None, test, None, None, exclude_diagonal, int(k), want_scores, want_best, want_knn, operands=(A, B, c))


# ---- the sweep for any metric and its fourth consumer, the neighbour bit matrix; DBSCAN on it (include/mfa_hip.h "Neighbour bits",
# "Clustering") ------------------------------------------------------------------------------------------------------------------
METRIC_CODES = {"plda": 0, "euclidean": 1, "dot": 2, "cosine": 2}      # cosine: the dot metric on rows made unit length here
NEIGHBOR_BITS_BYTES = 4 << 30                                # the largest bit matrix ``neighbor_bits`` hands out
_PLDA_TWIN_CODES.update({-8: "an unknown metric", -9: "a threshold that is not a number"})
_CLUSTER_TWIN_CODES = {-2: "a number of points outside [0, 2^31)", -3: "min_samples below 1"}


def metric_code(metric) -> int:
    name = getattr(metric, "name", metric)
    if name not in METRIC_CODES:
        raise _lib.MfaHipError(f"metric {metric!r}: one of {sorted(METRIC_CODES)}")
    return METRIC_CODES[name]


def score_threshold(metric, eps: float) -> float:
    """The sweep's threshold for "distance <= eps": plda −eps (the distance is −LLR), euclidean −eps² (eps < 0: no pair passes),
    cosine 1 − eps."""
    code, eps = metric_code(metric), float(eps)
    if code == 0:
        return -eps
    if code == 1:
        return float("inf") if eps < 0 else -(eps * eps)
    return 1.0 - eps


def score_to_distance(metric, scores):
    """Distances from the sweep's scores (numpy): −score, sqrt(−score) floored at 0, 1 − score."""
    code, s = metric_code(metric), np.asarray(scores, dtype=np.float64)
    if code == 0:
        return -s
    return np.sqrt(np.maximum(-s, 0.0)) if code == 1 else 1.0 - s


def _unit_rows(x):
    """Rows made unit length in float64 (torch or numpy); a zero row becomes NaN and is nobody's neighbour."""
    if isinstance(x, torch.Tensor):
        return x / torch.sqrt((x * x).sum(dim=1, keepdim=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def _metric_dim(code: int, model, x) -> int:
    if code == 0:
        if model is None:
            raise _lib.MfaHipError("the plda metric needs the model")
        return model.dim
    return int(np.shape(x)[-1])


def _sweep_metric(metric, model, test, operands):
    """(the library's metric code, the vectors' dimension, whether rows are made unit length first) of a sweep for ``metric``, or
    over ready ``operands`` (the plda form)."""
    if operands is not None:
        return 0, int(np.shape(operands[0])[1]), False
    code = metric_code(metric)
    return code, _metric_dim(code, model, test), getattr(metric, "name", metric) == "cosine"


def metric_sweep(engine, metric, test, train, threshold=None, model=None, train_n=None, exclude_diagonal: bool = False, k: int = 1,
                 want_scores=False, want_best=False, want_knn=False, want_bits=True, operands=None):
    """One sweep on the device for ``metric`` ("plda", "euclidean", "cosine", or "dot": cosine's sweep on the rows as they are;
    mfa_neighbor_bits_batch): (scores, best, knn, bits), each
    None unless asked for.  ``threshold`` is on the score, as the library takes it (``score_threshold``); ``bits`` is int64
    [n_test, ceil(n_train / 64)] on the device, the words' bits as they are.  ``operands``: the debug entry's (A, B, c)."""
    return _device_sweep(engine, _METRIC_SWEEP, *_sweep_metric(metric, model, test, operands), test, train, threshold, model, train_n,
                         exclude_diagonal, k, want_scores, want_best, want_knn, want_bits, operands)


def metric_sweep_host(metric, test, train, threshold=None, model=None, train_n=None, exclude_diagonal: bool = False, k: int = 1,
                      want_scores=False, want_best=False, want_knn=False, want_bits=True, operands=None):
    """``metric_sweep`` on the host twins (mfa_debug_neighbor_bits_host / mfa_debug_neighbor_sweep_host): numpy in and out, ``bits``
    uint64."""
    return _host_sweep(_METRIC_SWEEP, *_sweep_metric(metric, model, test, operands), test, train, threshold, model, train_n, exclude_diagonal,
                       k, want_scores, want_best, want_knn, want_bits, operands)


def _bits_size_check(nt: int, ns: int, max_bytes: int) -> None:
    size = nt * ((ns + 63) // 64) * 8
    if size > max_bytes:
        raise _lib.MfaHipError(f"neighbor_bits: a bit matrix of {nt} x {ns} pairs ({size} bytes) exceeds {max_bytes} bytes")


def neighbor_bits(engine, metric, test, train, eps: float, model=None, train_n=None, max_bytes: int = NEIGHBOR_BITS_BYTES) -> torch.Tensor:
    """The ε-neighbourhoods as a bit matrix: int64 words [n_test, ceil(n_train / 64)] on the device, bit j & 63 of word j >> 6 of row i
    set iff the distance of test i to train j is at most ``eps`` in ``metric`` (plda: −LLR, vectors in the model's space).  N²/8
    bytes where the score matrix takes 8 N²; one above ``max_bytes`` is refused."""
    _bits_size_check(int(np.shape(test)[0]), int(np.shape(train)[0]), max_bytes)
    return metric_sweep(engine, metric, test, train, score_threshold(metric, eps), model, train_n)[3]


def neighbor_bits_host(metric, test, train, eps: float, model=None, train_n=None, max_bytes: int = NEIGHBOR_BITS_BYTES) -> np.ndarray:
    _bits_size_check(int(np.shape(test)[0]), int(np.shape(train)[0]), max_bytes)
    return metric_sweep_host(metric, test, train, score_threshold(metric, eps), model, train_n)[3]


def knn(engine, metric, test, train, k: int, model=None, train_n=None, exclude_diagonal: bool = False):
    """``plda_knn`` for any metric: (indices int32 [n_test, k], scores float64 [n_test, k]) on the device, the nearest first; the
    scores are the sweep's (``score_to_distance`` makes distances of them)."""
    return metric_sweep(engine, metric, test, train, None, model, train_n, exclude_diagonal, int(k), want_knn=True, want_bits=False)[2]


def knn_host(metric, test, train, k: int, model=None, train_n=None, exclude_diagonal: bool = False):
    return metric_sweep_host(metric, test, train, None, model, train_n, exclude_diagonal, int(k), want_knn=True, want_bits=False)[2]


def _square_bits(bits, n) -> int:
    n = int(bits.shape[0]) if n is None else int(n)
    if bits.ndim != 2 or tuple(bits.shape) != (n, (n + 63) // 64):
        raise _lib.MfaHipError(f"dbscan_from_bits: words {tuple(bits.shape)} for {n} points (a square matrix of [n, ceil(n / 64)] words)")
    return n


def dbscan_from_bits(engine, bits, min_samples: int, n=None):
    """DBSCAN on a square neighbour matrix (mfa_dbscan_from_bits): dict(labels, core, count: int32 [n] on the device, n_clusters, rounds,
    bits: the symmetrised matrix).  A tensor on the engine's device is symmetrised in place; anything else is copied first."""
    if isinstance(bits, torch.Tensor) and bits.dtype == torch.int64 and bits.device == engine.device and bits.is_contiguous():
        d = bits
    else:
        a = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
        d = torch.from_numpy(np.ascontiguousarray(a).astype(np.uint64, copy=False).view(np.int64).copy()).to(engine.device)
    n = _square_bits(d, n)
    labels, core, count = (torch.empty(n, dtype=torch.int32, device=engine.device) for _ in range(3))
    n_clusters, rounds = engine._launch_dbscan(d, n, int(min_samples), labels, core, count)
    return dict(labels=labels, core=core, count=count, n_clusters=n_clusters, rounds=rounds, bits=d)


def dbscan_from_bits_host(bits, min_samples: int, n=None):
    """``dbscan_from_bits`` on the host twin: numpy arrays, the input left alone."""
    a = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    h = np.ascontiguousarray(a).view(np.uint64).copy() if a.dtype == np.int64 else np.ascontiguousarray(a, dtype=np.uint64).copy()
    n = _square_bits(h, n)
    labels, core, count = (np.empty(n, np.int32) for _ in range(3))
    n_clusters = ctypes.c_int32(0)
    twin_call("mfa_debug_dbscan_from_bits_host", _CLUSTER_TWIN_CODES, h, n, int(min_samples), labels, core, count, ctypes.byref(n_clusters))
    return dict(labels=labels, core=core, count=count, n_clusters=int(n_clusters.value), bits=h)


# ---- HDBSCAN: the pair form, the core scores and the mutual-reachability spanning tree (include/mfa_hip.h "HDBSCAN") -------------------
_HDBSCAN_TWIN_CODES = {-2: "dimension outside [1, 1024]", -3: "neighbours outside [0, 64]", -4: "a psi entry that is not positive and finite",
                       -5: "2^31 points or more", -8: "an unknown metric"}


def pair_metric(metric):
    """(the library's metric code, rows made unit length first, the metric of ``score_to_distance``) of the pair form: cosine is
    euclidean on unit rows, which is what the reference's hdbscan branch clusters."""
    name = getattr(metric, "name", metric)
    code = metric_code(name)
    return (1, True, "euclidean") if name == "cosine" else (code, False, name)


def _pair_k(k) -> int:
    k = int(k)
    if not 0 <= k <= 64:
        raise _lib.MfaHipError(f"core_scores: {k} neighbours (0 to 64: a row's list is one wavefront register); min_samples up to 65")
    return k


def core_scores(engine, metric, x, k: int, model=None, want_v: bool = False):
    """The pair form of ``x`` [n, D] and every point's core score (mfa_hdbscan_core_batch): dict(y [n, D], q [n], core [n], v [n, n] or
    None, code) on the device.  ``k = min_samples − 1`` (0 to 64): the core score is the k-th best score over the other points, −inf
    for a point with fewer than k finite ones, +inf at k = 0.  Scores are larger-is-nearer; ``score_to_distance`` of
    ``pair_metric(metric)[2]`` makes distances of them."""
    code, unit, _ = pair_metric(metric)
    k = _pair_k(k)
    x = _plda_vectors(engine, x, _metric_dim(code, model, x), "core_scores")
    if unit:
        x = _unit_rows(x)
    n, dev = int(x.shape[0]), engine.device
    psi = _plda_device_model(engine, model)[2] if code == 0 else None
    y, q, core = torch.empty_like(x), torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    v = torch.empty((n, n), dtype=torch.float64, device=dev) if want_v else None
    engine._launch_hdbscan_core(x, code, psi, k, y, q, core, v)
    return dict(y=y, q=q, core=core, v=v, code=code)


def pair_prepare(engine, metric, x, model=None):
    """(y [n, D], q [n]) of the pair form on the device: v(i, j) = (q_i + q_j) + w · y_i · y_j, bit-symmetric in (i, j)."""
    r = core_scores(engine, metric, x, 0, model)
    return r["y"], r["q"]


def core_scores_host(metric, x, k: int, model=None, want_v: bool = False, v=None):
    """``core_scores`` on the host twin: numpy arrays.  ``v``: a score matrix to take the core scores from (tests: the device's own)."""
    code, unit, _ = pair_metric(metric)
    k = _pair_k(k)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    if _metric_dim(code, model, x) != x.shape[1]:
        raise _lib.MfaHipError(f"core_scores_host: vectors {x.shape} for a model of dimension {model.dim}")
    if unit:
        x = np.ascontiguousarray(_unit_rows(x))
    n = int(x.shape[0])
    psi = np.ascontiguousarray(model.psi, dtype=np.float64) if code == 0 else None
    v_in = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    if v_in is not None and v_in.shape != (n, n):
        raise _lib.MfaHipError(f"core_scores_host: a score matrix {v_in.shape} for {n} points")
    y, q, core = np.empty_like(x), np.empty(n), np.empty(n)
    out_v = np.empty((n, n)) if want_v else None
    twin_call("mfa_debug_hdbscan_core_host", _HDBSCAN_TWIN_CODES, x, n, int(x.shape[1]), code, psi, k, y, q, core, out_v, v_in)
    return dict(y=y, q=q, core=core, v=out_v, code=code)


def pair_prepare_host(metric, x, model=None):
    r = core_scores_host(metric, x, 0, model)
    return r["y"], r["q"]


def finish_tree(n: int, lo, hi, score):
    """The spanning forest's edges sorted by the edge order (larger score, then smaller lo, then smaller hi); the components that
    no finite score joins are tied to the first one's smallest member at score −inf (distance +inf): n − 1 edges."""
    lo, hi, score = np.asarray(lo, np.int32), np.asarray(hi, np.int32), np.asarray(score, np.float64)
    if n > 1 and lo.shape[0] < n - 1:
        parent = np.arange(n)

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for a, b in zip(lo.tolist(), hi.tolist()):
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)                      # the smaller root stays: a root is its component's smallest member
        roots = sorted({find(i) for i in range(n)})
        lo = np.concatenate([lo, np.full(len(roots) - 1, roots[0], np.int32)])
        hi = np.concatenate([hi, np.asarray(roots[1:], np.int32)])
        score = np.concatenate([score, np.full(len(roots) - 1, -np.inf)])
    order = np.lexsort((hi, lo, -score))
    return lo[order], hi[order], score[order]


def mreach_mst(engine, metric, y, q, core):
    """The minimum spanning tree of the mutual-reachability graph (mfa_hdbscan_mst_batch) from the pair form and the core scores on
    the device: dict(lo, hi, score: numpy [n − 1], sorted by the edge order; found: the edges the device found, rounds).  No n × n
    array is stored: every Borůvka round is one sweep."""
    code = pair_metric(metric)[0]
    dev = engine.device
    y, q, core = (_device_f64(engine, a) for a in (y, q, core))
    n = int(y.shape[0])
    if y.dim() != 2 or tuple(q.shape) != (n,) or tuple(core.shape) != (n,):
        raise _lib.MfaHipError(f"mreach_mst: y {tuple(y.shape)}, q {tuple(q.shape)} and core {tuple(core.shape)} do not go together")
    m = max(n - 1, 1)
    lo, hi = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
    score = torch.empty(m, dtype=torch.float64, device=dev)
    found, rounds = engine._launch_hdbscan_mst(y, q, core, code, lo, hi, score)
    flo, fhi, fs = finish_tree(n, lo[:found].cpu().numpy(), hi[:found].cpu().numpy(), score[:found].cpu().numpy())
    return dict(lo=flo, hi=fhi, score=fs, found=found, rounds=rounds)


def mreach_mst_host(metric, y, q, core, v=None):
    """``mreach_mst`` on the host twin, Kruskal under the same edge order; ``v``: a score matrix to use in place of the pair form's."""
    code = pair_metric(metric)[0]
    y = np.ascontiguousarray(np.atleast_2d(y), dtype=np.float64)
    q, core = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(core, dtype=np.float64)
    n = int(y.shape[0])
    v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    if q.shape != (n,) or core.shape != (n,) or (v is not None and v.shape != (n, n)):
        raise _lib.MfaHipError("mreach_mst_host: y, q, core and v do not go together")
    m = max(n - 1, 1)
    lo, hi, score = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m)
    found = ctypes.c_int32(0)
    twin_call("mfa_debug_hdbscan_mst_host", _HDBSCAN_TWIN_CODES, y, q, core, v, n, int(y.shape[1]), code, lo, hi, score, ctypes.byref(found))
    f = int(found.value)
    flo, fhi, fs = finish_tree(n, lo[:f], hi[:f], score[:f])
    return dict(lo=flo, hi=fhi, score=fs, found=f)


# ---- Silhouette: every point's coefficient from the pair sweep, the columns ordered by cluster (include/mfa_hip.h "Silhouette") ---------
_SILHOUETTE_TWIN_CODES = {-2: "dimension outside [1, 1024]", -4: "a psi entry that is not positive and finite", -5: "2^31 points or more",
                          -6: "a number of clusters outside [2, the number of points]",
                          -7: "offsets that are not 0 = off[0] < ... < off[C] = the number of points", -8: "an unknown metric"}


def _silhouette_offsets(offsets) -> np.ndarray:
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    if off.ndim != 1 or off.shape[0] < 1:
        raise _lib.MfaHipError(f"silhouette: offsets {off.shape} (one more than the clusters)")
    return off


def _silhouette_result(sil, parts, v, code):
    a, b, bj = parts if parts is not None else (None, None, None)
    return dict(sil=sil, a=a, b=b, bj=bj, v=v, code=code)


def silhouette(engine, metric, x, offsets, model=None, want_parts: bool = False, want_v: bool = False):
    """Every row's silhouette coefficient (mfa_silhouette_batch) for rows ordered by cluster: cluster c is the rows
    ``offsets[c] : offsets[c + 1]``.  dict(sil [n], a, b [n] and bj int32 [n] or None, v [n, n] or None, code) on the device.
    ``metric`` as ``core_scores`` takes it: cosine is euclidean on unit rows there too; the cosine distance itself is "dot" on rows the
    caller made unit length.  No n × n array is stored unless ``want_v``."""
    code, unit, _ = pair_metric(metric)
    x = _plda_vectors(engine, x, _metric_dim(code, model, x), "silhouette")
    if unit:
        x = _unit_rows(x)
    n, dev = int(x.shape[0]), engine.device
    off = torch.from_numpy(_silhouette_offsets(offsets)).to(dev)
    psi = _plda_device_model(engine, model)[2] if code == 0 else None
    sil = torch.empty(n, dtype=torch.float64, device=dev)
    parts = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
             torch.empty(n, dtype=torch.int32, device=dev)) if want_parts else None
    v = torch.empty((n, n), dtype=torch.float64, device=dev) if want_v else None
    engine._launch_silhouette(x, code, psi, off, sil, *(parts or (None, None, None)), v)
    return _silhouette_result(sil, parts, v, code)


def silhouette_host(metric, x, offsets, model=None, want_parts: bool = False, want_v: bool = False, v=None):
    """``silhouette`` on the host twin: numpy arrays.  ``v``: a score matrix to take the distances from (tests: the device's own)."""
    code, unit, _ = pair_metric(metric)
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    if _metric_dim(code, model, x) != x.shape[1]:
        raise _lib.MfaHipError(f"silhouette_host: vectors {x.shape} for a model of dimension {model.dim}")
    if unit:
        x = np.ascontiguousarray(_unit_rows(x))
    n = int(x.shape[0])
    off = _silhouette_offsets(offsets)
    psi = np.ascontiguousarray(model.psi, dtype=np.float64) if code == 0 else None
    v_in = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    if v_in is not None and v_in.shape != (n, n):
        raise _lib.MfaHipError(f"silhouette_host: a score matrix {v_in.shape} for {n} points")
    sil = np.empty(n)
    parts = (np.empty(n), np.empty(n), np.empty(n, np.int32)) if want_parts else None
    out_v = np.empty((n, n)) if want_v else None
    twin_call("mfa_debug_silhouette_host", _SILHOUETTE_TWIN_CODES, x, n, int(x.shape[1]), code, psi, off, int(off.shape[0]) - 1, sil,
              *(parts or (None, None, None)), out_v, v_in)
    return _silhouette_result(sil, parts, out_v, code)
