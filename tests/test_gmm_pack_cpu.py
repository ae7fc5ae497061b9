"""The model packer (csrc/gmm_pack.cpp) without a GPU, through mfa_debug_gmm_pack: the row layout, the bf16×3 and the
column-scaled f16×2 operand tables, the flags mfa_load_gmm keeps, and the pdf-list sort.

Bounds.  bf16×3: a float32 has 24 significand bits, three bf16 pieces hold 8 each, every remainder is exact in float32 — the
pieces sum to the weight exactly (float64 holds the sum).  f16×2: v = w·2^e_k is exact; hi = f16(v) errs by ≤ 2^-11·|v|
(or 2^-25, half the subnormal spacing 2^-24); lo = f16(v − hi) errs by ≤ 2^-11·|v − hi| ≤ 2^-22·|v| (or 2^-25 again), and
v − hi itself is exact in float32 — so |hi + lo − v| ≤ max(2^-22·|v|, 2^-25), met with equality by some values."""
import ctypes as C

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from tests import gmm_ref, helpers

SIZES = [1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 26, 32, 33, 40, 70]
DIMS = [39, 40, 45, 48, 50]


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _pack(am, sort=None, keys=None):
    """Everything mfa_load_gmm would upload, as numpy arrays; `sort`: a pdf list to sort along (in place, with `keys`)."""
    po = np.ascontiguousarray(am.pdf_offsets, np.int32)
    gc = np.ascontiguousarray(am.gconsts, np.float32)
    mi = np.ascontiguousarray(am.means_invvars, np.float32)
    iv = np.ascontiguousarray(am.inv_vars, np.float32)
    n = len(po) - 1
    info, acc = np.zeros(13, np.int32), C.c_float(0)
    call = lambda *arrs: _lib.lib().mfa_debug_gmm_pack(am.dim, n, po.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data,
                                                       info.ctypes.data, C.byref(acc), *arrs)
    assert call(*([None] * 9), None, None, 0, None) == 0          # sizes first
    kpad, rows, blocks, split = (int(v) for v in info[:4])
    out = dict(row0=np.zeros(n + 1, np.int32), nblk=np.zeros(n, np.int32), slot=np.zeros(n, np.int32),
               w=np.zeros(blocks * 32 * kpad, np.float32), gc=np.zeros(blocks * 32, np.float32),
               wb=np.zeros(blocks * 32 * kpad * 3, np.uint16), wh=np.zeros(blocks * 32 * kpad * 2, np.uint16),
               gch=np.zeros(blocks * 32, np.float32), fscale=np.full(kpad, np.nan, np.float32))
    counts = np.zeros(6, np.int32)
    rc = call(*(_ptr(out[k]) for k in ("row0", "nblk", "slot", "w", "gc", "wb", "wh", "gch", "fscale")),
              _ptr(sort), _ptr(keys), 0 if sort is None else len(sort), counts.ctypes.data)
    assert rc == 0
    out.update(kpad=kpad, rows=rows, blocks=blocks, split=bool(split), acc_scale=float(acc.value), counts=counts,
               has_slot_class=[bool(v) for v in info[4:9]], has_single32=bool(info[9]), has_multi_block=bool(info[10]),
               max_nblk=int(info[11]), all_pdfs_32row=bool(info[12]))
    return out


def _packed_offset(row, k, kpad):
    """numpy copy of mfa_packed_offset (csrc/gmm_pack.hpp)"""
    m, o = k >> 3, k & 7
    h, c = o & 1, o >> 1
    return (row >> 5) * 32 * kpad + ((2 * m + h) * 32 + (row & 31)) * 4 + c


def _split_piece(table, row, k, piece, kpad, pieces):
    """16-bit word of (row, column k, piece) in a split-operand table: blocks of [step][piece][half][row] units of 8 words"""
    steps = kpad // 16
    unit = (row >> 5) * steps * pieces * 2 * 32 + (((k >> 4) * pieces + piece) * 2 + ((k >> 3) & 1)) * 32 + (row & 31)
    return table[unit * 8 + (k & 7)]


def _model(dim, seed, zero_column=None):
    rng = np.random.default_rng(seed)
    am = helpers.random_gmm(rng, dim, [int(g) for g in rng.permutation(SIZES)])
    if zero_column is not None:
        am.means_invvars[:, zero_column] = 0.0
    return am


def _slot(g):
    return 1 if g <= 1 else 4 if g <= 4 else 8 if g <= 8 else 16 if g <= 16 else 32


SKEWED_DIMS = [39, 40, 45]


@pytest.fixture(scope="module", params=DIMS + [("skewed", d) for d in SKEWED_DIMS], ids=str)
def packed(request):
    """(model, packed arrays, the column of means·inv_vars the fixture zeroed or None): helpers.random_gmm models at DIMS, and
    models with the column spread of a trained one (tests/gmm_ref.py) at SKEWED_DIMS."""
    if isinstance(request.param, tuple):
        dim = request.param[1]
        rng = np.random.default_rng(200 + dim)
        am = gmm_ref.skewed_gmm(rng, dim, [int(g) for g in rng.permutation(SIZES)]).am
        return am, _pack(am), None
    dim = request.param
    zero_column = 3 if dim == 40 else None
    am = _model(dim, 100 + dim, zero_column=zero_column)
    return am, _pack(am), zero_column


def test_layout(packed):
    am, pk, _ = packed
    dim, kpad, rows = am.dim, pk["kpad"], pk["rows"]
    assert kpad == (80 if 2 * dim <= 80 else 96 if 2 * dim <= 96 else (2 * dim + 7) // 8 * 8)
    g = np.diff(am.pdf_offsets)
    slot = np.array([_slot(x) for x in g])
    nblk = np.where(slot == 32, (g + 31) // 32, 1)
    assert np.array_equal(pk["slot"], slot) and np.array_equal(pk["nblk"], nblk)
    # rows are handed out in class order 32, 16, 8, 4, 1 (pdf order inside a class)
    want, r = np.zeros(len(g), np.int64), 0
    for cls in (32, 16, 8, 4, 1):
        for p in np.flatnonzero(slot == cls):
            want[p] = r
            r += 32 * nblk[p] if cls == 32 else cls
    assert np.array_equal(pk["row0"][:-1], want)
    assert np.all(pk["row0"][:-1] % slot == 0)
    assert rows % 4 == 0 and r <= rows < r + 4 and pk["row0"][-1] == rows
    assert pk["blocks"] == (rows + 1 + 31) // 32
    # every Gaussian's weights and gconst, read back through the layout
    k = np.arange(2 * dim)
    used = np.zeros(pk["blocks"] * 32, bool)
    for p in range(len(g)):
        for i in range(g[p]):
            row, gi = int(pk["row0"][p]) + i, am.pdf_offsets[p] + i
            got = pk["w"][_packed_offset(row, k, kpad)]
            assert np.array_equal(got[:dim], am.means_invvars[gi]) and np.array_equal(got[dim:], np.float32(-0.5) * am.inv_vars[gi])
            assert pk["gc"][row] == am.gconsts[gi]
            used[row] = True
    # pad rows, the dummy row `rows` among them, and the pad columns: zero weights; pad gconsts −1e30
    assert not used[rows]
    wmat = pk["w"][_packed_offset(np.arange(pk["blocks"] * 32)[:, None], np.arange(kpad)[None, :], kpad)]
    assert np.all(wmat[~used] == 0.0) and np.all(wmat[:, 2 * dim:] == 0.0)
    assert np.all(pk["gc"][~used] == np.float32(-1e30))
    # the flags mfa_load_gmm keeps
    assert pk["has_slot_class"] == [bool(np.any(slot == c)) for c in (32, 16, 8, 4, 1)]
    assert pk["has_single32"] == bool(np.any((slot == 32) & (nblk == 1)))
    assert pk["has_multi_block"] == bool(np.any(nblk > 1)) and pk["max_nblk"] == nblk.max()
    assert pk["all_pdfs_32row"] == bool(np.all(slot == 32))


def test_all_pdfs_32row_flag():
    am = helpers.random_gmm(np.random.default_rng(7), 39, [17, 32, 40])
    pk = _pack(am)
    assert pk["all_pdfs_32row"] and pk["has_slot_class"] == [True, False, False, False, False]
    assert pk["has_single32"] and pk["has_multi_block"] and pk["max_nblk"] == 2


def _bf16_to_f64(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def test_split_tables(packed):
    am, pk, zero_column = packed
    dim, kpad, rows = am.dim, pk["kpad"], pk["rows"]
    if dim > 48:
        assert not pk["split"] and kpad > 96 and pk["acc_scale"] == 1.0   # above 48 dims: no split tables
        return
    assert pk["split"]
    row = np.arange(pk["blocks"] * 32)[:, None]
    k = np.arange(kpad)[None, :]
    w = pk["w"][_packed_offset(row, k, kpad)].astype(np.float64)
    # ---- bf16×3: the three pieces of every weight sum to it exactly
    pieces = [_bf16_to_f64(_split_piece(pk["wb"], row, k, q, kpad, 3)) for q in range(3)]
    assert np.array_equal(pieces[0] + pieces[1] + pieces[2], w)
    # ---- f16×2
    s, fscale = pk["acc_scale"], pk["fscale"].astype(np.float64)
    assert np.log2(s) == np.round(np.log2(s)) and 2.0 ** -20 <= s <= 2.0 ** 12
    nonzero = np.any(w[:rows] != 0.0, axis=0)
    want_nonzero = np.arange(kpad) < 2 * dim
    if zero_column is not None:
        want_nonzero[zero_column] = False                                          # the fixture zeroed this column of means·inv_vars
    assert np.array_equal(nonzero, want_nonzero)
    assert np.all(fscale[~nonzero] == 0.0) and np.all(fscale[nonzero] > 0.0)
    e = np.zeros(kpad)
    e[nonzero] = np.log2(s / fscale[nonzero])
    assert np.array_equal(e, np.round(e))                                 # powers of two
    hi = _split_piece(pk["wh"], row, k, 0, kpad, 2).view(np.float16).astype(np.float64)
    lo = _split_piece(pk["wh"], row, k, 1, kpad, 2).view(np.float16).astype(np.float64)
    assert np.all(np.abs(hi) <= 32768.0) and np.all(np.abs(lo) <= 32768.0)
    v = np.ldexp(w, e.astype(np.int64)[None, :])
    err = np.abs(hi + lo - v)
    bound = np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)
    print(f"dim {dim}: acc_scale 2^{int(np.log2(s))}, e_k in [{int(e.min())}, {int(e.max())}], max |hi+lo-v|/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(pk["gch"], pk["gc"] * np.float32(s))


def test_sort_unkeyed_is_keyed_with_equal_keys():
    rng = np.random.default_rng(3)
    am = _model(39, 11)
    n = len(am.pdf_offsets) - 1
    pdfs = rng.integers(0, n, size=200).astype(np.int32)
    assert set(np.diff(am.pdf_offsets)[pdfs]) == set(SIZES)                   # a list holding every class
    a, b, keys = pdfs.copy(), pdfs.copy(), np.full(len(pdfs), 5, np.int32)
    pa, pb = _pack(am, sort=a), _pack(am, sort=b, keys=keys)
    assert np.array_equal(a, b) and np.array_equal(pa["counts"], pb["counts"]) and np.all(keys == 5)
    # class order {32 rows one block, 32 rows several blocks, 16, 8, 4, 1}, list order kept inside a class
    g = np.diff(am.pdf_offsets)
    cls = np.array([0 if 16 < x <= 32 else 1 if x > 32 else 2 if x > 8 else 3 if x > 4 else 4 if x > 1 else 5 for x in g])
    assert np.array_equal(a, pdfs[np.argsort(cls[pdfs], kind="stable")])
    assert np.array_equal(pa["counts"], np.bincount(cls[pdfs], minlength=6))
    # with real keys: ascending inside every class, ties in list order
    c, keys = pdfs.copy(), rng.integers(0, 9, size=len(pdfs)).astype(np.int32)
    order = np.lexsort((np.arange(len(pdfs)), keys, cls[pdfs]))
    want_keys = keys[order]
    _pack(am, sort=c, keys=keys)
    assert np.array_equal(c, pdfs[order]) and np.array_equal(keys, want_keys)
