"""List passes and redo sweeps on small strided grids (gmm_band_kernel<…, true>, gmm_band_f32_strided_kernel).

A list pass (table growth, retry beam) scores a handful of utterances and a redo sweep a handful of tiles; both walk their
items on a small fixed grid instead of launching one wavefront per item of the whole batch.  Only the mapping from
wavefront to item changes, so every output must keep its bits.  MFA_LIST_GRID=1 and =3 (ungrouped plans; 1, 16 and 24 for
grouped ones, see PLANS) shrink the grid until wavefronts walk several items and the stride does not divide the item
count; each case is compared
  * with the same call under the default grid and under a grid as large as the full one (one item per wavefront, the
    mapping the launches had before): status, ali, words, n_words, like, frame_like and the score matrix, bit for bit;
  * with the one-launch dense path (``score`` + ``align``) under MFA_GMM_BF16=0, where dense and lazy scoring run the same
    f32 arithmetic for every class and are bit-identical (tests/test_gpu_lazy.py compares the same way): here the list
    passes go through the strided f32 kernel for every class;
  * cell by cell with the dense matrix under the default arithmetic: bit-identical except in pdfs of several blocks, which
    both paths merge on the f16 pipe with their own block schedules (≤ 1e-4 relative, as tests/test_gpu_lazy.py holds them).
Shapes: 11 utterances of 130–300 frames (the last 64-frame sub-tile of a 256-frame list window is ragged, the frame counts
differ), a 40-dimensional model whose mixtures cover every slot class (1, 4, 8, 16, 32 rows and several blocks), random
graphs of 40–1 100 states; grouped (8 runs) and ungrouped score plans."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests.test_gpu_parity import _random_graph

pytestmark = pytest.mark.gpu

DIM = 40
N_UTT = 11
KEYS = ("status", "ali", "words", "n_words", "like", "frame_like")
CAPS = dict(max_tokens=2048, bp_tokens_per_frame=1100, acoustic_scale=0.1, want_frame_likes=True)
FIRST_BEAM, RETRY_BEAM = 8.0, 32.0          # tight enough that some utterances of the pool fail the first beam
WIDE_BEAM = 30.0                            # keeps far more than the first tier's 64 tokens alive


# (score plan's runs, MFA_LIST_GRID).  A launch over a grouped plan rounds its grid up to a multiple of the runs, so 1 is one
# workgroup per run (every value up to 8 is): 16 and 24 give two and three per run, strides of 8 and 12 wavefronts — a
# list of three utterances is 12 items per run, which 8 does not divide, and the second and third workgroup of a run walk too.
PLANS = [(8, 1), (8, 16), (8, 24), (1, 1), (1, 3)]


def _dev(e, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(e.device)


class Pool:
    """24 utterances over one model; every case draws its batch from it.  ``need_retry(…)`` tells, from the dense path,
    which of them fail the first beam (and so sit on the retry list)."""

    def __init__(self, engine, fx):
        rng = np.random.default_rng(7100)
        self.tm = fx.mono_tm
        sizes = [int(x) for x in rng.choice([1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 26, 32, 40, 70], size=self.tm.num_pdfs)]
        assert {1, 4, 8, 16, 32, 70} <= set(sizes)
        self.am = helpers.random_gmm(rng, DIM, sizes)
        self.fsts, self.eps_fsts, self.feats = [], [], []
        while len(self.fsts) < 24:
            f = _random_graph(rng, self.tm, int(rng.choice([40, 150, 400, 1100])))
            fe = helpers.with_eps(rng, f, frac=0.2)
            if engine.needs_general_decoder(f) or engine.needs_general_decoder(fe) or helpers.has_negative_eps_cycle(fe):
                continue
            self.fsts.append(f)
            self.eps_fsts.append(fe)
            self.feats.append(rng.normal(0, 3.0, size=(int(rng.integers(130, 301)), DIM)).astype(np.float32))
        self._retry = {}

    def batch(self, idx, eps=False, feats=None):
        fsts = [(self.eps_fsts if eps else self.fsts)[u] for u in idx]
        feats = [self.feats[u] for u in idx] if feats is None else feats
        fo = np.concatenate([[0], np.cumsum([x.shape[0] for x in feats])]).astype(np.int64)
        return fsts, feats, fo

    def need_retry(self, engine, monkeypatch, eps):
        """Per utterance of the pool: the dense path's status (1, 2: decoded, or failed, by the retry beam; 0: by the first)."""
        if eps not in self._retry:
            fsts, feats, fo = self.batch(range(24), eps)
            monkeypatch.setenv("MFA_GMM_BF16", "0")
            g = engine.pack_graphs(fsts, self.tm)
            d = _dev(engine, np.concatenate(feats))
            ll, ll_off, ll_cols = engine.score(d, fo, g.pdf_list, g.pdf_off_host, g.class_counts)
            st = engine.align(g, ll, ll_off, ll_cols, fo, beam=FIRST_BEAM, retry_beam=RETRY_BEAM, **CAPS)["status"].cpu().numpy()
            monkeypatch.delenv("MFA_GMM_BF16")
            print(f"pool statuses (eps={eps}) at beam {FIRST_BEAM}/{RETRY_BEAM}: {st.tolist()}")
            self._retry[eps] = st
        return self._retry[eps]


@pytest.fixture(scope="module")
def pool(engine, fx):
    p = Pool(engine, fx)
    engine.load_gmm(p.am)
    return p


def _same(a, b, what):
    for k in KEYS + ("loglikes",):
        assert torch.equal(a[k], b[k]), f"{k} differs {what}"


_refs = {}   # (case, groups) → the runs that do not depend on MFA_LIST_GRID, computed once


def _check(engine, pool, monkeypatch, case, groups, grid, idx, beam, retry, eps=False, feats=None, dense_cells=True, window=64):
    """Runs the batch under MFA_LIST_GRID=grid and compares as the module's docstring says.  Returns
    (dense result under f32 arithmetic, lazy result under the default arithmetic, packed graphs, dense f32 scores, frame offsets)."""
    engine.load_gmm(pool.am)
    fsts, feats, fo = pool.batch(idx, eps, feats)
    d = _dev(engine, np.concatenate(feats))
    kw = dict(beam=beam, retry_beam=retry, **CAPS)
    lazy_kw = dict(kw, window=window)
    monkeypatch.delenv("MFA_LIST_GRID", raising=False)
    if (case, groups) not in _refs:
        g = engine.pack_graphs(fsts, pool.tm, groups=groups)
        assert (g.group_counts is not None) == (groups > 1)
        default = engine.align_features(g, d, fo, **lazy_kw)
        monkeypatch.setenv("MFA_LIST_GRID", str(1 << 20))            # capped at the full grid: one item per wavefront
        full = engine.align_features(g, d, fo, **lazy_kw)
        monkeypatch.delenv("MFA_LIST_GRID")
        _same(default, full, "between the default grid and a full one")
        ll, ll_off, ll_cols = engine.score(d, fo, g.pdf_list, g.pdf_off_host, g.class_counts)
        monkeypatch.setenv("MFA_GMM_BF16", "0")
        ll32, _, _ = engine.score(d, fo, g.pdf_list, g.pdf_off_host, g.class_counts)
        dense32 = engine.align(g, ll32, ll_off, ll_cols, fo, **kw)
        monkeypatch.delenv("MFA_GMM_BF16")
        torch.cuda.synchronize()
        _refs[(case, groups)] = (g, default, ll, ll32, ll_off, dense32)
    g, default, ll, ll32, ll_off, dense32 = _refs[(case, groups)]
    monkeypatch.setenv("MFA_LIST_GRID", str(grid))
    got = engine.align_features(g, d, fo, **lazy_kw)
    _same(default, got, f"between the default grid and MFA_LIST_GRID={grid}")
    # the dense path, same f32 arithmetic on both sides
    monkeypatch.setenv("MFA_GMM_BF16", "0")
    got32 = engine.align_features(g, d, fo, **lazy_kw)
    monkeypatch.delenv("MFA_GMM_BF16")
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(dense32[k], got32[k]), f"{k} differs between lazy (MFA_LIST_GRID={grid}) and dense scoring"
    d32, s32 = ll32.cpu().numpy(), got32["loglikes"].cpu().numpy()
    w = s32 != 0.0
    assert w.any() and np.array_equal(d32[w], s32[w]), "a lazily scored f32 cell differs from the dense kernel's value"
    if not dense_cells:
        return dense32, got, g, ll32, fo
    # default arithmetic, cell by cell against the dense matrix
    dd, ss = ll.cpu().numpy(), got["loglikes"].cpu().numpy()
    cc, P = g.class_counts.cpu().numpy(), np.diff(g.pdf_off_host)
    exact = 0
    for u in range(len(fsts)):
        T = int(fo[u + 1] - fo[u])
        du, su = dd[ll_off[u]: ll_off[u + 1]].reshape(T, P[u]), ss[ll_off[u]: ll_off[u + 1]].reshape(T, P[u])
        multi = np.zeros(P[u], dtype=bool)
        multi[cc[u, 0]: cc[u, 0] + cc[u, 1]] = True
        w = su != 0.0
        assert np.array_equal(du[:, ~multi][w[:, ~multi]], su[:, ~multi][w[:, ~multi]]), f"utterance {u}"
        exact += int(w[:, ~multi].sum())
        if w[:, multi].any():
            a_, b_ = du[:, multi][w[:, multi]], su[:, multi][w[:, multi]]
            assert np.abs(a_ - b_).max() <= 1e-4 * max(1.0, float(np.abs(a_).max()))
    assert exact > 0
    return dense32, got, g, ll32, fo


def _pick(pool, engine, monkeypatch, eps, n_retry):
    st = pool.need_retry(engine, monkeypatch, eps)
    hard, easy = np.flatnonzero((st == 1) | (st == 2)).tolist(), np.flatnonzero(st == 0).tolist()   # (overflow statuses: neither)
    assert len(hard) >= n_retry and len(easy) >= N_UTT - n_retry, (hard, easy)
    return sorted(hard[:n_retry] + easy[: N_UTT - n_retry])


@pytest.mark.parametrize("groups,grid", PLANS)
@pytest.mark.parametrize("n_retry", [0, 1, 3])
def test_retry_list_of_none_one_and_several(engine, pool, monkeypatch, n_retry, groups, grid):
    """(a) The retry-beam pass over a list of 0, 1 and 3 utterances (chosen from the pool by what the dense path reports)."""
    idx = _pick(pool, engine, monkeypatch, False, n_retry)
    dense, _, _, _, _ = _check(engine, pool, monkeypatch, f"retry{n_retry}", groups, grid, idx, FIRST_BEAM, RETRY_BEAM)
    st = dense["status"].cpu().numpy()
    assert int(((st == 1) | (st == 2)).sum()) == n_retry and int((st == 0).sum()) == N_UTT - n_retry, st.tolist()


@pytest.mark.parametrize("groups,grid", PLANS)
def test_table_growth_list_is_not_empty(engine, pool, monkeypatch, groups, grid):
    """(b) A beam that keeps more tokens alive than the first tier's 64: those utterances are decoded by the table-growth
    list pass.  The oracle's token count on the dense scores shows that the list is not empty."""
    idx = list(range(N_UTT))
    dense, _, g, ll32, fo = _check(engine, pool, monkeypatch, "grow", groups, grid, idx, WIDE_BEAM, 0.0)
    if ("grow", "toks") not in _refs:
        ll = ll32.cpu().numpy()
        off = np.concatenate([[0], np.cumsum(np.diff(fo) * np.diff(g.pdf_off_host))])
        toks = []
        for u in idx[:4]:
            pl = g.pdf_lists_host[u]
            ref = helpers.oracle_align(pool.tm, pool.fsts[u], ll[off[u]: off[u + 1]].reshape(-1, len(pl)), pl, beam=WIDE_BEAM,
                                       retry_beam=0.0, want_stats=True)
            toks.append(ref["max_toks"])
        _refs[("grow", "toks")] = toks
    toks = _refs[("grow", "toks")]
    print("most live tokens of the first four utterances:", toks)
    assert max(toks) > 2 * 64, toks


@pytest.mark.parametrize("groups,grid", PLANS)
def test_bf16_redo_of_tiles_outside_the_f16_range(engine, pool, monkeypatch, groups, grid):
    """(c) Whole 64-frame tiles of three utterances scaled by 10⁴ (squares of ~10⁹: far outside the f16 range): the f16 pass
    declines them and the bf16×3 sweep scores them — in the first tier's windows and in the list passes.  In those tiles
    every cell equals the MFA_GMM_F16=0 run's (bf16×3 everywhere); elsewhere the two runs differ in some cell, i.e. the f16
    pass did score the rest.  (No cell-by-cell comparison with the dense matrix under the default arithmetic here: the dense
    kernels hand a whole 256-frame tile to the bf16×3 pass, the band kernel a 64-frame one.)"""
    idx = _pick(pool, engine, monkeypatch, False, 3)
    _, feats, _ = pool.batch(idx)
    feats = [x.copy() for x in feats]
    tiles = {0: 0, 4: 1, 7: (feats[7].shape[0] - 1) // 64}            # utterance of the batch → scaled tile (the last: ragged)
    for u, tl in tiles.items():
        feats[u][64 * tl: 64 * tl + 64] *= 1.0e4
    _, got, g, _, fo = _check(engine, pool, monkeypatch, "redo", groups, grid, idx, FIRST_BEAM, RETRY_BEAM, feats=feats,
                             dense_cells=False)
    _redo_cells(engine, monkeypatch, g, feats, fo, got, {u: [tl] for u, tl in tiles.items()}, 64)


def _redo_cells(engine, monkeypatch, g, feats, fo, got, tiles, window):
    """``tiles``: utterance of the batch → its scaled 64-frame tiles.  See test_bf16_redo_of_tiles_outside_the_f16_range."""
    monkeypatch.setenv("MFA_GMM_F16", "0")
    bf = engine.align_features(g, _dev(engine, np.concatenate(feats)), fo, beam=FIRST_BEAM, retry_beam=RETRY_BEAM, window=window,
                               **CAPS)
    monkeypatch.delenv("MFA_GMM_F16")
    a, b = got["loglikes"].cpu().numpy(), bf["loglikes"].cpu().numpy()
    P = np.diff(g.pdf_off_host)
    off = np.concatenate([[0], np.cumsum(np.diff(fo) * P)])
    other_differs = False
    for u in range(len(feats)):
        T = int(fo[u + 1] - fo[u])
        au, bu = a[off[u]: off[u + 1]].reshape(T, P[u]), b[off[u]: off[u + 1]].reshape(T, P[u])
        both = (au != 0.0) & (bu != 0.0)
        scaled = np.zeros(T, dtype=bool)
        for tl in tiles.get(u, ()):
            one = np.zeros(T, dtype=bool)
            one[64 * tl: 64 * tl + 64] = True
            sel = both & one[:, None]
            assert np.isfinite(au[sel]).all() and np.array_equal(au[sel], bu[sel]), f"utterance {u}: a redone cell is not the bf16×3 value"
            if 64 * tl < 128:   # (a tile of the first windows is scored whatever becomes of the utterance)
                assert sel.any(), f"utterance {u}, tile {tl}: no cell of the scaled tile was scored"
            scaled |= one
        sel = both & ~scaled[:, None]
        other_differs |= bool((au[sel] != bu[sel]).any())
    assert other_differs, "the f16 pass scored nothing: the sweep was not a redo"


@pytest.mark.parametrize("groups,grid", PLANS)
def test_redo_sweep_takes_several_trips_and_several_items_of_a_block(engine, pool, monkeypatch, groups, grid):
    """(c′) The sweep of a first-tier window reads the flags of 64 items per wavefront and trip.  144 utterances (the pool six
    times over) in windows of 128 frames are 288 items per sweep, item = 2·utterance + sub-tile: with one workgroup (per run)
    wavefront 0 reads items 0–63 and, on a second trip, 256–287.  Scaled tiles, all in the first window: items 0, 1 and 10 (three
    flagged items in one block), 80 (wavefront 1's block), 261 and 262 (two in the block of the second trip)."""
    idx = list(range(24)) * 6
    _, feats, _ = pool.batch(idx)
    feats = [x.copy() for x in feats]
    tiles = {0: [0, 1], 5: [0], 40: [0], 130: [1], 131: [0]}
    for u, tls in tiles.items():
        for tl in tls:
            feats[u][64 * tl: 64 * tl + 64] *= 1.0e4
    _, got, g, _, fo = _check(engine, pool, monkeypatch, "redo-wide", groups, grid, idx, FIRST_BEAM, RETRY_BEAM, feats=feats,
                             dense_cells=False, window=128)
    _redo_cells(engine, monkeypatch, g, feats, fo, got, tiles, 128)


@pytest.mark.parametrize("groups,grid", PLANS)
def test_epsilon_graphs_through_the_list_decoder(engine, pool, monkeypatch, groups, grid):
    """(e) The same graphs with a fifth of their arcs split by an epsilon arc: the ε instantiations, retry list of two (the
    pool's third retry utterance overflows its back-pointer table once its arcs are split)."""
    idx = _pick(pool, engine, monkeypatch, True, 2)
    dense, _, g, _, _ = _check(engine, pool, monkeypatch, "eps", groups, grid, idx, FIRST_BEAM, RETRY_BEAM, eps=True)
    assert "state_nemit" in g.tensors
    st = dense["status"].cpu().numpy()
    assert int(((st == 1) | (st == 2)).sum()) == 2 and int((st == 0).sum()) == N_UTT - 2, st.tolist()
