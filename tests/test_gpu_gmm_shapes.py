"""Acoustic scoring off the tuned shapes (tests/gmm_ref.py has the cases, the float64 reference and the bound B).

Rules, wherever a case does not say otherwise:
  * a single-Gaussian column equals the C++ oracle bit for bit in every mode;
  * on the float32 kernels (MFA_GMM_BF16=0, and the plain kernel) a mixture column of a helpers.random_gmm model stays within
    4·spacing(float32(max |oracle|)) of the C++ oracle (test_gmm_real_mixture_model's bound);
  * every other mixture cell stays within B of the float64 reference;
  * no cell of a dense run is left at 0.0 (the runs here score into zero-filled buffers: engine.score's own buffer is
    uninitialised memory, in which an unwritten cell can hold an earlier launch's correct score).
Each test prints its worst err / B."""
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd.engine import offsets
from oracle import oracle as O
from tests import gmm_ref as R
from tests import helpers
from tests.test_gmm_pack_cpu import _pack
from tests.test_gpu_parity import _dev, _random_graph

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "bf16x3": {"MFA_GMM_F16": "0"}, "f32": {"MFA_GMM_BF16": "0"}}
_ENV = ("MFA_GMM_F16", "MFA_GMM_BF16", "MFA_GMM_NAIVE", "MFA_GMM_PACK_NB")


def _mode(monkeypatch, mode=None, **env):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(MODES[mode] if mode else {}, **env).items():
        monkeypatch.setenv(k, v)


def _score(engine, am, feats_list, pdf_lists):
    """tests.test_gpu_parity._score, into a zero-filled buffer."""
    engine.load_gmm(am)
    frame_off = offsets([f.shape[0] for f in feats_list])
    sorted_lists, counts = zip(*[engine.sort_pdf_list(p) for p in pdf_lists])
    pdf_off = offsets([len(p) for p in sorted_lists])
    ll_off = offsets(np.diff(frame_off) * np.diff(pdf_off))
    out = torch.zeros(int(ll_off[-1]), dtype=torch.float32, device=engine.device)
    engine._launch_score(_dev(engine, np.concatenate(feats_list).astype(np.float32)), _dev(engine, frame_off), len(feats_list),
                         int(np.diff(frame_off).max()), _dev(engine, np.concatenate(sorted_lists).astype(np.int32)),
                         _dev(engine, pdf_off), _dev(engine, np.stack(counts).astype(np.int32)), None, _dev(engine, ll_off), out)
    ll = out.cpu().numpy()
    return [ll[ll_off[u]: ll_off[u + 1]].reshape(f.shape[0], len(sorted_lists[u])) for u, f in enumerate(feats_list)], sorted_lists


_REFS = {}


def _refs(key, am, feats, sorted_lists):
    """(float64 reference, C++ oracle, B) per utterance — computed once per case and left unchanged."""
    if key not in _REFS:
        out = []
        for x, pl in zip(feats, sorted_lists):
            ref = R.ref64(x, am, pl)
            orc = O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl)
            for a in (ref, orc):
                a.setflags(write=False)
            out.append((ref, orc, R.bound(x, am, pl, ref)))
        _REFS[key] = out
    return _REFS[key]


def _check(key, am, feats, got, sorted_lists, f32_rule, what):
    """The module's rules on one run; returns the worst err / B over mixture cells."""
    n_gauss = np.diff(am.pdf_offsets)
    worst = worst_several = 0.0
    for u, (ref, orc, B) in enumerate(_refs(key, am, feats, sorted_lists)):
        g = got[u]
        assert g.shape == ref.shape
        assert np.isfinite(g).all() and (g != 0.0).all(), f"{what}, utterance {u}: {int((g == 0.0).sum())} of {g.size} cells were not written"
        single = n_gauss[sorted_lists[u]] == 1
        assert np.array_equal(g[:, single], orc[:, single]), f"{what}, utterance {u}: single-Gaussian columns differ from the oracle"
        if not (~single).any() or not g.size:
            continue
        ratio = (np.abs(g.astype(np.float64) - ref) / B)[:, ~single]
        worst = max(worst, float(ratio.max()))
        several = n_gauss[sorted_lists[u]][~single] > 32
        if several.any():
            worst_several = max(worst_several, float(ratio[:, several].max()))
        if f32_rule:
            err = float(np.abs(g[:, ~single] - orc[:, ~single]).max())
            assert err <= R.f32_rule(orc), f"{what}, utterance {u}: {err} from the oracle, float32 rule {R.f32_rule(orc)}"
        else:
            at = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert ratio.max() <= 1.0, f"{what}, utterance {u}: err / B = {ratio.max():.3f} at {at}"
    print(f"{what}: worst err / B = {worst:.4f} (pdfs of several blocks: {worst_several:.4f})")
    return worst


def _run_case(engine, monkeypatch, case, mode, what=None, **env):
    _mode(monkeypatch, mode, **env)
    got, sl = _score(engine, case.am, case.feats, case.lists)
    assert all(np.array_equal(a, b) for a, b in zip(sl, R.sorted_lists(case.am, case.lists)))
    plain = case.am.dim > 48 or env.get("MFA_GMM_NAIVE") == "1"
    _check(case.name, case.am, case.feats, got, sl, (mode == "f32" or plain) and not case.skewed,
           what or f"{case.name}, {'plain kernel' if plain else mode}")
    return got, sl


# ---- a. narrow and edge dimensions

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dim", R.DIMS_EDGE)
def test_narrow_and_edge_dimensions(engine, monkeypatch, dim, mode):
    """Padded 16-k steps with fscale 0 (dims 3 … 36), the 16-byte feature loads of dim % 8 == 0 with whole groups of padding
    (8, 16, 24), the switch from 80 to 96 operand columns (41), the last dimensions of the MFMA kernels (47, 48)."""
    _run_case(engine, monkeypatch, R.edge_case(dim), mode)


# ---- b. the plain kernel

@pytest.mark.parametrize("dim", R.DIMS_PLAIN)
def test_plain_kernel_wide_models(engine, monkeypatch, dim):
    _run_case(engine, monkeypatch, R.edge_case(dim), None)


@pytest.mark.parametrize("dim", R.DIMS_NAIVE)
def test_plain_kernel_as_cross_check(engine, monkeypatch, dim):
    """MFA_GMM_NAIVE=1 against the oracle and against the MFMA kernels."""
    case = R.edge_case(dim)
    plain, sl = _run_case(engine, monkeypatch, case, None, MFA_GMM_NAIVE="1")
    f32, _ = _run_case(engine, monkeypatch, case, "f32")
    default, _ = _run_case(engine, monkeypatch, case, "default")
    n_gauss = np.diff(case.am.pdf_offsets)
    for u in range(len(plain)):
        single = n_gauss[sl[u]] == 1
        assert np.array_equal(plain[u][:, single], f32[u][:, single]) and np.array_equal(plain[u][:, single], default[u][:, single])
        assert np.abs(plain[u] - f32[u]).max() <= R.f32_rule(f32[u])


# ---- c. more columns than pdfs

@pytest.mark.parametrize("dim,env,mode", [(52, {}, None), (39, {"MFA_GMM_NAIVE": "1"}, None), (39, {}, "default")],
                         ids=["plain-52", "naive-39", "default-39"])
def test_lists_with_repeats_longer_than_the_model(engine, monkeypatch, dim, env, mode):
    """A list is a list of columns, not of pdfs: 12 entries over a model of 5 pdfs, on the longest utterance, so that
    T_u · P_u > max_frames · num_pdfs.  Every cell is written and correct."""
    case = R.repeats_case(dim)
    T, P = np.array([f.shape[0] for f in case.feats]), np.array([len(l) for l in case.lists])
    assert (T * P).max() > T.max() * case.am.num_pdfs and P.max() == 12 and case.am.num_pdfs == 5
    _run_case(engine, monkeypatch, case, mode, **env)


# ---- d. a wide model through the product path

WIDE_TEXTS = ["this is the acoustic corpus i'm talking pretty fast here this is the acoustic corpus",
              "this is the acoustic corpus", "talking pretty fast here"]


def _walk_feats(rng, fst, tm, am):
    """Frames along a left-to-right walk of the graph: the shortest path to a final state, every arc's frame drawn close to
    the first Gaussian of the arc's pdf, with up to two frames on the self-loop of every state passed."""
    S = fst.num_states
    src = np.repeat(np.arange(S), np.diff(fst.arc_offsets))
    dst = fst.arcs["nextstate"].astype(np.int64)
    dist = np.where(np.isfinite(fst.final), 0, 1 << 30).astype(np.int64)
    for _ in range(S + 1):
        nd = dist.copy()
        np.minimum.at(nd, src, dist[dst] + 1)
        if np.array_equal(nd, dist):
            break
        dist = nd
    mean = am.means_invvars.astype(np.float64) / am.inv_vars
    dev = 1.0 / np.sqrt(am.inv_vars.astype(np.float64))

    def frame(arc):
        g = am.pdf_offsets[tm.id2pdf[fst.arcs["ilabel"][arc]]]
        return mean[g] + 0.3 * dev[g] * rng.normal(size=am.dim)

    s, out = int(fst.start), []
    while dist[s] > 0:
        arcs = np.arange(fst.arc_offsets[s], fst.arc_offsets[s + 1])
        step = arcs[(dst[arcs] != s) & (dist[dst[arcs]] == dist[s] - 1)][0]
        out.append(frame(step))
        s = int(dst[step])
        loops = np.arange(fst.arc_offsets[s], fst.arc_offsets[s + 1])
        loops = loops[dst[loops] == s]
        for _ in range(int(rng.integers(0, 3)) if loops.size else 0):
            out.append(frame(loops[0]))
    return np.asarray(out, np.float32)


@pytest.mark.parametrize("mixtures", [False, True], ids=["single-gaussians", "mixtures"])
def test_wide_model_through_the_product_path(engine, fx, monkeypatch, mixtures):
    """A 52-dimensional model (dense scoring by the plain kernel, then the decoder — mfa_align_features_batch's fallback)
    on training graphs whose default packing gives the longest utterance more columns than the model has pdfs."""
    _mode(monkeypatch)
    tm = fx.mono_tm
    am = R.wide_models(tm.num_pdfs)[int(mixtures)]
    engine.load_gmm(am)
    fsts = [fx.mono_graph(t) for t in WIDE_TEXTS]
    rng = np.random.default_rng(7700)
    feats = [_walk_feats(rng, f, tm, am) for f in fsts]
    fo = offsets([f.shape[0] for f in feats])
    graphs = engine.pack_graphs(fsts, tm)
    ll_cols = np.diff(graphs.pdf_off_host)
    assert ll_cols.max() > tm.num_pdfs, ll_cols
    T = np.diff(fo)
    assert (T * ll_cols).max() > T.max() * tm.num_pdfs and np.argmax(T) == np.argmax(ll_cols) == 0
    kw = dict(beam=100.0, retry_beam=400.0)
    res = engine.align_features(graphs, _dev(engine, np.concatenate(feats)), fo, max_tokens=2048, bp_tokens_per_frame=1024,
                                want_frame_likes=True, **kw)
    res = {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}
    unwritten = int((res["loglikes"] == 0.0).sum())
    assert unwritten == 0, f"{unwritten} of {res['loglikes'].size} cells were not written"
    for u, f in enumerate(fsts):
        ref = helpers.oracle_align_feats(tm, f, feats[u], am, **kw)
        assert ref["status"] in (0, 1)
        a, b = int(fo[u]), int(fo[u + 1])
        assert res["status"][u] == ref["status"], (u, res["status"][u], ref["status"])
        assert np.array_equal(res["ali"][a:b], ref["ali"]), f"utterance {u}: alignment differs from the oracle's"
        if mixtures:
            assert abs(float(res["like"][u]) - ref["like"]) / (b - a) < 1e-3
        else:      # single Gaussians: the scores are the oracle's bit for bit, and so is everything the decoder makes of them
            assert np.array_equal(res["words"][a: a + int(res["n_words"][u])], ref["words"])
            assert res["like"][u] == np.float32(ref["like"]), (res["like"][u], ref["like"])
            assert np.array_equal(res["frame_like"][a:b], ref["per_frame"])


# ---- lazy against dense (e, f, g)

def _toy_tm(num_pdfs):
    """What _random_graph and pack_graphs read of a transition model, over the pdfs of a small synthetic model."""
    n = 3 * num_pdfs
    return types.SimpleNamespace(num_transition_ids=n, num_pdfs=num_pdfs,
                                 id2pdf=np.concatenate([[-1], np.arange(n) % num_pdfs]).astype(np.int32))


def _lazy_vs_dense(engine, graphs, am, feats, d_feats, fo, exact_outputs, what, **kw):
    """_both of tests/test_gpu_lazy.py with the exception test_lazy_random_graphs_all_slot_classes makes: a column of a pdf
    of several blocks, merged by the two paths with different block schedules, agrees to 1e-4·scale; every other lazily
    written cell is the dense cell bit for bit — and, like every mixture cell, within B of the float64 reference.  Returns
    (dense matrices, lazily written masks) per utterance."""
    ll, ll_off, ll_cols = engine.score(d_feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts)
    dense = engine.align(graphs, ll, ll_off, ll_cols, fo, want_frame_likes=True, **kw)
    lazy = engine.align_features(graphs, d_feats, fo, want_frame_likes=True, **kw)
    torch.cuda.synchronize()
    d, s = ll.cpu().numpy(), lazy["loglikes"].cpu().numpy()
    cc, P = graphs.class_counts.cpu().numpy(), np.diff(graphs.pdf_off_host)
    mats, masks, exact_cells, written, cells, worst = [], [], 0, 0, 0, 0.0
    for u in range(graphs.n_utt):
        T = int(fo[u + 1] - fo[u])
        du, su = d[ll_off[u]: ll_off[u + 1]].reshape(T, P[u]), s[ll_off[u]: ll_off[u + 1]].reshape(T, P[u])
        multi = np.zeros(P[u], bool)
        multi[cc[u, 0]: cc[u, 0] + cc[u, 1]] = True
        w = su != 0.0
        if exact_outputs:
            multi[:] = False
        bad = w[:, ~multi] & (du[:, ~multi] != su[:, ~multi])
        assert not bad.any(), f"utterance {u}: {int(bad.sum())} lazily scored cells differ from the dense kernel's, first at frame {np.argwhere(bad)[0][0]}"
        exact_cells += int(w[:, ~multi].sum())
        if w[:, multi].any():
            a_, b_ = du[:, multi][w[:, multi]], su[:, multi][w[:, multi]]
            assert np.abs(a_ - b_).max() <= 1e-4 * max(1.0, float(np.abs(a_).max()))
            pl = graphs.pdf_lists_host[u][multi]
            ref = R.ref64(feats[u], am, pl)
            ratio = (np.abs(su[:, multi].astype(np.float64) - ref) / R.bound(feats[u], am, pl, ref))[w[:, multi]]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"utterance {u}: a lazily scored cell of a pdf of several blocks is {ratio.max():.3f} B off"
        mats.append(du); masks.append(w)
        written += int(w.sum()); cells += w.size
    assert exact_cells > 0
    print(f"{what}: lazy scoring wrote {written / cells:.2f} of the cells, {exact_cells} of them the dense kernels' bits; "
          f"pdfs of several blocks: worst err / B = {worst:.4f}")
    same = 0
    for u in range(graphs.n_utt):
        a, b = int(fo[u]), int(fo[u + 1])
        if int(dense["status"][u]) == int(lazy["status"][u]) and torch.equal(dense["ali"][a:b], lazy["ali"][a:b]):
            same += 1
            if int(dense["status"][u]) in (0, 1):
                assert abs(float(dense["like"][u]) - float(lazy["like"][u])) / (b - a) < 1e-3
    if exact_outputs:
        for k in ("status", "ali", "words", "n_words", "like", "frame_like"):
            assert torch.equal(dense[k], lazy[k]), f"{k} differs between lazy and dense scoring"
    else:
        assert same >= graphs.n_utt - 1
    return mats, masks


def _graph_batch(engine, rng, am, feats, states=(8, 40, 150)):
    tm = _toy_tm(am.num_pdfs)
    engine.load_gmm(am)
    fsts = [_random_graph(rng, tm, int(rng.choice(states))) for _ in feats]
    return engine.pack_graphs(fsts, tm), _dev(engine, np.concatenate(feats)), offsets([f.shape[0] for f in feats])


_LAZY_KW = dict(beam=1.0e4, retry_beam=0.0, max_tokens=2048, bp_tokens_per_frame=1100, acoustic_scale=0.1)


def _lazy_all_ways(engine, monkeypatch, am, feats, seed, what):
    """Lazy against dense on random graphs: all on the float32 kernels (everything bit for bit), then the default arithmetic."""
    rng = np.random.default_rng(seed)
    _mode(monkeypatch, "f32")
    graphs, d_feats, fo = _graph_batch(engine, rng, am, feats)
    _lazy_vs_dense(engine, graphs, am, feats, d_feats, fo, True, f"{what}, f32", **_LAZY_KW)
    _mode(monkeypatch, "default")
    _lazy_vs_dense(engine, graphs, am, feats, d_feats, fo, False, f"{what}, default", **_LAZY_KW)


# ---- e. skewed models

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dim", R.DIMS_SKEWED)
def test_skewed_models_dense(engine, monkeypatch, dim, mode):
    """Columns whose scales spread over eight decades of inv_var, a component under the cutoff and a tie in the maximum in
    every larger pdf, frames from the model's own Gaussians: every mode within B of the float64 reference."""
    _run_case(engine, monkeypatch, R.skewed_case(dim), mode)


@pytest.mark.parametrize("dim", R.DIMS_SKEWED)
def test_skewed_models_lazy_equals_dense(engine, monkeypatch, dim):
    case = R.skewed_case(dim)
    _lazy_all_ways(engine, monkeypatch, case.am, case.feats, 7800 + dim, case.name)


# ---- f. pdfs of more than 1 024 Gaussians

@pytest.mark.parametrize("mode", list(MODES))
def test_pdfs_of_more_than_1024_gaussians_dense(engine, monkeypatch, mode):
    case = R.huge_case()
    assert _pack(case.am)["max_nblk"] >= 33          # the block count does not fit the five low bits of a column's row word
    _run_case(engine, monkeypatch, case, mode)


def test_pdfs_of_more_than_1024_gaussians_lazy_equals_dense(engine, monkeypatch):
    case = R.huge_case()
    _lazy_all_ways(engine, monkeypatch, case.am, case.feats, 7900, case.name)


# ---- g. the f16 range edge

@lru_cache(maxsize=None)
def _range_fscale():
    return _pack(R.range_case().am)["fscale"]


def _range_base(engine, monkeypatch):
    """The default run on the unmodified features (scored once)."""
    if "base" not in _REFS:
        case = R.range_case()
        _mode(monkeypatch, "default")
        _REFS["base"] = _score(engine, case.am, case.feats, case.lists)[0]
    return _REFS["base"]


@pytest.mark.parametrize("name,k,target,declined", R.RANGE_VARIANTS, ids=[v[0].replace(" ", "-") for v in R.RANGE_VARIANTS])
def test_f16_range_edge_dense(engine, monkeypatch, name, k, target, declined):
    """One scaled operand of frame 300 at 64 990: its 256-frame tile stays on the f16 pass, within B.  At 65 010: the tile is
    the bf16×3 pass's, bit for bit.  (A plain operand that large has a squared operand far out of range: declined on both
    sides, see gmm_ref.RANGE_VARIANTS.)  Every other tile is untouched either way."""
    case = R.range_case()
    range_base = _range_base(engine, monkeypatch)
    feats = R.range_feats(case, _range_fscale(), k, target)
    _mode(monkeypatch, "bf16x3")
    bf16, sl = _score(engine, case.am, feats, case.lists)
    _mode(monkeypatch, "default")
    got, _ = _score(engine, case.am, feats, case.lists)
    _check(f"{case.name} {name}", case.am, feats, got, sl, False, f"{case.name}, {name}")
    mix = np.diff(case.am.pdf_offsets)[sl[0]] > 1
    tile = slice(256, 512)
    if declined:
        assert np.array_equal(got[0][tile], bf16[0][tile])
    else:
        assert (got[0][tile][:, mix] != bf16[0][tile][:, mix]).any()       # the f16 pass kept the tile
    keep = np.r_[0:256, 512:700]
    assert np.array_equal(got[0][keep], range_base[0][keep]) and np.array_equal(got[1], range_base[1])
    assert (got[0][keep][:, mix] != bf16[0][keep][:, mix]).any()           # … which the f16 pass scored


@pytest.mark.parametrize("name,k,target,declined", R.RANGE_VARIANTS, ids=[v[0].replace(" ", "-") for v in R.RANGE_VARIANTS])
def test_f16_range_edge_lazy_equals_dense(engine, monkeypatch, name, k, target, declined):
    """The same frames through align_features, which splits the features in a kernel of its own and keeps its own range
    flags: whatever it writes is the dense run's cell, in the tile of frame 300 too."""
    case = R.range_case()
    feats = R.range_feats(case, _range_fscale(), k, target)
    _mode(monkeypatch, "default")
    graphs, d_feats, fo = _graph_batch(engine, np.random.default_rng(8000), case.am, feats, states=(40,))
    mats, masks = _lazy_vs_dense(engine, graphs, case.am, feats, d_feats, fo, False, f"{case.name}, {name}", **_LAZY_KW)
    for sub in range(256, 512, 64):                                         # every 64-frame sub-tile of the tile was visited
        assert masks[0][sub: sub + 64].any()


# ---- h. more items than workgroups

@pytest.mark.parametrize("mode", ["default", "f32"])
def test_more_items_than_workgroups(engine, monkeypatch, mode):
    """700 short utterances in one launch: the workgroups pop more (utterance, tile) items than there are workgroups.  Every
    cell is correct, and twenty of the utterances scored alone give the same bits."""
    case = R.many_case()
    got, sl = _run_case(engine, monkeypatch, case, mode)
    pick = np.random.default_rng(8100).choice(R.N_MANY, size=R.MANY_ALONE, replace=False)
    for u in pick:
        alone, _ = _score(engine, case.am, [case.feats[u]], [case.lists[u]])
        assert np.array_equal(alone[0], got[u]), f"utterance {u} scored alone differs"
