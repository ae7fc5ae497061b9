"""The corpus driver's software pipeline on the host: ``CorpusAligner._pass`` over several batches — graphs of batch b + 1
compiled on the worker thread into rotating staging pools while batch b is packed, launched and collected — with the
capacity redo of ``_collect`` (``engine.redo_capacity``: status 3/4 → hard bounds → general decoder, merged back by index; also
driven directly, with ``frame_like`` among the arrays) and the mixed-batch path of ``_prepare``.  The native graph compiler, the staging pools and their rotation, ``_prepare``, ``_collect`` and its merge are
the real ones; the device (features, packing, the decoders) is a scripted stub whose "alignment" of an utterance names the
utterance it was decoded for, so a graph read from a reused pool or a result merged into the wrong slot shows.

Also: ``gather_pcm`` takes any int16 sequence, and the batch cache of ``_batches`` never serves another run's batches."""
import numpy as np
import torch

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd.aligner import AlignOptions, CorpusAligner, CorpusUtterance
from montreal_forced_aligner_amd.engine import AlignmentEngine, StagingPool, StagingRing, _speaker_groups, offsets, redo_capacity
from tests import helpers

T = 50                      # frames per utterance (the stub's 160 samples per frame)
PER_BATCH = 4
N_BATCHES = 6
HARD = 1 << 20              # the stub graphs' hard bounds: how the scripted decoder tells the redo from the first decode
STAGE = {"first": 1, "hard": 2, "general": 3}
WORDS = ["this", "is", "the", "acoustic", "corpus", "talking", "pretty", "fast", "here", "nothing"]


def _key(f):
    return (int(f.start), np.asarray(f.arc_offsets, dtype=np.int64).tobytes(), np.ascontiguousarray(f.arcs).tobytes(),
            np.asarray(f.final, dtype=np.float32).tobytes())


class _Graphs:
    def __init__(self, utts):
        self.utts, self.n_utt, self.max_states = utts, len(utts), 1

    def hard_bounds(self):
        return HARD, HARD


class _Event:
    def synchronize(self):
        pass


class StubEngine:
    """Host-only stand-in for ``AlignmentEngine``: its real staging rotation over three pageable pools, packing that names
    the utterance each graph it is handed is a fresh compile of (-1: none), and decoders that answer from a script."""

    device = torch.device("cpu")
    num_ceps = 13
    needs_general_decoder = staticmethod(AlignmentEngine.needs_general_decoder)
    next_staging = AlignmentEngine.next_staging

    def __init__(self, script):
        self._staging = StagingRing(self.device, 3, pinned=False)
        self.script = script          # utterance → {stage: status} (0 where not given)
        self.expected = {}            # _key(graph) → utterance
        self.packed = []              # (pack call, [utterance per graph])
        self.calls = []               # (stage, utterance) per decoded utterance
        self.bad_rows = []            # (stage, utterance): features that are not the utterance's own

    def configure_mfcc(self, **kw):
        pass

    def load_gmm(self, am):
        pass

    def num_frames(self, n):
        return n // 160

    def _ident(self, fsts, what):
        ids = [self.expected.get(_key(f), -1) for f in fsts]
        self.packed.append((what, ids))
        return _Graphs(ids)

    def pack_graphs(self, fsts, tm, pool=None, **kw):
        pool = pool or self.next_staging()         # (as the engine does: its own next pool when none is given)
        return self._ident(fsts, "pack_graphs")

    def pack_graphs_general(self, fsts, tm):
        return self._ident(fsts, "pack_graphs_general")

    def gather_rows(self, feats, rows):
        return feats[torch.from_numpy(np.asarray(rows, dtype=np.int64))]

    def align_features(self, graphs, feats, fo, max_tokens=1024, **kw):
        return self._decode(graphs, feats, fo, "hard" if max_tokens == HARD else "first")

    def align_general(self, graphs, feats, fo, **kw):
        return self._decode(graphs, feats, fo, "general")

    def _decode(self, graphs, feats, fo, stage):
        n, total = graphs.n_utt, int(fo[-1])
        status, n_words = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ali, words, like = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(n, np.float32)
        frame_like = np.zeros(total, np.float32)
        for j, u in enumerate(graphs.utts):
            a, b = int(fo[j]), int(fo[j + 1])
            self.calls.append((stage, u))
            if u < 0 or not np.all(feats[a:b, 0].numpy() == u):
                self.bad_rows.append((stage, u))
            status[j] = self.script.get(u, {}).get(stage, 0)
            ali[a:b] = _ali_code(u, stage)
            words[a], words[a + 1], n_words[j] = u, STAGE[stage], 2
            like[j] = _like(u, stage)
            frame_like[a:b] = _frame_like(u, stage)
        return {k: torch.from_numpy(v) for k, v in dict(status=status, ali=ali, words=words, n_words=n_words, like=like,
                                                        frame_like=frame_like).items()}


def _ali_code(u, stage):
    return 1000 * STAGE[stage] + u


def _like(u, stage):
    return np.float32(-u - 0.25 * STAGE[stage])


def _frame_like(u, stage):
    return np.float32(-0.5 * u - 0.125 * STAGE[stage])


def _texts(n):
    rng = np.random.default_rng(5)
    out = set()
    while len(out) < n:
        out.add(" ".join(rng.choice(WORDS, size=3, replace=False)))
    return sorted(out)


def _feats(idx):
    return torch.from_numpy(np.repeat(np.asarray(idx, dtype=np.float32), T)[:, None])


def _fo(n):
    return np.arange(n + 1, dtype=np.int64) * T


def _wide(f):
    """The graph with 65 more copies of the start state's first arc: a state too wide for the wavefront decoder."""
    s = int(f.start)
    a0, a1 = int(f.arc_offsets[s]), int(f.arc_offsets[s + 1])
    arcs = np.concatenate([f.arcs[:a1], np.repeat(f.arcs[a0:a0 + 1], 65), f.arcs[a1:]])
    offs = np.asarray(f.arc_offsets, dtype=np.int64).copy()
    offs[s + 1:] += 65
    return K.Fst(f.start, offs, arcs, np.asarray(f.final, dtype=np.float32).copy())


def _rewrite(kind, u, f):
    return helpers.with_eps(np.random.default_rng(100 + u), f) if kind == "eps" else _wide(f)


def _setup(fx, monkeypatch, script, rewrites=None):
    """24 utterances of T frames with distinct three-word transcripts, 6 batches of 4.  ``rewrites``: utterance → "eps" (a
    graph with epsilon input arcs, still the wavefront decoder's) or "wide" (one for the general decoder) in place of what
    the compiler made — their batches take ``_prepare``'s mixed path.  Returns the aligner, its stub engine, the utterances
    and the pool-ownership log."""
    rewrites = rewrites or {}
    texts = _texts(PER_BATCH * N_BATCHES)
    utts = [CorpusUtterance(f"s{u % 3}-{u}", f"s{u % 3}", np.zeros(T * 160, dtype=np.int16), t) for u, t in enumerate(texts)]
    eng = StubEngine(script)
    al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=eng,
                       options=AlignOptions(batch_frames=PER_BATCH * T))
    u_of = {t: u for u, t in enumerate(texts)}
    for u, t in enumerate(texts):          # what each packed graph must be, bit for bit: a fresh compile of its transcript
        f = al.compiler.compile_fsts([t], al.scaled, columns=True)[0]
        eng.expected[_key(_rewrite(rewrites[u], u, f) if u in rewrites else f)] = u
    compile_fsts = al.compiler.compile_fsts

    def compile_eps(tx, *a, **kw):
        out = compile_fsts(tx, *a, **kw)
        if not any(u_of[t] in rewrites for t in tx):
            return out
        return [_rewrite(rewrites[u_of[t]], u_of[t], f) if u_of[t] in rewrites else f for t, f in zip(tx, out)]

    monkeypatch.setattr(al.compiler, "compile_fsts", compile_eps)

    def mfcc(utts_, idx):
        return list(idx), _fo(len(idx))

    def final_features(mfcc_, fo, rows, cmvn, d_lda, fmllr):
        return _feats(mfcc_)

    def launch(utts_, prep, spk_ids, cmvn, d_lda, fmllr):
        if not prep["idx"]:
            return None
        idx = prep["idx"]
        mfcc_, fo = al._mfcc(utts_, idx)
        feats = al._final_features(mfcc_, fo, None, cmvn, d_lda, fmllr)
        res = al._decode(prep["graphs"], feats, fo, al.opt.max_tokens, al.opt.bp_tokens_per_frame)
        host = {k: res[k].numpy().copy() for k in ("status", "ali", "words", "n_words", "like")}
        rows = np.array([spk_ids[utts_[i].speaker] for i in idx], dtype=np.int32)
        return dict(res=res, feats=feats, fo=fo, rows=rows, host=host, event=_Event())

    monkeypatch.setattr(al, "_mfcc", mfcc)
    monkeypatch.setattr(al, "_final_features", final_features)
    monkeypatch.setattr(al, "_launch", launch)
    own = helpers.PoolOwnership(monkeypatch, al)
    submit = al._submit_compile

    def submit_and_wait(utts_, idx_all):
        # the worker's writes land before the collection that could race them: a shared pool shows deterministically
        fut = submit(utts_, idx_all)
        fut.result()
        return fut

    monkeypatch.setattr(al, "_submit_compile", submit_and_wait)
    return al, eng, utts, own


def _final(script, u, general):
    """(stage, status) an utterance ends with, and the stages it goes through."""
    s = script.get(u, {})
    if u in general:
        return "general", s.get("general", 0), ["general"]
    stages = ["first"]
    if s.get("first", 0) in (3, 4):
        stages.append("hard")
        if s.get("hard", 0) in (3, 4):
            stages.append("general")
    return stages[-1], s.get(stages[-1], 0), stages


def _run_and_check(al, eng, utts, own, script, general=(), passes=1):
    spk_ids = {f"s{k}": k for k in range(3)}
    for p in range(passes):
        eng.calls.clear()
        al.failure_reasons = {}
        want_feats = p == 0 and passes > 1
        results, kept = al._pass(utts, spk_ids, None, None, want_feats=want_feats)
        assert len(al._batches(utts)) == N_BATCHES
        # pool ownership: no pool handed out while a batch whose graphs live in it is not collected yet
        assert own.check() == N_BATCHES * (p + 1)
        # graph contents: every graph packed — first tier, mixed batch, redo, general fallback — is its transcript's
        assert all(u >= 0 for _w, ids in eng.packed for u in ids), \
            [(w, ids) for w, ids in eng.packed if min(ids) < 0]
        assert eng.bad_rows == []
        # every utterance decoded by exactly the stages its script sends it through, and merged back into its own slot
        want_calls = sorted((st, u) for u in range(len(utts)) for st in _final(script, u, general)[2])
        assert sorted(eng.calls) == want_calls
        reasons = {}
        for u in range(len(utts)):
            stage, status, _ = _final(script, u, general)
            if status in (0, 1):
                assert results[u] is not None, u
                out, k = results[u]
                a, b = int(out.frame_off[k]), int(out.frame_off[k + 1])
                assert b - a == T
                assert np.all(out.ali[a:b] == _ali_code(u, stage)), (u, stage, out.ali[a:b][:3])
                assert int(out.n_words[k]) == 2 and list(out.words[a: a + 2]) == [u, STAGE[stage]], u
                assert out.like[k] == _like(u, stage) and int(out.status[k]) == status
            else:
                assert results[u] is None, u
                reasons[utts[u].utt_id] = _lib.status_reason(status)
        assert al.failure_reasons == reasons
        if want_feats:
            # what fMLLR statistics get: every alignment as merged, failed utterances' frames zeroed
            seen = set()
            for idx, feats, ali, fo, rows in kept:
                ali = ali.numpy()
                for k, u in enumerate(idx):
                    stage, status, _ = _final(script, u, general)
                    seg = ali[int(fo[k]): int(fo[k + 1])]
                    assert np.all(seg == (_ali_code(u, stage) if status in (0, 1) else 0)), u
                    assert np.all(feats[int(fo[k]): int(fo[k + 1]), 0].numpy() == u)
                    seen.add(u)
            assert seen == set(range(len(utts)))


def _b(batch, k):
    return batch * PER_BATCH + k


# first-decode overflows in batches 0 and 1; one goes on to the general decoder, one fails there, one fails outright
SCRIPT_CONSECUTIVE = {
    _b(0, 1): {"first": 3},
    _b(1, 0): {"first": 4, "hard": 3},
    _b(1, 2): {"first": 3},
    _b(1, 3): {"first": 2},
    _b(2, 1): {"first": 4, "hard": 4, "general": 2},
}
SCRIPT_LAST = {
    _b(5, 0): {"first": 3},
    _b(5, 2): {"first": 4, "hard": 3, "general": 1},
    _b(5, 3): {"first": 1},
}


def test_overflow_in_consecutive_batches(fx, monkeypatch):
    al, eng, utts, own = _setup(fx, monkeypatch, SCRIPT_CONSECUTIVE)
    _run_and_check(al, eng, utts, own, SCRIPT_CONSECUTIVE)


def test_overflow_in_the_last_batch_only(fx, monkeypatch):
    al, eng, utts, own = _setup(fx, monkeypatch, SCRIPT_LAST)
    _run_and_check(al, eng, utts, own, SCRIPT_LAST)


def test_mixed_batch_and_overflows(fx, monkeypatch):
    """Batches 1 and 4 are not the compiler's batch objects: a graph with epsilon input arcs (batch 1, which also overflows
    on the first decode) and one too wide for the wavefront decoder (batch 4, for ``_general``) send them down
    ``_prepare``'s mixed path, whose packing draws a pool of its own; batches 1, 2 and 4 overflow."""
    rewrites = {_b(1, 2): "eps", _b(4, 0): "wide"}
    script = {_b(1, 0): {"first": 3}, _b(1, 2): {"first": 4}, _b(2, 3): {"first": 4}, _b(4, 0): {"general": 2},
              _b(4, 1): {"first": 3, "hard": 3}}
    al, eng, utts, own = _setup(fx, monkeypatch, script, rewrites)
    _run_and_check(al, eng, utts, own, script, general=(_b(4, 0),))
    assert [ids for w, ids in eng.packed if w == "pack_graphs_general"] == [[_b(4, 0)], [_b(4, 1)]]
    assert sum(w == "pack_graphs" and _b(1, 2) in ids for w, ids in eng.packed) == 2       # first decode and redo


def test_two_passes_in_a_row(fx, monkeypatch):
    """The two-pass flow: a pass that keeps what fMLLR estimation needs, then a second pass over the same batches."""
    al, eng, utts, own = _setup(fx, monkeypatch, SCRIPT_CONSECUTIVE)
    _run_and_check(al, eng, utts, own, SCRIPT_CONSECUTIVE, passes=2)


# ------------------------------------------------------------------------------------------- the shared ladder, directly
RESULT_KEYS = ("ali", "words", "n_words", "like", "status", "frame_like")


def _ladder(fx, script, n=5):
    """One batch of ``n`` utterances of T frames through the stub's first decode, then ``redo_capacity`` on the host copy
    of its results (``frame_like`` among them).  Returns the stub, the arrays before and after, and the positions redone."""
    texts = _texts(n)
    eng = StubEngine(script)
    al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=eng)
    fsts = [al.compiler.compile_fsts([t], al.scaled, columns=True)[0] for t in texts]
    for u, f in enumerate(fsts):
        eng.expected[_key(f)] = u
    feats, fo = _feats(range(n)), _fo(n)
    first = eng._decode(_Graphs(list(range(n))), feats, fo, "first")
    host = {k: first[k].numpy().copy() for k in RESULT_KEYS}
    before = {k: v.copy() for k, v in host.items()}
    eng.calls.clear()

    def decode(graphs, f, o, max_tokens, bp_tokens_per_frame):
        assert (max_tokens, bp_tokens_per_frame) == graphs.hard_bounds()
        return eng.align_features(graphs, f, o, max_tokens=max_tokens, bp_tokens_per_frame=bp_tokens_per_frame)

    redone = redo_capacity(eng, fsts, fx.mono_tm, feats, fo, host, decode, 10.0, 40.0, 0.1)
    return eng, before, host, redone


def test_ladder_merges_every_array_of_every_stage(fx):
    """Statuses 0, 3, 4, 2, 3 at the first decode; utterance 2 still 4 with the hard bounds (on to the general decoder),
    utterance 4 fails (2) there: each utterance's ali, words[:n_words], n_words, like, status and frame_like are those of
    the last stage it went through, and utterances 0 and 3 — no capacity status — keep every byte of theirs."""
    script = {1: {"first": 3}, 2: {"first": 4, "hard": 4}, 3: {"first": 2}, 4: {"first": 3, "hard": 2}}
    eng, before, host, redone = _ladder(fx, script)
    assert redone == [1, 2, 4]
    assert sorted(eng.calls) == sorted([("hard", 1), ("hard", 2), ("hard", 4), ("general", 2)])
    assert eng.packed == [("pack_graphs", [1, 2, 4]), ("pack_graphs_general", [2])]
    assert eng.bad_rows == []
    final = {0: ("first", 0), 1: ("hard", 0), 2: ("general", 0), 3: ("first", 2), 4: ("hard", 2)}
    for u, (stage, status) in final.items():
        a, b = u * T, (u + 1) * T
        assert np.all(host["ali"][a:b] == _ali_code(u, stage)), u
        assert int(host["n_words"][u]) == 2 and list(host["words"][a: a + 2]) == [u, STAGE[stage]], u
        assert host["like"][u] == _like(u, stage) and int(host["status"][u]) == status, u
        assert np.all(host["frame_like"][a:b] == _frame_like(u, stage)), u
    for u in (0, 3):
        for k in RESULT_KEYS:
            sl = slice(u * T, (u + 1) * T) if k in ("ali", "words", "frame_like") else u
            assert np.array_equal(host[k][sl], before[k][sl]), (u, k)


def test_ladder_without_capacity_status_touches_nothing(fx):
    eng, before, host, redone = _ladder(fx, {1: {"first": 2}, 3: {"first": 1}})
    assert redone == [] and eng.packed == [] and eng.calls == []
    assert all(np.array_equal(host[k], before[k]) for k in RESULT_KEYS)


# ---------------------------------------------------------------------------------------------------------- small pieces
class _HostPool(StagingPool):
    def to_device(self, view, stream=None):
        return torch.from_numpy(view.copy())


def test_gather_pcm_takes_any_int16_sequence():
    """``CorpusUtterance.pcm`` as a list, a tensor, another dtype or a strided view: gathered like the int16 array."""
    eng = AlignmentEngine.__new__(AlignmentEngine)
    eng.lib, eng.stream = _lib.lib(), None
    rng = np.random.default_rng(3)
    base = [rng.integers(-30000, 30000, size=n).astype(np.int16) for n in (401, 1, 2000, 17, 333)]
    given = [base[0].tolist(), torch.from_numpy(base[1].copy()), base[2].astype(np.int32), np.repeat(base[3], 2)[::2], base[4]]
    out, so = eng.gather_pcm(given, pool=_HostPool(torch.device("cpu"), pinned=False))
    assert list(np.diff(so)) == [401, 1, 2000, 17, 333]
    assert np.array_equal(out.numpy(), np.concatenate(base))


def test_batches_are_never_another_runs(fx):
    """``speaker_cmvn`` called on its own leaves the batch cache set: neither a list refilled in place (same object, same
    length, other durations) nor a changed ``batch_frames`` may be served the batches it cached."""
    eng = StubEngine({})
    eng.cmvn_stats = lambda mfcc, fo, rows, n: torch.zeros((n, 2, eng.num_ceps + 1), dtype=torch.float64)
    al = CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=eng, options=AlignOptions(batch_frames=300))
    al._mfcc = lambda utts, idx: (None, _fo(len(idx)))

    def fresh(utts):
        return CorpusAligner(fx.mono_tm, fx.mono_am, fx.mono_tree, fx.mono_lex, engine=eng,
                             options=AlignOptions(batch_frames=al.opt.batch_frames))._batches(utts)

    def corpus(lengths):
        return [CorpusUtterance(f"u{k}", "s", np.zeros(n * 160, dtype=np.int16), "this is") for k, n in enumerate(lengths)]

    utts = corpus([100, 50, 200, 120, 80, 60])
    al.speaker_cmvn(utts)
    assert al._batches(utts) == fresh(utts) == [[1, 5, 4, 0], [3], [2]]
    utts[:] = corpus([200, 120, 80, 60, 100, 50])
    assert al._batches(utts) == fresh(utts) == [[5, 3, 2, 4], [1], [0]]
    al.opt.batch_frames = 1000
    assert al._batches(utts) == fresh(utts) == [[5, 3, 2, 4, 1, 0]]


def test_offsets_and_speaker_groups_are_the_expressions_they_replace():
    def same(got, want):
        assert got.dtype == want.dtype and np.array_equal(got, want), (got, want)

    for lengths in ([], [7], [3, 0, 5], np.array([4, 4, 1], dtype=np.int32), np.zeros(0, dtype=np.int64), (2, 9)):
        same(offsets(lengths), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
        same(offsets(lengths, np.int32), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))
    # empty, one utterance, speakers first seen out of order with gaps between their numbers, labels that are not numbers
    for utt2spk in (np.zeros(0, dtype=np.int32), np.array([5], dtype=np.int32), np.array([9, 2, 9, 40, 2, 2, 7], dtype=np.int32),
                    np.array([3, 3, 0], dtype=np.int64), ["zoe", "al", "zoe", "mo"]):
        spk_ids, inv, order, spk_off = _speaker_groups(utt2spk)
        want_ids, want_inv = np.unique(np.asarray(utt2spk), return_inverse=True)
        same(spk_ids, want_ids)
        same(inv, want_inv)
        same(order, np.argsort(want_inv, kind="stable").astype(np.int32))
        same(spk_off, np.concatenate([[0], np.cumsum(np.bincount(want_inv, minlength=len(want_ids)))]).astype(np.int32))
