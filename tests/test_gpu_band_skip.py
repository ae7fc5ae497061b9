"""gmm_band_kernel's class-0 column mask: inside a run's index range it scores a column only if the column's own last depth
reaches the band's lower bound, and a pdf that sits twice in one 32-column staging window once (the repeat gets the first
occurrence's staged scores).  Nothing the decoder reads may change, and both skips must really be on.

Every case is built on the host first — features from the oracle's front end, the plan arrays of
mfa_build_score_plan_grouped, the oracle decoder's per-frame token depths (``frame_band``), as tools/band_study.py does — and
its preconditions (a skipped column exists, a pdf sits twice / three times in a range, a first occurrence at staged column 31,
ranges beyond 32 and 64 columns) are asserted there, so that no case can pass vacuously.  Then, per case and for the f16×2
and the bf16×3 kernel:
  (i)   every written lazy cell carries the dense kernel's bits (``_both`` of test_gpu_lazy.py),
  (ii)  alignments, words, likelihood and status equal the dense path's exactly and the oracle's,
  (iii) the oracle's decoder reads no cell that was not written: decoding the lazy matrix with every unwritten cell poisoned
        (+1e30, a score no path could refuse) gives what decoding the dense matrix gives — per (frame, pdf), the oracle's
        unit; per (frame, column) it is the device decoder that would read a skipped cell's zero, and (ii) compares it,
  (iv)  economy: in a window whose speculation held, the class-0 columns with a written cell are at most the columns the
        own-interval rule predicts; over the case they are fewer than the index ranges hold.
A repeat column is written (it receives the copy), so written cells cannot show that a pdf was scored once: for case B the
host asserts that the predicted blocks (one per pdf and staging window) are fewer than the own-interval columns, and the
device side that every own-interval column — repeats included — is written with the dense kernel's bits."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import graph as G
from oracle import oracle as O
from tests import helpers, synth
from tests.test_band_skip_rule_cpu import own_last_depths
from tests.test_gpu_lazy import _both
from tests.test_score_plan_cpu import _plan

pytestmark = pytest.mark.gpu

K = 64
SR = 16000
KW = dict(retry_beam=40.0, max_tokens=1024, bp_tokens_per_frame=256)


class Setup:
    """World, model (trained on the oracle's features: the host can then decode every case by itself), transforms."""

    def __init__(self):
        self.world = synth.SynthWorld.build()
        self.lda, self.fm = synth.seeded_lda(), synth.seeded_fmllr(8)
        self.model = synth.train_triphone(self.world, self.feats, n_train=24, n_gauss=32, n_classes=2)
        self.gc = G.TrainingGraphCompiler(self.model.tm, self.model.tree, self.world.lexicon)
        self.scaled = self.model.tm.scaled_log_probs(1.0, 0.1)
        am = self.model.am
        assert np.all(np.diff(am.pdf_offsets) == 32)              # every pdf one 32-row block: slot class 0
        self.pdf_class = np.zeros(am.num_pdfs, np.int32)

    def feats(self, pcm, spk):
        mf = O.mfcc(pcm.astype(np.float32), O.default_mfcc_opts())
        return O.affine(O.affine(O.splice(O.cmvn_apply(O.cmvn_stats([mf]), mf)), self.lda), self.fm[spk % 8])

    def speak(self, words, frames, seed):
        """Audio of `frames` frames for the given words (first pronunciation each, a short pause after every third word),
        as SynthWorld.utterance lays it out, and the words that fitted."""
        w = self.world
        rng = np.random.default_rng(seed)
        voice = seed % w.bank.shape[0]
        n_sil = w.phone_index["sil"]
        samples = 160 * frames
        body = samples - int(0.1 * SR)
        seq, kept, used = [("sil", int(0.1 * SR))], [], int(0.1 * SR)
        for i, word in enumerate(words):
            part = [(ph, int(0.03 * SR) + int(rng.geometric(1.0 / (0.03 * SR))))
                    for ph in w.lexicon.word_pronunciations(word)[0].pronunciation.split()]
            if i % 3 == 2:
                part.append(("sil", int(0.05 * SR)))
            if used + sum(d for _, d in part) > body:
                break
            seq += part; kept.append(word); used += sum(d for _, d in part)
        out = np.zeros(samples, np.float32)
        pos = 0
        for ph, dur in seq:
            out[pos: pos + dur] = w.bank[voice, w.phone_index[ph], (int(rng.integers(0, SR - 1)) + np.arange(dur)) % SR]
            pos += dur
        out += w.bank[voice, n_sil, (np.arange(samples) + 777) % SR]
        return np.clip(out * 3276.8, -32768, 32767).astype(np.int16), kept

    def n_phones(self, word):
        return len(self.world.lexicon.word_pronunciations(word)[0].pronunciation.split())


@pytest.fixture(scope="module")
def setup():
    return Setup()


def predict(s, fst, x, groups, look, beam):
    """Host prediction for one utterance: the oracle's lazy decoder (first beam) with per-frame token depths against the plan.
    Per window: the class-0 columns inside the runs' index ranges, those passing the own-interval test, the blocks the
    kernel visits (one per pdf and 32-column staging window), whether the speculation holds, and the shapes met."""
    tm, am = s.model.tm, s.model.am
    pdf_of_arc = tm.id2pdf[fst.arcs["ilabel"]].astype(np.int32)
    sd, col, cp, cf, cl, cc, gc = _plan(fst, pdf_of_arc, s.pdf_class, 32, groups)
    own = own_last_depths(fst, col, sd, len(cp))
    r = O.align_feats(fst.num_states, fst.start, fst.arc_offsets, fst.arcs, fst.final, x, am.gconsts, am.means_invvars,
                      am.inv_vars, am.pdf_offsets, tm.id2pdf, 0.1, beam, 40.0, state_depth=sd)
    fb, T = r["frame_band"], x.shape[0]
    bounds = np.concatenate([[0], np.cumsum(gc)])
    wins = []
    lagging = False       # after a failed speculation the utterance stays one window behind, on the proven band, to its end
    for t0 in range(0, T, K):
        lo, dmax = (0, 0) if t0 == 0 else (int(fb[t0, 0]), int(fb[t0, 1]))
        hi = dmax + (K - 1 if lagging else look)
        held = int(fb[t0: min(T, t0 + K), 1].max()) + 1 <= hi or look >= K - 1 or lagging
        lagging = lagging or not held
        w = dict(t0=t0, held=held, in_range=set(), needed=set(), blocks=0, skipped=0, twice=0, thrice=0, first_at_31=0, longest=0)
        for k in range(len(gc)):
            a = bounds[k] + int((cl[bounds[k]: bounds[k + 1]] < lo).sum())
            b = bounds[k] + int((cf[bounds[k]: bounds[k + 1]] <= hi).sum())
            a = min(a, b)
            w["longest"] = max(w["longest"], b - a)
            w["in_range"].update(range(a, b))
            need = [c for c in range(a, b) if own[c] >= lo]
            w["needed"].update(need)
            w["skipped"] += (b - a) - len(need)
            pdfs = [int(cp[c]) for c in need]
            w["twice"] += int(any(pdfs.count(q) >= 2 for q in set(pdfs)))
            w["thrice"] += int(any(pdfs.count(q) >= 3 for q in set(pdfs)))
            for j0 in range(a, b, 32):                              # staging windows of the kernel's walk
                seen = {}
                for c in range(j0, min(b, j0 + 32)):
                    if own[c] >= lo and int(cp[c]) not in seen:
                        seen[int(cp[c])] = c
                w["blocks"] += len(seen)
                if j0 + 31 in seen.values() and any(int(cp[c]) == int(cp[j0 + 31]) and own[c] >= lo for c in range(j0 + 32, b)):
                    w["first_at_31"] += 1
        wins.append(w)
    return dict(status=r["status"], wins=wins, n0=int(cc[0]), tokens=int(fb[:, 2].max()), cp=cp, cf=cf, cl=cl, gc=gc)


def build_case(s, texts, frames, groups, look, beam, unspoken=None):
    """``unspoken``: {utterance: words} added to its transcript and not to its audio."""
    spoken = [s.speak(t, T, 9000 + 13 * i) for i, (t, T) in enumerate(zip(texts, frames))]
    fsts = [G.add_transition_probs(s.gc.compile_fst(" ".join(kept + (unspoken or {}).get(i, []))), s.scaled)
            for i, (_, kept) in enumerate(spoken)]
    xs = [s.feats(pcm, 0) for pcm, _ in spoken]
    assert [x.shape[0] for x in xs] == list(frames)
    preds = [predict(s, f, x, groups, look, beam) for f, x in zip(fsts, xs)]
    return dict(fsts=fsts, xs=xs, preds=preds, groups=groups, look=look, beam=beam)


def total(case, key, only_held=False):
    return sum((len(w[key]) if isinstance(w[key], set) else w[key]) for p in case["preds"] for w in p["wins"]
               if w["held"] or not only_held)


def run_case(engine, s, case, monkeypatch):
    """(i)–(iv) on the device, default arithmetic and bf16×3."""
    engine.load_gmm(s.model.am)
    assert np.array_equal(np.asarray(engine.slot_class), s.pdf_class)
    fsts, xs, preds = case["fsts"], case["xs"], case["preds"]
    graphs = engine.pack_graphs(fsts, s.model.tm, groups=case["groups"])
    fo = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)
    feats = torch.from_numpy(np.concatenate(xs).astype(np.float32)).to(engine.device)
    # the device plan is the host's
    for u, p in enumerate(preds):
        assert np.array_equal(graphs.pdf_lists_host[u], p["cp"])
    cl_dev = graphs.pdf_last_depth.cpu().numpy()
    assert np.array_equal(cl_dev, np.concatenate([p["cl"] for p in preds]))
    monkeypatch.setenv("MFA_LAZY_LOOKAHEAD", str(case["look"]))
    tm, am = s.model.tm, s.model.am
    for f16 in ("1", "0"):
        monkeypatch.setenv("MFA_GMM_F16", f16)
        dense, lazy, _ = _both(engine, graphs, feats, fo, beam=case["beam"], **KW)          # (i), (ii) dense
        s_ll = lazy["loglikes"].cpu().numpy()
        ll_dense, ll_off, _ = engine.score(feats, fo, graphs.pdf_list, graphs.pdf_off_host, graphs.class_counts)
        d_ll = ll_dense.cpu().numpy()
        res = {k: v.cpu().numpy() for k, v in lazy.items() if isinstance(v, torch.Tensor)}
        wrote_all = wrote_held = 0
        for u, (fst, x, p) in enumerate(zip(fsts, xs, preds)):
            T, P = x.shape[0], len(p["cp"])
            a, b = int(fo[u]), int(fo[u + 1])
            su = s_ll[ll_off[u]: ll_off[u + 1]].reshape(T, P)
            du = d_ll[ll_off[u]: ll_off[u + 1]].reshape(T, P)
            pl = graphs.pdf_lists_host[u]
            # (ii) the oracle, from the features
            ref = helpers.oracle_align(tm, fst, O.gmm_loglikes(x, am.gconsts, am.means_invvars, am.inv_vars, am.pdf_offsets, pl),
                                       pl, beam=case["beam"], retry_beam=40.0)
            assert res["status"][u] == ref["status"] == p["status"]
            # (iii) the oracle's decoder on the device's scores, unwritten cells poisoned, vs the dense matrix.  The oracle
            # knows pdfs, not columns: a (frame, pdf) cell takes the value of whichever of the pdf's columns was written
            # (written columns of one pdf carry the same bits, (i)) and the poison if none was.
            upl, inv = np.unique(pl, return_inverse=True)
            dense_pdf = np.zeros((T, len(upl)), np.float32)
            dense_pdf[:, inv] = du
            lazy_pdf = np.full((T, len(upl)), np.float32(1e30))
            for c in range(P):
                wr = su[:, c] != 0.0
                lazy_pdf[wr, inv[c]] = su[wr, c]
            on_dense = helpers.oracle_align(tm, fst, dense_pdf, upl, beam=case["beam"], retry_beam=40.0)
            on_lazy = helpers.oracle_align(tm, fst, lazy_pdf, upl, beam=case["beam"], retry_beam=40.0)
            assert on_lazy["status"] == on_dense["status"] == ref["status"]
            if ref["status"] in (0, 1):                          # (2: both beams failed — there is no path to compare)
                assert np.array_equal(res["ali"][a:b], ref["ali"])
                assert np.array_equal(res["words"][a: a + int(res["n_words"][u])], ref["words"])
                assert abs(float(res["like"][u]) - ref["like"]) / T < 1e-3
                assert on_lazy["like"] == on_dense["like"]
                assert np.array_equal(on_lazy["ali"], on_dense["ali"]) and np.array_equal(on_lazy["words"], on_dense["words"])
            # (iv) per window whose speculation held (first tier, first beam, tables not outgrown)
            if p["status"] != 0 or p["tokens"] > 48:
                continue
            for w in p["wins"]:
                t0 = w["t0"]
                cols = set(np.nonzero((su[t0: t0 + K, : p["n0"]] != 0.0).any(axis=0))[0].tolist())
                print(f"f16={f16} utt {u} t0 {t0}: written {len(cols)} needed {len(w['needed'])} in range {len(w['in_range'])} held {w['held']}")
                if w["held"]:
                    assert cols <= w["needed"], sorted(cols - w["needed"])
                    assert len(cols) <= len(w["needed"])
                    wrote_held += len(cols)
                wrote_all += len(cols)
        held_range = sum(len(w["in_range"]) for p in preds if p["status"] == 0 and p["tokens"] <= 48 for w in p["wins"] if w["held"])
        assert 0 < wrote_held < held_range, (wrote_held, held_range)
    monkeypatch.delenv("MFA_GMM_F16")
    monkeypatch.delenv("MFA_LAZY_LOOKAHEAD")


def words_of(s, seed, n):
    rng = np.random.default_rng(seed)
    return [s.world.words[int(i)] for i in rng.integers(0, len(s.world.words), n)]


def repeating(s, seed, phones_lo=11, phones_hi=13, times=4):
    """A phrase of 11–13 phones said `times` times: every word comes back 33–41 graph depths later — past the column
    cluster span of 32, so its pdfs get a second column in the same run."""
    rng = np.random.default_rng(seed)
    while True:
        phrase = [s.world.words[int(i)] for i in rng.integers(0, len(s.world.words), 3)]
        if phones_lo <= sum(s.n_phones(w) for w in phrase) <= phones_hi:
            return phrase * times


def case_a(s):
    texts = [words_of(s, 100 + i, 20) for i in range(6)]
    return build_case(s, texts, [70, 129, 200, 257, 290, 300], groups=8, look=32, beam=10.0)


def case_b(s):
    texts = [repeating(s, 200 + i, times=8) for i in range(4)]
    return build_case(s, texts, [130, 193, 257, 300], groups=8, look=32, beam=10.0)


def case_b3(s):
    """The proven band (look-ahead 63) over eight runs: ranges deep enough to hold a pdf three times, short enough for all
    three to sit in one staging window."""
    texts = [repeating(s, 300 + i, phones_lo=11, phones_hi=12, times=8) for i in range(4)]
    return build_case(s, texts, [257, 300, 290, 270], groups=8, look=63, beam=10.0)


C_BEAM = 1.0


def case_c(s):
    """One run and the proven band: ranges of several staging windows, a first occurrence at staged column 31 whose repeat
    falls into a later staging window (scored again there).  A small first beam; utterance 2's transcript has thirty words its
    audio has not, so its first pass fails and the retry-beam pass runs over it (this model's linear graphs never fail the
    first beam and pass the second: the pass ends in the failure status, having scored its windows all the same)."""
    texts = [words_of(s, 400, 20), repeating(s, 401, times=8), words_of(s, 402, 20), repeating(s, 403, phones_lo=11, phones_hi=11, times=8)]
    return build_case(s, texts, [129, 257, 193, 300], groups=1, look=63, beam=C_BEAM, unspoken={2: words_of(s, 499, 30)})


def test_case_a_columns_below_the_band_are_skipped(engine, setup, monkeypatch):
    case = case_a(setup)
    assert total(case, "skipped", only_held=True) > 0                # a column inside a run's range with own_last < lo
    run_case(engine, setup, case, monkeypatch)


def test_case_b_repeated_pdfs_are_scored_once_per_staging_window(engine, setup, monkeypatch):
    case = case_b(setup)
    assert total(case, "twice") > 0                                  # some run's range holds a pdf twice
    assert total(case, "blocks") < total(case, "needed")             # … and the walk visits fewer blocks than needed columns
    run_case(engine, setup, case, monkeypatch)


def test_case_b_three_occurrences_in_one_range(engine, setup, monkeypatch):
    case = case_b3(setup)
    assert total(case, "thrice") > 0
    assert total(case, "blocks") < total(case, "needed")
    run_case(engine, setup, case, monkeypatch)


def test_case_c_long_ranges_last_tile_of_one_frame_and_retry_pass(engine, setup, monkeypatch):
    case = case_c(setup)
    longest = max(w["longest"] for p in case["preds"] for w in p["wins"])
    assert longest > 64                                              # more than two staging windows in one range
    assert any(32 < w["longest"] <= 64 for p in case["preds"] for w in p["wins"])
    assert any(x.shape[0] % 64 == 1 for x in case["xs"])             # a last tile of one frame
    assert total(case, "first_at_31") > 0                            # a first occurrence in the last staged column, repeat later
    assert [p["status"] for p in case["preds"]] == [0, 0, 2, 0]      # utterance 2: the retry-beam pass (strided grid, 32-column chunks)
    run_case(engine, setup, case, monkeypatch)
