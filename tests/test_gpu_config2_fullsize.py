"""BASELINE configs[2] at its REAL size against the oracle: the bench's own model
(`synth.train_triphone` defaults: 4 960 pdfs × 32 Gaussians, D = 40, 51 MB of operands), per-speaker CMVN + fMLLR, beam 10 /
retry 40, and the bench's own batch — the 4 096 distinct 10 s utterances of rank 0 — through the DEFAULT product path:
`align_features` with grouped score plans (pdf id mod 8 runs of ≈60 columns), the ≤ 2 048-column bitmap, the speculative
48-arc look-ahead, the 64-token first tier with its lag-mode redo, and the retry-beam list pass.

Size-independent properties on all 4 096: status ∈ {0, 1}; one transition-id per frame; the alignment splits into complete
phones that some choice of the transcript's pronunciations spells; word ids = transcript; a second run is bit-identical.
Oracle, whole path from PCM (its own MFCC, per-speaker CMVN, splice+LDA+fMLLR, Kaldi's lazy decodable, FasterDecoder), on
six utterances — every utterance of the batch that needed the retry beam (up to three) plus the first ones that did not:
frame-identical alignment, identical words, per-frame |Δ log-likelihood| < 1e-3."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import ctm as C
from montreal_forced_aligner_amd import graph as G
from oracle import oracle as O
from tests import helpers, synth

pytestmark = pytest.mark.gpu

N_UTT = 4096
N_SPK = 1000


def test_headline_model_and_batch_against_the_oracle(engine):
    world = synth.SynthWorld.build()
    engine.configure_mfcc()
    dev = engine.device
    lda = synth.seeded_lda()
    fm = synth.seeded_fmllr(N_SPK)
    d_lda = torch.from_numpy(lda).to(dev)

    def device_features(pcm_list, spks):           # bench.py's device_features: per-utterance CMVN for the trainer
        so = np.concatenate([[0], np.cumsum([len(p) for p in pcm_list])]).astype(np.int64)
        mfcc, fo = engine.mfcc(torch.from_numpy(np.concatenate(pcm_list)).to(dev), so)
        u2s = np.arange(len(pcm_list), dtype=np.int32)
        st = engine.cmvn_stats(mfcc, fo, u2s, len(pcm_list))
        f = engine.features(mfcc, fo, u2s, st, lda=d_lda, fmllr=torch.from_numpy(fm[np.asarray(spks) % N_SPK]).to(dev))
        return f, fo

    model = synth.train_triphone(world, lambda pcm, spk: device_features([pcm], [spk])[0].cpu().numpy(), n_train=120)
    am, tm = model.am, model.tm
    assert am.num_pdfs == 4960 and am.num_gauss == 4960 * 32 and am.dim == 40
    engine.load_gmm(am)

    utts = [world.utterance(i) for i in range(N_UTT)]                    # bench.py rank 0: ids 0 .. 4095
    compiler = G.TrainingGraphCompiler(tm, model.tree, world.lexicon)
    scaled = tm.scaled_log_probs(1.0, 0.1)
    fsts = compiler.compile_fsts([u[1] for u in utts], scaled)           # native batch compiler
    graphs = engine.pack_graphs(fsts, tm)                                # grouped plans (8 runs), depth-clustered columns
    assert graphs.groups == 8 and int(np.diff(graphs.pdf_off_host).max()) <= 2048

    spk = np.array([u[3] for u in utts], dtype=np.int64)
    ids, inv = np.unique(spk, return_inverse=True)
    pcm = torch.from_numpy(np.concatenate([u[0] for u in utts])).to(dev)
    so = np.arange(N_UTT + 1, dtype=np.int64) * synth.UTT_SAMPLES
    mfcc, fo = engine.mfcc(pcm, so)
    stats = engine.cmvn_stats(mfcc, fo, inv.astype(np.int32), len(ids))            # per-speaker CMVN over the batch
    feats = engine.features(mfcc, fo, inv.astype(np.int32), stats, lda=d_lda, fmllr=torch.from_numpy(fm[ids % N_SPK]).to(dev))
    del pcm, mfcc

    def run():
        r = engine.align_features(graphs, feats, fo, beam=10.0, retry_beam=40.0, max_tokens=256, bp_tokens_per_frame=128)
        out = {k: r[k].cpu().numpy() for k in ("ali", "words", "n_words", "like", "status")}
        del r
        torch.cuda.empty_cache()
        return out

    r1 = run()
    status = r1["status"]
    assert np.all((status == 0) | (status == 1)), dict(zip(*np.unique(status, return_counts=True)))
    assert np.all(r1["ali"] > 0)
    pt, wt = world.lexicon.phone_table, world.lexicon.word_table
    for u in range(N_UTT):
        a, b = int(fo[u]), int(fo[u + 1])
        assert b - a == 1000
        words = r1["words"][a: a + int(r1["n_words"][u])]
        assert [wt.find(int(w)) for w in words] == utts[u][1].split(), u
        ivs = C.generate_ctm(r1["ali"][a:b], tm, pt, 0.01)               # raises unless a sequence of complete phones
        assert ivs[0].begin == 0.0 and ivs[-1].end == 10.0
        C.phones_to_pronunciations(world.lexicon, words, ivs)            # raises unless the transcript spells the phones
    r2 = run()
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), f"second run differs in {k}"

    retried = [int(u) for u in np.flatnonzero(status == 1)]
    print(f"retry-beam utterances of the batch: {retried}")
    picks = retried[:3] + [u for u in range(N_UTT) if status[u] == 0][: 6 - min(3, len(retried))]
    worst = 0.0
    for u in picks:
        # the oracle's own features: MFCC of every utterance of the speaker (for its CMVN), then splice + LDA + fMLLR
        mates = [v for v in range(N_UTT) if spk[v] == spk[u]]
        mf = {v: O.mfcc(utts[v][0].astype(np.float32), O.default_mfcc_opts()) for v in mates}
        cm = O.cmvn_stats([mf[v] for v in mates])
        x = O.affine(O.affine(O.splice(O.cmvn_apply(cm, mf[u])), lda), fm[spk[u] % N_SPK])
        ref = helpers.oracle_align_feats(tm, fsts[u], x, am, beam=10.0, retry_beam=40.0)
        a, b = int(fo[u]), int(fo[u + 1])
        assert ref["status"] == status[u], (u, ref["status"], status[u])
        assert np.array_equal(r1["ali"][a:b], ref["ali"]), f"utterance {u}: boundaries differ from the oracle"
        assert np.array_equal(r1["words"][a: a + int(r1["n_words"][u])], ref["words"])
        worst = max(worst, abs(float(r1["like"][u]) - ref["like"]) / (b - a))
        print(f"utterance {u}: status {status[u]}, oracle evaluated {ref['cells']} score cells "
              f"({ref['cells'] / (1000 * am.num_pdfs):.4f} of T x P_model)")
    assert worst < 1e-3, worst
