"""``IvectorTrainer`` on the device end to end at G = 8, D = 13, R = 6 over 40 short utterances drawn from a known extractor: the
resident statistics against the longdouble restatement, at every iteration the device's E-step for the device's current model
against the host twin's and the accumulators against the longdouble sums (the bounds of tests/ivector_ref.py), ``final.ie``
written and reloaded, ``export_ivectors`` against the chain of stage functions by hand, and the kalpy-shaped objects."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import ivector as IV
from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd.stats import (gaussian_selection, gaussian_selection_host, ivector_estep, ivector_estep_host,
                                               ivector_utterance_statistics, prune_posteriors, prune_posteriors_host, ubm_statistics)
from montreal_forced_aligner_amd.train import IvectorDeviceBackend, IvectorHostBackend, IvectorTrainer
from tests import ivector_ref as R

pytestmark = pytest.mark.gpu
G, D, RD = 8, 13, 6


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    truth = R.true_model(G=G, D=D, R=RD, seed=11)
    x, off, comp = R.draw(truth, n_utt=40, frames=(20, 40), seed=12)
    d = tmp_path_factory.mktemp("ivector")
    R.ubm_of(x, comp, G).write(d / "final.dubm")
    utts = [(f"utt{i:02d}", x[off[i]: off[i + 1]]) for i in range(len(off) - 1)]
    return dict(x=x, off=off, utts=utts, dir=d)


KW = dict(num_iterations=3, subsample=2, ivector_dimension=RD, num_gselect=4, min_post=0.025, gaussian_min_count=20)


def test_trainer_against_the_host_backend(engine, corpus, tmp_path):
    be = IvectorDeviceBackend(engine=engine)
    tr = IvectorTrainer(backend=be, **KW)
    seen = []

    def compare(i, model, st):
        gamma, X = (t.cpu().numpy() for t in be.utt_stats[0])
        mean, var, _ = (t.cpu().numpy() for t in ivector_estep(engine, model, *be.utt_stats[0], want_var=True))
        refs = R.estep(model, gamma, X)
        R.check_estep(mean, var, refs, model, f"iteration {i}")
        twin = IV.IvectorStats.zeros(G, D, RD)
        tmean, tvar, _ = ivector_estep_host(model, gamma, X, into=twin, want_var=True)
        for un, r in enumerate(refs):
            assert np.linalg.norm(mean[un] - tmean[un]) <= R.mean_distance_bound(r, tmean[un], tvar[un], model), (i, un)
        acc, mag, n = R.accumulate(model, gamma, X, mean, var)
        R.check_accumulators(st, acc, mag, n, f"iteration {i}")
        assert st.n == twin.n == 40 and np.array_equal(st.S, be.S.cpu().numpy())
        seen.append(i)

    tr.on_statistics = compare
    tr.train(corpus["utts"], corpus["dir"] / "final.dubm", tmp_path)
    assert seen == [1, 2, 3] and len(be.batches) == 1
    print("objective per frame:", np.round(tr.objectives, 5), "counts", tr.update_counts)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(tr.objectives, tr.objectives[1:]))

    # the resident statistics: the selection and the pruned posteriors are the host's bits, γ, X and S within the bound
    ubm = tr.ubm
    gs = gaussian_selection_host(corpus["x"], ubm, 4)[0]
    assert np.array_equal(gs, gaussian_selection(engine, be.batches[0], ubm, 4)[0].cpu().numpy())
    _st, post = ubm_statistics(engine, be.batches[0], ubm, torch.from_numpy(gs).to(engine.device), want_post=True)
    pruned = prune_posteriors(engine, post, 0.025, 2.0).cpu().numpy()
    assert R.bits(pruned) == R.bits(prune_posteriors_host(post.cpu().numpy(), 0.025, 2.0))
    ref = R.utt_stats(corpus["x"], corpus["off"], gs, pruned, G)
    R.check_utt_stats(be.utt_stats[0][0].cpu().numpy(), be.utt_stats[0][1].cpu().numpy(), be.S.cpu().numpy(), ref, "resident statistics")

    # the host backend starts from the same seeded model and keeps EM's guarantee too (its posteriors are libm's expf, not the
    # device's, so the two walks are compared per iteration above, on one model, not at their ends)
    host = IvectorTrainer(backend=IvectorHostBackend(), **KW).train(corpus["utts"], corpus["dir"] / "final.dubm")
    assert R.bits(host.models[0].M) == R.bits(tr.models[0].M)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(host.objectives, host.objectives[1:]))

    # final.ie written and reloaded
    final = IV.IvectorExtractorModel.read(tmp_path / "final.ie")
    assert R.bits(final.M, final.sigma_inv) == R.bits(tr.model.M, tr.model.sigma_inv) and final.prior_offset == tr.model.prior_offset
    assert sorted(p.name for p in tmp_path.glob("*.ie")) == ["1.ie", "2.ie", "3.ie", "4.ie", "final.ie"]


def test_export_and_the_kalpy_objects(engine, corpus, tmp_path, monkeypatch):
    from montreal_forced_aligner_amd import kalpy_api as KA

    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    tr = IvectorTrainer(backend=IvectorDeviceBackend(engine=engine), **dict(KW, num_iterations=1))
    tr.train(corpus["utts"], corpus["dir"] / "final.dubm", tmp_path)
    ubm, model, utts = tr.ubm, tr.model, corpus["utts"][:7]

    # export_ivectors against the chain by hand
    calls = []
    ex = KA.IvectorExtractor(corpus["dir"] / "final.dubm", tmp_path / "final.ie", acoustic_weight=0.5, max_count=20.0, num_gselect=4,
                             min_post=0.025)
    ex.export_ivectors(tmp_path / "ivectors.ark", utts, write_scp=True, callback=calls.append)
    assert calls == [k for k, _ in utts]
    x = torch.from_numpy(np.concatenate([m for _k, m in utts])).to(engine.device)
    off = np.concatenate([[0], np.cumsum([m.shape[0] for _k, m in utts])])
    gs, _ = gaussian_selection(engine, x, ubm, 4)
    _st, post = ubm_statistics(engine, x, ubm, gs, want_post=True)
    post = prune_posteriors(engine, post, 0.025, 0.5)
    gamma, X, _ = ivector_utterance_statistics(engine, x, off, gs, post, G, max_count=20.0)
    assert (gamma.sum(dim=1) <= 20.0 * (1 + 1e-12)).all()
    mean = ivector_estep(engine, IV.IvectorExtractorModel.read(tmp_path / "final.ie"), gamma, X)[0].cpu().numpy()
    mean[:, 0] -= model.prior_offset
    table = dict(K.read_ark((tmp_path / "ivectors.ark").read_bytes(), "vector"))
    assert list(table) == [k for k, _ in utts]
    assert all(v.dtype == np.float32 and np.array_equal(v, mean[i].astype(np.float32)) for i, v in enumerate(table.values()))
    assert len(K.read_scp(tmp_path / "ivectors.scp")) == 7
    # one utterance alone: a batch of one, within the distance two solves can have of each other — here the same bits,
    # because an utterance's rows of the products do not depend on its neighbours
    assert np.array_equal(ex.extract_ivector(utts[3][1]), table[utts[3][0]])

    # generate_post, ScalePosterior, the posterior archive, the statistics accumulator
    gmm = KA.DiagGmm.read(corpus["dir"] / "final.dubm")
    entries = []
    for k, m in utts:
        p = gmm.generate_post(m, num_post=4, min_post=0.025)
        assert len(p) == m.shape[0] and all(1 <= len(f) <= 4 and abs(sum(v for _i, v in f) - 1) < 1e-5 for f in p)
        entries.append((k, KA.ScalePosterior(2.0, p)))
    KA.PosteriorArchive.write(tmp_path / "post.ark", entries)
    reader = KA.PosteriorArchive(tmp_path / "post.ark")
    assert list(reader) == entries
    calls = []
    acc = KA.IvectorExtractorStatsAccumulator(tmp_path / "final.ie")
    acc.accumulate_stats(utts + [("stranger", utts[0][1])], reader, callback=calls.append)
    assert calls == [k for k, _ in utts]
    post2 = prune_posteriors(engine, _st_post(engine, x, ubm, gs), 0.025, 1.0)
    g, p = KA.posterior_matrices([f for _k, e in entries for f in e], 4)
    dense = post2.cpu().numpy() * np.float32(2.0)
    want_p = np.zeros_like(dense)
    want_g = np.full(dense.shape, -1, np.int32)
    for t in range(dense.shape[0]):
        keep = np.flatnonzero(dense[t])
        want_p[t, : len(keep)], want_g[t, : len(keep)] = dense[t, keep], gs.cpu().numpy()[t, keep]
    assert np.array_equal(g, want_g) and np.array_equal(p, want_p)
    want = IV.IvectorStats.zeros(G, D, RD)
    dev = lambda a: torch.from_numpy(a).to(engine.device)
    gamma, X, S = ivector_utterance_statistics(engine, x, off, dev(g), dev(p), G, want_S=True)
    ivector_estep(engine, acc.model, gamma, X, into=want)
    st = acc.ivector_stats
    assert R.bits(st.gamma, st.Y, st.Rq, st.isum, st.iscat, st.S) == R.bits(want.gamma, want.Y, want.Rq, want.isum, want.iscat, S.cpu().numpy())
    assert st.n == 7


def _st_post(engine, x, ubm, gs):
    return ubm_statistics(engine, x, ubm, gs, want_post=True)[1]
