"""``DubmTrainer`` on the device end to end, over the two corpora of tests/test_ubm_cpu.py: at every iteration the device's
statistics for the device's current model equal the host twin's for that same model within the bound of tests/ubm_ref.py,
the first selection is the host's bit for bit, the log-likelihood conditions of the CPU test hold, ``final.dubm`` reloads and
selects; and the kalpy-shaped objects give the stage functions' results."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import kaldi_io as K
from montreal_forced_aligner_amd import ubm as U
from montreal_forced_aligner_amd.stats import gaussian_selection, gaussian_selection_host, ubm_statistics, ubm_statistics_host
from montreal_forced_aligner_amd.train import DubmTrainer, UbmDeviceBackend
from tests import ubm_ref as R
from tests.test_ubm_cpu import check_trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_mfcc_after(engine):
    yield
    engine.configure_mfcc()


def run_trainer(engine, utts, tmp_path, **kw):
    be = UbmDeviceBackend(engine=engine, batch_frames=6000)
    tr = DubmTrainer(backend=be, **kw)
    seen = []

    def compare(i, model, st):
        """the device statistics of iteration i against the twin's for the same model and selection"""
        twin = None
        for b, gs in zip(be.batches, be.gselect):
            x, g = b.cpu().numpy(), gs.cpu().numpy()
            twin = ubm_statistics_host(x, model, g, into=twin)
        x = np.concatenate([b.cpu().numpy() for b in be.batches])
        g = np.concatenate([gs.cpu().numpy() for gs in be.gselect])
        ref = R.ubm_acc(x, model, g)
        for got, want, bound in ((st.occ, twin.occ, ref["B_occ"]), (st.mean_acc, twin.mean_acc, ref["B_mean"]),
                                 (st.var_acc, twin.var_acc, ref["B_var"])):
            assert (np.abs(got - want) <= 2 * bound).all(), i
        assert abs(st.tot_like - twin.tot_like) <= 2 * ref["B_tot"] and st.tot_count == twin.tot_count, i
        seen.append(i)

    tr.on_statistics = compare
    tr.initialize(utts)
    first = tr.models[0]
    for b, gs in zip(be.batches, be.gselect):                  # the first selection is the host's
        assert np.array_equal(gs.cpu().numpy(), gaussian_selection_host(b.cpu().numpy(), first, tr.num_gselect)[0])
    tr2 = DubmTrainer(backend=be, **kw)
    tr2.on_statistics = compare
    tr2.train(utts, tmp_path)
    assert seen == list(range(1, tr2.num_iterations + 1))
    assert all(np.array_equal(a, b) for a, b in zip(tr2.models[0].arrays(), first.arrays()))      # seeded: the same init twice
    return tr2


def test_trainer_on_a_known_mixture(engine, tmp_path):
    _truth, utts = R.mixture8()
    tr = run_trainer(engine, utts, tmp_path, num_iterations=4, num_gselect=8, num_gaussians=8, num_iterations_init=4,
                     initial_gaussian_proportion=0.5, num_frames=5000)
    print("init", np.round(tr.init_loglikes, 4), "train", np.round(tr.loglikes, 4))
    assert tr.backend.num_frames == 20000 and len(tr.backend.batches) == 4
    assert all(b >= a - 1e-4 * abs(a) for a, b in zip(tr.loglikes, tr.loglikes[1:]))
    assert tr.loglikes[-1] > tr.init_loglikes[0]
    final = check_trainer(tr, tmp_path)
    x = torch.from_numpy(utts[0][1]).to(engine.device)
    gs, _ = gaussian_selection(engine, x, final, 3)
    assert np.array_equal(gs.cpu().numpy(), gaussian_selection_host(utts[0][1], final, 3)[0])


def test_trainer_on_the_reference_recording(engine, tmp_path):
    utts = R.wav_features()
    tr = run_trainer(engine, utts, tmp_path, num_iterations=2, num_gselect=30, num_gaussians=16, num_iterations_init=4)
    print("init", np.round(tr.init_loglikes, 4), "select", round(tr.select_loglike, 4), "train", np.round(tr.loglikes, 4))
    final = check_trainer(tr, tmp_path)
    assert tr.loglikes[-1] > tr.init_loglikes[0]
    x = np.concatenate([m for _k, m in utts])
    gs, _ = gaussian_selection(engine, torch.from_numpy(x).to(engine.device), final, 30)
    assert np.array_equal(gs.cpu().numpy(), gaussian_selection_host(x, final, 30)[0])


def test_kalpy_objects_give_the_stage_functions_results(engine, fx, tmp_path, monkeypatch):
    from montreal_forced_aligner_amd import kalpy_api as KA

    monkeypatch.setattr(KA, "get_engine", lambda device=0: engine)
    engine.configure_mfcc(use_energy=1, raw_energy=0)
    sr = 16000
    pieces = {"s1-a": fx.pcm[: 6 * sr], "s1-b": fx.pcm[6 * sr: 14 * sr], "s2-c": fx.pcm[14 * sr: 24 * sr]}
    d_pcm, so = engine.gather_pcm(list(pieces.values()))
    mfcc, fo = engine.mfcc(d_pcm, so)
    host = mfcc.cpu().numpy()
    feats = {k: host[fo[i]: fo[i + 1]] for i, k in enumerate(pieces)}
    K.write_table(tmp_path / "feats.ark", list(feats.items()), "matrix", tmp_path / "feats.scp")
    KA.VadComputer().export_vad(tmp_path / "vad.ark", list(feats.items()), write_scp=True)
    archive = lambda: KA.FeatureArchive(tmp_path / "feats.scp", vad_file_name=tmp_path / "vad.scp", subsample_n=5, use_sliding_cmvn=True)
    utts = list(archive())
    assert [k for k, _ in utts] == list(pieces) and all(m.shape[1] == 13 for _k, m in utts)
    x = np.concatenate([m for _k, m in utts])

    # DiagGmm as the reference's init phase drives it
    gmm = KA.DiagGmm(6, 13)
    gmm.init_from_random_frames(x)
    before = gmm.ubm
    like = gmm.train_one_iter(x, KA.MleDiagGmmOptions(), 0, 1)
    st = ubm_statistics(engine, torch.from_numpy(x).to(engine.device), before)
    assert like == st.loglike_per_frame
    assert all(np.array_equal(a, b) for a, b in zip(gmm.ubm.arrays(), U.update(before, st, True, 1e-5)[0].arrays()))
    gmm.Split(8, 0.1)
    assert gmm.NumGauss() == 8 and gmm.Dim() == 13
    gmm.write(tmp_path / "1.dubm")

    # gaussian_selection, the archive written and read
    model = KA.DiagGmm.read(tmp_path / "1.dubm")
    entries, tot = [], 0.0
    for k, m in utts:
        gselect, like = model.gaussian_selection(m, 5)
        want, ll = gaussian_selection(engine, torch.from_numpy(m).to(engine.device), model.ubm, 5)
        assert gselect == want.cpu().numpy().tolist() and like == float(ll.double().sum().item())
        entries.append((k, gselect)); tot += like
    KA.GselectArchive.write(tmp_path / "gselect.ark", entries)
    ga = KA.GselectArchive(tmp_path / "gselect.ark")
    assert list(ga) == entries

    # GlobalGmmStatsAccumulator over the feature archive, then mle_update
    calls = []
    acc = KA.GlobalGmmStatsAccumulator(tmp_path / "1.dubm")
    acc.accumulate_stats(archive(), ga, callback=calls.append)
    assert calls == list(pieces)
    g = np.concatenate([np.asarray(v, dtype=np.int32) for _k, v in entries])
    want = ubm_statistics(engine, torch.from_numpy(x).to(engine.device), model.ubm, torch.from_numpy(g).to(engine.device))
    assert R.bits(acc.gmm_accs.stats) == R.bits(want)
    total = KA.AccumDiagGmm()
    total.Resize(model)
    total.Add(1.0, acc.gmm_accs)
    model.mle_update(total, remove_low_count_gaussians=False)
    assert all(np.array_equal(a, b) for a, b in zip(model.ubm.arrays(), U.update(KA.DiagGmm.read(tmp_path / "1.dubm").ubm, want, False)[0].arrays()))
