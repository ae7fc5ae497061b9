"""The host layer by role: every name ``engine`` used to define is still importable from it and is the object its new module
defines; ``ragged`` stays free of torch; the staging ring hands its pools out in a fixed cycle, waiting for the one it
returns; and the helpers that replaced repeated expressions compute those expressions."""
import copy
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd import _lib, engine, frontend, packing, pipeline, ragged, speaker_train, staging, stats, train
from montreal_forced_aligner_amd.stats import _common, alignment, pairs, speaker

REEXPORTS = {
    engine: ("AlignmentEngine", "redo_capacity", "DEFAULT_MFCC"),
    pipeline: ("Pipeline",),
    packing: ("PackedGraphs",),
    staging: ("StagingPool", "StagingRing"),
    alignment: ("GmmStats", "check_delta_fmllr", "fmllr_statistics", "gmm_statistics", "gmm_statistics_host", "tid_tables"),
    ragged: ("offsets", "_speaker_groups"),
    frontend: ("DEFAULT_PITCH", "_PITCH_ALIAS"),
    _lib: ("_ptr",),
}

# the public names of stats.py before it became a package, and ``_unit_rows``, by the module that defines each now
STATS_NAMES = {
    alignment: ("model_arrays", "check_delta_fmllr", "tid_tables", "silence_weights", "fmllr_statistics", "GmmStats", "gmm_statistics",
                "gmm_statistics_twofeats", "gmm_statistics_host", "gmm_statistics_twofeats_host", "LdaStats", "lda_statistics",
                "lda_statistics_host", "gaussian_means", "MlltStats", "mllt_statistics", "mllt_statistics_host", "TREE_NO_KEY",
                "TREE_MAX_PHONES", "TREE_MAX_CLASSES", "tree_key", "TreeStats", "tree_tid_tables", "tree_statistics",
                "tree_statistics_host"),
    speaker: ("gaussian_selection", "ubm_statistics", "gaussian_selection_host", "ubm_statistics_host", "prune_posteriors",
              "prune_posteriors_host", "ivector_utterance_statistics", "ivector_utterance_statistics_host", "ivector_estep",
              "ivector_estep_host"),
    pairs: ("PLDA_BLOCK_BYTES", "PLDA_MATRIX_BYTES", "plda_transform", "plda_transform_host", "plda_scores", "plda_classify", "plda_knn",
            "plda_sweep", "plda_prepare_host", "plda_scores_host", "plda_classify_host", "plda_knn_host", "plda_sweep_host",
            "METRIC_CODES", "NEIGHBOR_BITS_BYTES", "metric_code", "score_threshold", "score_to_distance", "metric_sweep",
            "metric_sweep_host", "neighbor_bits", "neighbor_bits_host", "knn", "knn_host", "dbscan_from_bits", "dbscan_from_bits_host",
            "pair_metric", "core_scores", "pair_prepare", "core_scores_host", "pair_prepare_host", "finish_tree", "mreach_mst",
            "mreach_mst_host", "_unit_rows"),
}
TRAIN_NAMES = ("UbmHostBackend", "UbmDeviceBackend", "DubmTrainer", "IvectorHostBackend", "IvectorDeviceBackend", "IvectorTrainer")


def _is_the_object_its_home_defines(package, name, home):
    obj = getattr(home, name)
    assert getattr(package, name) is obj
    if hasattr(obj, "__module__"):            # (classes and functions: defined there, not passed through)
        assert obj.__module__ == home.__name__


@pytest.mark.parametrize("name,home", [(n, m) for m, names in REEXPORTS.items() for n in names])
def test_engine_reexports_the_object_of_the_new_module(name, home):
    _is_the_object_its_home_defines(engine, name, home)


def test_the_list_of_stats_names_is_whole():
    names = [n for group in STATS_NAMES.values() for n in group]
    assert len(names) == len(set(names)) == 69 + 1


@pytest.mark.parametrize("name,home", [(n, m) for m, names in STATS_NAMES.items() for n in names])
def test_stats_reexports_the_object_of_its_submodule(name, home):
    _is_the_object_its_home_defines(stats, name, home)


@pytest.mark.parametrize("name", TRAIN_NAMES)
def test_train_reexports_the_speaker_trainers(name):
    _is_the_object_its_home_defines(train, name, speaker_train)


def test_device_model_cache_is_kept_per_model_for_one_device_at_a_time():
    calls = []

    class Model:
        def arrays(self):
            calls.append(1)
            return np.arange(3.0), np.ones((2, 2), dtype=np.float32)

    class Engine:
        device = torch.device("cpu")

    model, eng = Model(), Engine()
    first = _common.device_model(eng, model, model.arrays)
    assert isinstance(first, tuple) and [t.dtype for t in first] == [torch.float64, torch.float32]
    assert all(t.device == eng.device for t in first) and torch.equal(first[0], torch.arange(3.0, dtype=torch.float64))
    assert _common.device_model(eng, model, model.arrays) is first and len(calls) == 1      # the same tuple, nothing computed again
    assert _common.device_model(eng, Model(), model.arrays) is not first                    # kept on the model object
    eng.device = torch.device("meta")
    second = _common.device_model(eng, model, model.arrays)
    assert second is not first and all(t.device.type == "meta" for t in second)
    assert list(model._device_arrays) == ["meta"]                                            # the other device's copies are let go
    eng.device = torch.device("cpu")
    assert _common.device_model(eng, model, model.arrays) is not first                       # so going back uploads again


def test_ragged_imports_without_torch():
    code = "import sys; import montreal_forced_aligner_amd.ragged; sys.exit(1 if 'torch' in sys.modules else 0)"
    root = Path(__file__).resolve().parent.parent
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


@pytest.mark.parametrize("n", [1, 2, 3])
def test_ring_hands_out_every_pool_once_per_round_and_waits_for_it_alone(n, monkeypatch):
    waited = []

    class Recording(staging.StagingPool):
        def wait(self):
            waited.append(self)
            super().wait()

    monkeypatch.setattr(staging, "StagingPool", Recording)
    ring = staging.StagingRing(torch.device("cpu"), n, pinned=False)
    assert len(ring.pools) == n and all(type(p) is Recording and not p.pinned for p in ring.pools)
    handed = []
    for _ in range(3 * n):
        before = len(waited)
        pool = ring.next()
        assert waited[before:] == [pool]              # waited for before it is returned, and for no other
        handed.append(pool)
    first = handed[:n]
    assert sorted(map(id, first)) == sorted(map(id, ring.pools))      # every pool once per n calls
    assert all(p is q for p, q in zip(handed, first * 3))             # and the same cycle again


def test_max_len_is_the_expression_it_replaces():
    for off in ([0], [0, 0], [0, 5], [0, 3, 3, 10], np.array([0, 4, 4, 6, 13], dtype=np.int32), np.array([0], dtype=np.int64)):
        n = len(off) - 1
        want = int(np.diff(off).max()) if n else 0
        got = ragged.max_len(off)
        assert type(got) is int and got == want, (off, got, want)


def _parent_fmllr_tables(tm, silence_phones, silence_weight):
    """fmllr_statistics' own tables before it called tid_tables."""
    id2pdf = np.maximum(tm.id2pdf, 0).astype(np.int32)
    sil = np.zeros(tm.id2phone.shape[0], dtype=np.float32)
    sil[np.isin(tm.id2phone, np.asarray(list(silence_phones), dtype=np.int64))] = 1.0
    w_host = np.where(sil > 0, np.float32(silence_weight), np.float32(1.0)).astype(np.float32)
    w_host[0] = 0.0
    return id2pdf, w_host


@pytest.mark.parametrize("silence_weight", [0.0, 0.25])
def test_tid_tables_with_silence_weights_is_the_fmllr_pair_it_replaces(fx, silence_weight):
    tm = fx.mono_tm
    phones = np.unique(tm.id2phone[1:])
    absent = int(phones.max()) + 7
    for silence in ([int(phones[0])], [int(phones[0]), int(phones[-1])], [], [absent], [int(phones[1]), absent]):
        got = stats.tid_tables(tm, weights=stats.silence_weights(tm, silence, silence_weight))
        want = _parent_fmllr_tables(tm, silence, silence_weight)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.flags.c_contiguous and np.array_equal(g, w), (silence, silence_weight)
        assert got[1][0] == 0.0
        if silence_weight != 1.0 and silence and silence != [absent]:
            assert (got[1][1:] == np.float32(silence_weight)).any()


def test_model_arrays_are_the_views_they_replace(fx):
    am = fx.mono_am
    f64 = copy.copy(am)
    f64.pdf_offsets = am.pdf_offsets.astype(np.int64)
    f64.gconsts, f64.means_invvars, f64.inv_vars = (np.asarray(a, dtype=np.float64) for a in (am.gconsts, am.means_invvars, am.inv_vars))
    strided = copy.copy(am)
    strided.pdf_offsets = np.repeat(am.pdf_offsets, 2)[::2]
    strided.gconsts = np.repeat(am.gconsts, 3)[::3]
    strided.means_invvars, strided.inv_vars = np.asfortranarray(am.means_invvars), np.repeat(am.inv_vars, 2, axis=1)[:, ::2]
    assert not strided.gconsts.flags.c_contiguous and not strided.inv_vars.flags.c_contiguous
    for gmm in (am, f64, strided):
        want = (np.ascontiguousarray(gmm.pdf_offsets, dtype=np.int32), np.ascontiguousarray(gmm.gconsts, dtype=np.float32),
                np.ascontiguousarray(gmm.means_invvars, dtype=np.float32), np.ascontiguousarray(gmm.inv_vars, dtype=np.float32))
        got = stats.model_arrays(gmm)
        assert len(got) == 4
        for g, w, orig in zip(got, want, (am.pdf_offsets, am.gconsts, am.means_invvars, am.inv_vars)):
            assert g.dtype == w.dtype and g.shape == w.shape and g.flags.c_contiguous and np.array_equal(g, w)
            assert np.array_equal(g, orig)
