"""The host twin of the equal alignment (mfa_debug_align_equal_host, csrc/align_equal_host.cpp over
csrc/align_equal_math.hpp) without a GPU: the properties that need no reference on the case set of
tests/align_equal_cases.py, and the twin's translation unit under the host sanitizers as a stand-alone program (nothing is
preloaded anywhere)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from montreal_forced_aligner_amd import _lib
from montreal_forced_aligner_amd import equal_align as E
from tests import align_equal_cases as A

ROOT = Path(__file__).resolve().parents[1]
SEED = 1234


@pytest.fixture(scope="module")
def batch():
    cs = A.cases()
    keys = np.arange(100, 100 + len(cs), dtype=np.uint32)
    fo = A.frame_offsets(cs)
    ali, status = E.equal_align_host([c.fst for c in cs], fo, keys, SEED)
    return cs, keys, fo, ali, status


def test_case_set_is_the_shape_the_device_test_needs(batch):
    cs, _keys, fo, _ali, status = batch
    assert len(cs) == 70 and min(c.T for c in cs) == 0 and max(c.T for c in cs) == 300
    assert (status == 0).sum() >= 40 and (status == 2).sum() >= 10


def test_every_result_is_a_path_with_evenly_spread_loops(batch):
    cs, _keys, fo, ali, status = batch
    for k, c in enumerate(cs):
        A.check_result(c, ali[fo[k]: fo[k + 1]], int(status[k]))


def test_same_bits_alone_in_another_batch_and_twice(batch):
    cs, keys, fo, ali, status = batch
    for k, c in enumerate(cs):
        a1, s1 = E.equal_align_host([c.fst], np.array([0, c.T]), keys[k: k + 1], SEED)
        assert int(s1[0]) == int(status[k]) and np.array_equal(a1, ali[fo[k]: fo[k + 1]]), c.name
    rev = list(range(len(cs)))[::-1]
    ar, sr = E.equal_align_host([cs[k].fst for k in rev], A.frame_offsets([cs[k] for k in rev]), keys[rev], SEED)
    assert np.array_equal(sr, status[rev])
    assert np.array_equal(ar, np.concatenate([ali[fo[k]: fo[k + 1]] for k in rev]))
    a2, s2 = E.equal_align_host([c.fst for c in cs], fo, keys, SEED)
    assert np.array_equal(a2, ali) and np.array_equal(s2, status)


def test_seed_and_key_choose_the_path(batch):
    cs, keys, fo, ali, status = batch
    other_seed, _ = E.equal_align_host([c.fst for c in cs], fo, keys, SEED + 1)
    other_key, _ = E.equal_align_host([c.fst for c in cs], fo, keys + 1000, SEED)
    differs_seed = differs_key = 0
    for k, c in enumerate(cs):
        if c.branching and status[k] == 0:
            differs_seed += not np.array_equal(other_seed[fo[k]: fo[k + 1]], ali[fo[k]: fo[k + 1]])
            differs_key += not np.array_equal(other_key[fo[k]: fo[k + 1]], ali[fo[k]: fo[k + 1]])
    assert differs_seed >= 1 and differs_key >= 1


def test_random_numbers_are_the_headers():
    """The mix of include/mfa_hip.h restated: a chain of two-way choices shows the draws' top bits one by one."""
    def fmix(h):
        h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
        return h

    def draw(seed, key, d):
        h = fmix(seed ^ 0x9E3779B9)
        h = fmix((h + key * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF)
        return fmix(h ^ ((d * 0xC2B2AE35 + 0x27D4EB2F) & 0xFFFFFFFF))

    n = 40                                    # state s → s + 1 by label 2 s + 1 or 2 s + 2
    f = A.make_fst(n + 1, [(s, 2 * s + 1 + b, s + 1) for s in range(n) for b in (0, 1)], [n])
    for seed, key in ((0, 0), (1234, 7), (0xFFFFFFFF, 0xFFFFFFFF)):
        ali, st = E.equal_align_host([f], np.array([0, n]), [key], seed)
        assert st[0] == 0
        want = [2 * s + 1 + ((draw(seed, key, s) * 2) >> 32) for s in range(n)]
        assert ali.tolist() == want
    three = A.make_fst(2, [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [1])
    picks = {int(E.equal_align_host([three], np.array([0, 1]), [k], 5)[0][0]) for k in range(64)}
    assert picks == {1, 2, 3}
    for k in range(8):
        assert int(E.equal_align_host([three], np.array([0, 1]), [k], 5)[0][0]) == 1 + ((draw(5, k, 0) * 3) >> 32)


def test_twin_refusals_and_empty_batch():
    lib = _lib.lib()
    assert lib.mfa_debug_align_equal_host(0, None, None, None, None, None, None, None, None, None, 0, None, None) == 0
    assert lib.mfa_debug_align_equal_host(1, None, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.mfa_debug_align_equal_host(-1, None, None, None, None, None, None, None, None, None, 0, None, None) == -1
    c = A.cases()[0]
    big = np.array([0, 1 << 31], dtype=np.int64)
    graph = [np.ascontiguousarray(a) for a in (
        np.array([0, c.fst.num_states], np.int64), np.array([0, c.fst.num_arcs], np.int64), np.zeros(1, np.int32),
        c.fst.arc_offsets.astype(np.int32), c.fst.final.astype(np.float32), c.fst.arcs["nextstate"].astype(np.int32),
        c.fst.arcs["ilabel"].astype(np.int32))]
    key, st = np.zeros(1, np.uint32), np.full(1, -1, np.int32)
    # 2^31 frames: refused before anything is allocated or written
    assert lib.mfa_debug_align_equal_host(1, *(a.ctypes.data for a in graph), big.ctypes.data, key.ctypes.data, 0, None,
                                          st.ctypes.data) == -2
    assert st[0] == -1
    with pytest.raises(ValueError, match="keys"):
        E.equal_align_host([c.fst], np.array([0, c.T]), [1, 2], 0)
    ali, st = E.equal_align_host([], np.zeros(1, np.int64), [], 0)
    assert ali.shape == (0,) and st.shape == (0,)


def test_twin_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "align_equal_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", str(exe),
                           str(ROOT / "tests" / "native" / "align_equal_check.cpp"),
                           str(ROOT / "montreal_forced_aligner_amd" / "csrc" / "align_equal_host.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout
