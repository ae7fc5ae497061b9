"""The wavefront decoder's launch plan (csrc/viterbi_plan.hpp) swept on the CPU, under the host sanitizers.

tests/native/viterbi_plan_check.cpp includes the header align_impl consumes and sweeps it over graph sizes up to 20 000
states, arc counts up to eight per state, the token capacities callers use, with and without epsilon arcs, dense and lazy:
every launch fits 160 KiB of LDS, capacities are multiples of 64, a hashed table has at least four buckets per token and
no more buckets than states, the token lists are in LDS exactly when they fit.  It also reports what it measured: the
sizes at which the tiers change, and that two branches (the refusal, the half-limit clause of the list decision) are never
reached.  A stand-alone program: the sanitizer runtimes are linked into it, nothing is preloaded.

The exported query (mfa_debug_viterbi_plan) is the same function; the second test holds the library's copy to the
thresholds the program prints.
"""
import re
import subprocess
from pathlib import Path

import pytest

from tests import decoder_tier_cases as D

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("viterbi_plan") / "viterbi_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined",
                           "-o", str(exe), str(ROOT / "tests" / "native" / "viterbi_plan_check.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_plan_sweep_holds_under_asan_and_ubsan(report):
    assert "all checks passed" in report and "runtime error" not in report and "FAILED" not in report, report
    assert "the refusal branch is unreachable in the sweep" in report
    assert "the clause is dead" in report


def test_library_plan_changes_tier_at_the_measured_thresholds(report):
    """The sizes the native sweep measured (3.8 arcs a state, one token per state, beam and retry beam), asked of the
    library: one state below each the tier has not changed, at it it has."""
    found = re.findall(r"threshold (epsilon-free|with epsilon arcs): token lists in HBM from max_states (\d+), "
                       r"capacity shrink from max_states (\d+)", report)
    assert len(found) == 2
    for which, hbm, shrink in found:
        eps, hbm, shrink = which != "epsilon-free", int(hbm), int(shrink)
        for lazy in (0, 1):
            def rows(S):
                return D.plan(S, int(3.8 * S) + 1, eps, lazy, retry_beam=40.0, max_tokens=S, bp_tokens_per_frame=S)
            assert all(r["lists_in_lds"] for r in rows(hbm - 1))
            assert not rows(hbm)[-1]["lists_in_lds"] and rows(hbm)[-1]["N"] == D.ceil64(hbm)
            assert all(r["N"] == D.ceil64(shrink - 1) for r in rows(shrink - 1)[1:])
            assert rows(shrink)[-1]["N"] < D.ceil64(shrink)
    # the documented sizes (tests/decoder_tier_cases.py, PackedGraphs.hard_bounds)
    assert [(w, int(a), int(b)) for w, a, b in found] == [("epsilon-free", 1836, 2881), ("with epsilon arcs", 1365, 1921)]
