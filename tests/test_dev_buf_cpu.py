"""The context's device-buffer type (csrc/dev_buf.hpp) over a fake device, under the host sanitizers.

tests/native/dev_buf_check.cpp instantiates the header with a device that counts live allocations, records the order of
sync / free / alloc / copy calls and fails the n-th allocation or copy on request; it asserts the guarantees the stage
files rely on (no call below capacity, sync → free → alloc on growth, empty after a failed growth, a table set that is
either replaced whole or left bit for bit as it was) and that nothing is live at exit.  It is a stand-alone program: the
sanitizer runtimes are linked into it, nothing is preloaded.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_dev_buf_guarantees_hold_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "dev_buf_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-o", str(exe), str(ROOT / "tests" / "native" / "dev_buf_check.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "all checks passed" in run.stdout and "runtime error" not in run.stdout, run.stdout
