"""The dense lane's logic (valida_amd/csrc/host/dense_lane.hpp) on the host, over a mock event API: tests/emu/dense_lane_host.cpp is a program of
its own (own main) that drives the lane from 4 threads x 2000 enter / leave pairs with random context destruction and checks that every wait
targets an event recorded earlier, that no context waits on its own event and that the tail order equals the acquisition order.  Built twice —
AddressSanitizer + UBSan, and ThreadSanitizer — and run directly: nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "dense_lane_host.cpp")


def _compiler():
    path = shutil.which("g++")
    assert path, "g++ not found"
    return path


# the sanitizer runtimes are linked statically: the program then runs directly in whatever environment the suite runs in, passed through unchanged
@pytest.mark.parametrize("name,flags", [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan"]),
                                        ("tsan", ["-fsanitize=thread", "-static-libtsan"])])
def test_lane_invariants_under_sanitizers(tmp_path, name, flags):
    exe = str(tmp_path / ("dense_lane_host_" + name))
    subprocess.run([_compiler(), "-O1", "-g", "-std=c++17", "-pthread"] + flags + [SRC, "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "4", "2000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "8000 records" in r.stdout and " 0 failures" in r.stdout, r.stdout
    waits = int(r.stdout.split(" waits")[0].split()[-1])
    assert waits > 0, "no thread ever met another context's tail: the run proves nothing\n" + r.stdout
