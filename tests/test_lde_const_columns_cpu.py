"""Constant trace columns in the fused LDE, without a GPU: tests/emu/lde_colmap_emu.cpp runs the changed kernel sources — k_ingest with its column
flags, k_lde_colmap, k_lde_fill_const and the mapped k_lde_a / k_lde_mid* / k_lde_c — under tools/hipemu and compares every LDE, with and without the
map, word for word with the oracle's committed LDE (coset_lde_batch + bit reversal) and the flags with numpy's (m == m[0]).all(0).  The program has its
own main and is built with AddressSanitizer + UBSan; it is run directly, nothing is loaded into this interpreter.

Heights: 2^13 (the smallest with three passes: k_lo = 12, k_hi = 1), 2^14, and 2^12 (one pass: the map is ignored, the result unchanged).
Blowup 2 and 4; widths 1, 5, 17."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "lde_colmap_emu.cpp")
P = 2013265921
SHIFT = 31
MID_ROW = 64 + 32  # the middle of the second 64-row block of k_ingest


def column(kind, n, rng):
    """One column of a pattern: a constant (0, 1, p - 1 in canonical form), a constant with one deviating row, or random."""
    if kind == "rand":
        return rng.integers(0, P, n, dtype=np.uint32)
    const = {"zero": 0, "one": 1, "pm1": P - 1, "but_last": 7, "but_first": 11, "but_mid": 13}[kind]
    c = np.full(n, const, dtype=np.uint32)
    if kind == "but_last":
        c[n - 1] = 8  # must not be flagged constant
    elif kind == "but_first":
        c[0] = 12
    elif kind == "but_mid":
        c[MID_ROW] = 14
    return c


def patterns(w):
    """The column kinds of every pattern matrix of width w."""
    out = {}
    if w == 1:
        for kind in ("rand", "zero", "one", "pm1", "but_last", "but_first", "but_mid"):  # 'rand' = no constant column, the constants = all columns constant
            out[kind] = [kind]
        return out
    out["none"] = ["rand"] * w
    out["only_col0"] = ["zero"] + ["rand"] * (w - 1)
    out["only_last"] = ["rand"] * (w - 1) + ["pm1"]
    out["all"] = [("zero", "one", "pm1")[j % 3] for j in range(w)]  # live count 0
    out["mixed"] = (["one", "but_last", "pm1", "but_first", "but_mid"] + ["rand", "zero"] * w)[:w]
    return out


def build_cases(log_n, log_blowup):
    rng = np.random.default_rng(1300 + 10 * log_n + log_blowup)
    words = []
    count = 0
    n = 1 << log_n
    for w in (1, 5, 17):
        for name, kinds in patterns(w).items():
            m = np.ascontiguousarray(np.stack([column(k, n, rng) for k in kinds], axis=1), dtype=np.uint32)
            const = (m == m[0]).all(0)
            assert list(const) == [k in ("zero", "one", "pm1") for k in kinds], name
            want = po.committed_lde(m, log_blowup, SHIFT)
            for j in np.nonzero(const)[0]:  # the premise of the whole change, on the oracle's side
                assert (want[:, j] == m[0, j]).all()
            words += [np.array([log_n, w, log_blowup, SHIFT], dtype=np.uint32), m.ravel(), const.astype(np.uint32), np.ascontiguousarray(want, dtype=np.uint32).ravel()]
            count += 1
    return count, np.concatenate([np.array([count], dtype=np.uint32)] + words)


SHAPES = [(13, 1), (13, 2), (14, 1), (14, 2), (12, 1), (12, 2)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The program, built once (kept under build/ while its sources are unchanged, as the other emulations are), and one run per shape — started
    together, each a process of its own: under AddressSanitizer every fiber switch of the emulator is slow, and the shapes are independent."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = os.path.join(ROOT, "build", "lde_colmap_emu_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(ROOT, "valida_amd", "csrc", "field.hpp")] + [
        os.path.join(ROOT, "valida_amd", "csrc", "kernels", f) for f in ("ntt.hip", "layout.hip", "butterfly.hpp", "launch.hpp", "device_common.hpp", "profiler.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # the sanitizer runtimes are linked statically: the program then runs directly in whatever environment the suite runs in
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-static-libasan", "-static-libubsan", "-x", "c++", "-I",
                        os.path.join(ROOT, "tools", "hipemu"), SRC, "-o", exe + ".tmp"], check=True, capture_output=True, text=True, timeout=600)
        os.replace(exe + ".tmp", exe)
    tmp = tmp_path_factory.mktemp("lde_colmap_emu")
    procs = {}
    for log_n, log_blowup in SHAPES:
        count, blob = build_cases(log_n, log_blowup)
        path = str(tmp / ("cases_%d_%d.bin" % (log_n, log_blowup)))
        blob.tofile(path)
        procs[(log_n, log_blowup)] = (count, subprocess.Popen([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    yield procs
    for _, p in procs.values():
        if p.poll() is None:
            p.kill()
        p.communicate()


@pytest.mark.parametrize("log_n,log_blowup", SHAPES)
def test_mapped_lde_kernels_under_emulation_match_the_oracle(runs, log_n, log_blowup):
    count, proc = runs[(log_n, log_blowup)]
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, (out + err)[-3000:]
    assert ("%d cases" % count) in out and " 0 failures" in out, out
