"""Row widths compiled into the Keccak MMCS kernels (valida_amd/csrc/kernels/merkle.hip: hash_row<Cols, N>, k_keccak_leaves<Cols, N>,
k_keccak_compress<N>): the very source under tools/hipemu.  Every width of the product's tables and the widths where the padding can go
wrong — 1, 2; odd widths (the 0x01 pad word in a high half); 32 (pad in word 32, end bit in word 33); 33 (both in word 33: 0x80000001);
34 (a full block, then a block of padding alone); 35; two- and three-block widths of the real list (40 .. 67, 95) — hashed through the
compile-time width, through the run-time width (N = 0) and through the oracle's Keccak MMCS: the three must agree word for word."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2013265921
c_u32p = ctypes.POINTER(ctypes.c_uint32)
LEAF_WIDTHS, LEAF_WIDTHS_STRIDED, INJECT_WIDTHS = (10, 14), (10,), (10, 20, 25, 40, 51, 55, 61, 67, 95)  # merkle.hip: VK_LEAF_WIDTHS, .._STRIDED, VK_INJECT_WIDTHS
EDGE_WIDTHS = (1, 2, 32, 33, 34, 35)
WIDTHS = sorted(set(LEAF_WIDTHS + INJECT_WIDTHS + EDGE_WIDTHS))
ROWS = 64


@pytest.fixture(scope="module")
def emu():
    before = os.environ.get("VGPU_KECCAK_PAIRS")
    os.environ["VGPU_KECCAK_PAIRS"] = "0"  # latched by the emulated launchers at their first launch (below): the thread-per-node kernels at every size
    src = os.path.join(ROOT, "tests", "emu", "keccak_row_width_emu.cpp")
    out = os.path.join(ROOT, "build", "libkeccakrowwidthemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp")] + [
        os.path.join(csrc, "kernels", f) for f in ("merkle.hip", "keccak.hpp", "keccak_pair.hpp", "challenger_dev.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DVK_ALIGNBIT_NOP=0", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    one = np.ones((1, 1), dtype=np.uint32)
    d = np.zeros(8, dtype=np.uint32)
    assert lib.emu_row_digests(5, one.ctypes.data_as(c_u32p), ctypes.c_uint64(1), 1, d.ctypes.data_as(c_u32p)) == 0
    if before is None:
        os.environ.pop("VGPU_KECCAK_PAIRS", None)
    else:
        os.environ["VGPU_KECCAK_PAIRS"] = before
    return lib


def rows_of(w):
    m = np.random.default_rng(4200 + w).integers(0, P, (ROWS, w), dtype=np.uint32)
    m[0, :] = 0          # canonical 0 and p - 1 in every column
    m[1, :] = P - 1
    return np.ascontiguousarray(m)


def row_digests(emu, mode, m, instance=0):
    d = np.zeros((m.shape[0], 8), dtype=np.uint32)
    rc = emu.emu_row_digests(mode, m.ctypes.data_as(c_u32p), ctypes.c_uint64(m.shape[0]), m.shape[1], d.ctypes.data_as(c_u32p))
    assert rc == instance, "width %d, mode %d: %d" % (m.shape[1], mode, rc)  # modes 3, 4: the width compiled into the instance launched; else 0
    return d


@pytest.mark.parametrize("w", WIDTHS)
def test_rows_of_a_compile_time_width_hash_as_the_generic_code_and_the_oracle(emu, w):
    m = rows_of(w)
    want = np.array([po.mmcs_root([m[i:i + 1]]) for i in range(ROWS)], dtype=np.uint32)
    assert np.array_equal(row_digests(emu, 0, m), want)  # hash_row<PtrCols, 0>
    assert np.array_equal(row_digests(emu, 1, m), want)  # hash_row<PtrCols, w>
    assert np.array_equal(row_digests(emu, 2, m), want)  # hash_row<StridedCols, w>
    # the product's dispatch: the instance of a listed width, the generic one for any other
    assert np.array_equal(row_digests(emu, 3, m, w if w in LEAF_WIDTHS else 0), want)
    assert np.array_equal(row_digests(emu, 4, m, w if w in LEAF_WIDTHS_STRIDED else 0), want)
    assert np.array_equal(row_digests(emu, 5, m), want)  # launch_keccak_leaves
    assert np.array_equal(row_digests(emu, 6, m), want)  # launch_keccak_leaves_strided


@pytest.fixture(scope="module")
def children():
    """2 * ROWS leaf digests (the layer under the injecting one) and the rows they hash."""
    tall = np.ascontiguousarray(np.random.default_rng(77).integers(0, P, (2 * ROWS, 3), dtype=np.uint32))
    return tall, np.ascontiguousarray(np.array([po.mmcs_root([tall[i:i + 1]]) for i in range(2 * ROWS)], dtype=np.uint32))


@pytest.mark.parametrize("w", WIDTHS)
def test_injecting_compress_of_a_compile_time_width(emu, children, w):
    tall, prev = children
    low = rows_of(w)
    want = np.array([po.mmcs_root([tall[2 * i:2 * i + 2], low[i:i + 1]]) for i in range(ROWS)], dtype=np.uint32)
    # k_keccak_compress<0>, k_keccak_compress<w>, the product's dispatch (the instance of a listed width, else the generic one), launch_keccak_compress
    for mode, instance in ((0, 0), (1, 0), (3, w if w in INJECT_WIDTHS else 0), (5, 0)):
        got = np.zeros((ROWS, 8), dtype=np.uint32)
        assert emu.emu_compress_layer(mode, prev.ctypes.data_as(c_u32p), low.ctypes.data_as(c_u32p), ctypes.c_uint64(ROWS), w, got.ctypes.data_as(c_u32p)) == instance, mode
        assert np.array_equal(got, want), mode


def test_the_tables_of_this_file_are_the_kernel_tables():
    """The widths tested above are read from here, not from merkle.hip: the two lists must stay the same."""
    src = open(os.path.join(ROOT, "valida_amd", "csrc", "kernels", "merkle.hip")).read()
    for name, widths in (("VK_LEAF_WIDTHS", LEAF_WIDTHS), ("VK_LEAF_WIDTHS_STRIDED", LEAF_WIDTHS_STRIDED), ("VK_INJECT_WIDTHS", INJECT_WIDTHS)):
        assert "#define %s(X) %s\n" % (name, " ".join("X(%d)" % w for w in widths)) in src, name
    emu_src = open(os.path.join(ROOT, "tests", "emu", "keccak_row_width_emu.cpp")).read()
    assert "#define EMU_WIDTHS(X) %s\n" % " ".join("X(%d)" % w for w in WIDTHS) in emu_src
