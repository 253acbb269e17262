"""The rank audit without a GPU: the host implementation of the contract (vgpu_rank_audit_host) against the restatement of
tests/rank_audit_ref.py (exact interpolation of the oracle's own chip transcription, numpy RREF) word for word, for both machine kinds; analytic
AIRs captured through vgpu_air_* whose null spaces are known in closed form; options; the device kernels' very source under tools/hipemu;
`check --rank` on the command line; the C ABI's new symbols.  The reference of each input is computed once per module and cut to the limits a
test asks for (counts do not depend on them).  The coupled columns pinned here are the reference's, not the code under test's."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rank_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_pair_audit_cpu import Interaction, Vcol, VcolTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
ALL_ROWS = 4096  # the option's largest row limit: no trace of a reference input is higher (mem of alu(50): 2048 rows)
INPUTS = {"fib1": lambda: va.Workload.fib(1), "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50)}
# fib(25), every chip: the columns the reference finds coupled on some row.  add / sub: the bytes of a, b and c, bound only through
# the carry sums; mul: the product's limbs; lt: the bytes behind the difference bits.
_BYTES = [0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14]
FIB25_COUPLED = {CPU: [], PROGRAM: [], MEM: [7, 8], ADD: _BYTES, SUB: _BYTES, MUL: [8, 9, 10, 11, 12, 13, 14, 15, 16], DIV: [12, 13], SHIFT: [], LT: [1, 2, 3, 5, 6, 7], COM: [],
                 BITWISE: [], OUTPUT: [], RANGE: [], STATIC_DATA: []}
_witness, _reference = {}, {}


def witness(name):
    if name not in _witness:
        w = INPUTS[name]()
        _witness[name] = (w.main_traces(), w.preprocessed())
    return _witness[name]


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def reference(machines, name, **limits):
    if name not in _reference:
        mt, prep = witness(name)
        _reference[name] = ref.audit(machines["basic"], mt, prep, max_entries=1 << 24, max_rows_per_entry=ALL_ROWS)
    return ref.recut(_reference[name], **limits) if limits else ref.recut(_reference[name], 1024, 4)


def both(machines, name, **limits):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, **limits)
    mt, prep = witness(name)
    reps = {k: va.rank_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
def test_fib1_every_chip(machines):
    mt, _ = witness("fib1")
    assert mt[CPU].shape[0] <= 32 and sum(1 for m in mt if m.shape[0] == 1) >= 8  # the height-1 chips: one evaluation, local and next at once
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and rep.total_entries == rep.reported > 0
    for c in rep.chips:
        assert c["pinned_columns"] + c["loose_columns"] == c["width"] and c["nullity"] >= c["zero"] and c["max_nullity"] <= c["width"]


def test_fib25_pinned_coupled_columns(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20)
    assert not rep.truncated and rep.chips[CPU]["height"] == 256
    for chip, cols in FIB25_COUPLED.items():
        assert sorted(e["column"] for e in want["entries"] if e["chip"] == chip) == cols, va.CHIP_NAMES[chip]
        assert rep.coupled_columns(chip) == cols and rep.chips[chip]["coupled_columns"] == len(cols)
        assert set(cols) <= set(rep.loose_columns(chip))
    # the shape the pair audit found for two columns, with its coefficients: a carry sum binds each byte only together with its partner
    e = [e for e in rep.entries if e["chip"] == ADD and e["column"] == 0][0]
    assert e["rows"][0]["n_support"] == 2 and e["rows"][0]["terms"] == [(0, P - 1), (4, 1)]
    for e in rep.entries:
        assert 0 < e["coupled"] <= rep.chips[e["chip"]]["coupled_rows"] <= rep.chips[e["chip"]]["height"]
        assert [r["row"] for r in e["rows"]] == sorted(set(r["row"] for r in e["rows"])) and len(e["rows"]) == min(e["coupled"], 4)


def test_alu50(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20, max_rows_per_entry=7)
    assert {c: rep.chips[c]["height"] for c in (CPU, MEM, ADD, SUB, LT)} == {CPU: 512, MEM: 2048, ADD: 256, SUB: 64, LT: 64}
    assert rep.coupled_columns(CPU) and rep.coupled_columns(ADD) == _BYTES


# ---- 2. analytic AIRs through the capture interface ------------------------------------------------------------------------------------------
SUM3, PROD, STEP, BUS, SQUARE, WIDE = range(6)


def analytic_machine():
    """Six captured AIRs: SUM3 (a, b, c: a + b - c), PROD (a, b, c: a b - c), STEP (x: when_transition next.x - x - 1), BUS (a, b, c, s: no
    constraint, one interaction of count s with the fields (a + b, c)), SQUARE (x: x x) and WIDE (70 columns: x_0 + x_35 - x_69)."""
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0

    def new(name, width):
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
        return air

    def push(air):
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)

    def var(air, col, is_next=0):
        return L.vgpu_air_variable(air, u(0), u(col), u(is_next))

    air = new(b"sum3", 3)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_add(air, u(var(air, 0)), u(var(air, 1)))), u(var(air, 2)))))
    push(air)
    air = new(b"prod", 3)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_mul(air, u(var(air, 0)), u(var(air, 1)))), u(var(air, 2)))))
    push(air)
    air = new(b"step", 1)
    step = L.vgpu_air_sub(air, u(L.vgpu_air_sub(air, u(var(air, 0, 1)), u(var(air, 0)))), u(L.vgpu_air_constant(air, u(1))))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_mul(air, u(L.vgpu_air_is_transition(air)), u(step))))
    push(air)
    air = new(b"bus", 4)
    ab = (VcolTerm * 2)(VcolTerm(0, 0, 1), VcolTerm(0, 1, 1))
    c = (VcolTerm * 1)(VcolTerm(0, 2, 1))
    count = (VcolTerm * 1)(VcolTerm(0, 3, 1))
    fields = (Vcol * 2)(Vcol(ab, 2, 0), Vcol(c, 1, 0))
    it = Interaction(fields, 2, Vcol(count, 1, 0), 0, 0, 1)
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
    push(air)
    air = new(b"square", 1)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_mul(air, u(var(air, 0)), u(var(air, 0)))))
    push(air)
    air = new(b"wide", 70)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_add(air, u(var(air, 0)), u(var(air, 35)))), u(var(air, 69)))))
    push(air)
    return va.Machine(m)


def analytic_traces(n):
    r = np.arange(n, dtype=np.uint32)
    prod = np.stack([np.where(r == 0, 0, 2), np.where(r == 0, 1, 3), np.where(r == 0, 0, 6)], axis=1)  # row 0: a = 0, b = 1, c = 0; else 2 3 = 6
    wide = (np.arange(70, dtype=np.uint32)[None, :] * 3 + r[:, None] + 1)
    return [np.stack([r + 1, 2 * r + 3, 3 * r + 4], axis=1).astype(np.uint32), prod.astype(np.uint32), r[:, None].astype(np.uint32),
            np.stack([r + 2, 5 * r + 1, r + 9, (r + 1) % 2], axis=1).astype(np.uint32), np.zeros((n, 1), dtype=np.uint32), wide.astype(np.uint32)]


def check_analytic(rep, n):
    """The closed forms of the six analytic AIRs at height n (every entry listed: call with max_rows_per_entry >= n)."""
    by = {(e["chip"], e["column"]): e for e in rep.entries}

    def vectors(chip, col):
        return {r["row"]: r["terms"] for r in by[(chip, col)]["rows"]} if (chip, col) in by else {}

    minus = P - 1
    # SUM3: J = [1, 1, -1] on every row
    c = rep.chips[SUM3]
    assert (c["nullity"], c["zero"], c["coupled_rows"], c["max_nullity"], c["pinned_columns"], c["coupled_columns"]) == (2 * n, 0, n, 2, 0, 3)
    assert c["loose"] == [n] * 3 and c["zeros"] == [0] * 3
    for col, v in ((0, [(0, minus), (1, 1)]), (1, [(0, minus), (1, 1)]), (2, [(0, 1), (2, 1)])):
        assert vectors(SUM3, col) == {r: v for r in range(n)} and all(x["n_support"] == 2 for x in by[(SUM3, col)]["rows"])
    # PROD: row 0 (a = 0, b = 1): J = [1, 0, -1]: column 1 is zero, columns 0 and 2 trade through the smallest non-pivot column WITH an entry
    c = rep.chips[PROD]
    assert (c["nullity"], c["zero"], c["coupled_rows"]) == (2 * n, 1, n) and c["loose"] == [n] * 3 and c["zeros"] == [0, 1, 0]
    assert vectors(PROD, 0)[0] == [(0, 1), (2, 1)] and vectors(PROD, 2)[0] == [(0, 1), (2, 1)] and 0 not in vectors(PROD, 1)
    inv3 = pow(3, P - 2, P)
    for r in range(1, n):  # J = [3, 2, -1]: R = [1, 2/3, -1/3]
        assert vectors(PROD, 0)[r] == vectors(PROD, 1)[r] == [(0, (P - 2 * inv3 % P) % P), (1, 1)] and vectors(PROD, 2)[r] == [(0, inv3), (2, 1)]
    # STEP: pinned on every row (row 0 through its local read only, row n - 1 through its next read only); n = 1: is_transition is 0
    c = rep.chips[STEP]
    if n == 1:
        assert (c["nullity"], c["zero"], c["coupled_rows"], c["loose"], c["zeros"], c["coupled_columns"]) == (1, 1, 0, [1], [1], 0)
    else:
        assert (c["nullity"], c["zero"], c["coupled_rows"], c["loose"], c["zeros"], c["pinned_columns"]) == (0, 0, 0, [0], [0], 1)
    # BUS: s = (r + 1) % 2.  Live rows: count row e_3, field rows [1, 1, 0, 0] and e_2: rank 3; other rows: only e_3
    live = [r for r in range(n) if (r + 1) % 2]
    c = rep.chips[BUS]
    assert c["constraints"] == 0 and c["interactions"] == 1
    assert (c["nullity"], c["zero"], c["coupled_rows"]) == (len(live) + 3 * (n - len(live)), 3 * (n - len(live)), len(live))
    assert c["loose"] == [n, n, n - len(live), 0] and c["zeros"] == [n - len(live)] * 3 + [0]
    if live:
        assert vectors(BUS, 0) == vectors(BUS, 1) == {r: [(0, minus), (1, 1)] for r in live} and (BUS, 2) not in by and (BUS, 3) not in by
    # SQUARE at x = 0: reported zero and loose although x is bound — the documented first-order limitation
    c = rep.chips[SQUARE]
    assert (c["nullity"], c["zero"], c["coupled_rows"], c["loose"], c["zeros"]) == (n, n, 0, [n], [n]) and (SQUARE, 0) not in by
    # WIDE: columns beyond lane 63
    c = rep.chips[WIDE]
    assert (c["nullity"], c["zero"], c["coupled_rows"], c["max_nullity"], c["coupled_columns"]) == (69 * n, 67 * n, n, 69, 3)
    assert rep.coupled_columns(WIDE) == [0, 35, 69] and len(rep.loose_columns(WIDE)) == 70
    assert vectors(WIDE, 69) == {r: [(0, 1), (69, 1)] for r in range(n)} and vectors(WIDE, 0) == vectors(WIDE, 35) == {r: [(0, minus), (35, 1)] for r in range(n)}


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(n):
    rep = va.rank_audit_host(analytic_machine(), analytic_traces(n), [], max_rows_per_entry=8)
    check_analytic(rep, n)


# ---- 3. options -------------------------------------------------------------------------------------------------------------------------------
def _host_raw(machine, mt, opts):
    """vgpu_rank_audit_host with a raw options pointer (None: NULL); (status, words)."""
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    n = len(mains)
    h = ctypes.c_void_p()
    rc = L.vgpu_rank_audit_host(machine._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * 1)(), (ctypes.c_void_p * 1)(), (ctypes.c_uint64 * 1)(),
                                (ctypes.c_uint64 * 1)(), ctypes.c_uint32(0), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
    return rc, (va._rank_report(h).words if rc == 0 else None)


def test_limits_and_truncation_keep_exact_totals(machines):
    full, _ = both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=ALL_ROWS)
    want, rep = both(machines, "fib25", max_entries=5, max_rows_per_entry=2)
    assert rep.truncated and rep.reported == 5 and rep.total_entries == full["total_entries"] > 5
    assert rep.chips == [c for c in ref.recut(full)["chips"]] and all(len(e["rows"]) == min(2, e["coupled"]) for e in rep.entries)
    assert [(e["chip"], e["column"]) for e in rep.entries] == sorted((e["chip"], e["column"]) for e in full["entries"])[:5]
    both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=300)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    full = reference(machines, "fib25")
    rep = va.rank_audit_host(machines["basic"], mt, prep, chips=[ADD, LT])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [ADD, LT]
    for c in rep.chips:
        if c["audited"]:
            assert c == full["chips"][c["chip"]]
        else:  # a zero block that keeps the shape
            assert (c["nullity"], c["zero"], c["coupled_rows"], c["max_nullity"], c["loose_columns"], c["pinned_columns"], c["coupled_columns"]) == (0,) * 7
            assert not any(c["loose"]) and not any(c["zeros"]) and (c["width"], c["height"]) == (full["chips"][c["chip"]]["width"], full["chips"][c["chip"]]["height"])
    assert rep.entries == [e for e in full["entries"] if e["chip"] in (ADD, LT)]
    with pytest.raises(va.VgpuError, match="chip_mask names a chip") as e:
        va.rank_audit_host(machines["basic"], mt, prep, chips=[20])
    assert e.value.code == -1


def test_reserved_null_and_defaults():
    machine, mt = analytic_machine(), analytic_traces(8)
    want = va.rank_audit_host(machine, mt, []).words
    rc, words = _host_raw(machine, mt, None)  # NULL opts: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = _host_raw(machine, mt, va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(0, 0)))  # zero fields select the defaults
    assert rc == 0 and np.array_equal(words, want)
    for bad in (va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(1, 0)), va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(0, 7)), va.RankAuditOpts((1 << 24) + 1, 0, 0, (ctypes.c_uint32 * 2)(0, 0)),
                va.RankAuditOpts(0, 4097, 0, (ctypes.c_uint32 * 2)(0, 0)), va.RankAuditOpts(0, 0, 1 << 6, (ctypes.c_uint32 * 2)(0, 0))):
        rc, _ = _host_raw(machine, mt, bad)
        assert rc == -1 and b"rank_audit" in va.lib().vgpu_last_error()
    with pytest.raises(va.VgpuError, match="at least 1"):
        va.rank_audit_host(machine, mt, [], max_entries=0)
    assert np.array_equal(va.rank_audit_host(machine, mt, []).words, want)  # the same words run after run


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "rank_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "librankauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "rank_audit.hpp"), os.path.join(csrc, "host", "mutation_audit.hpp"),
            os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("rank_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_rank_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, rows_per_wave=0, max_entries=1024, max_rows_per_entry=4, chips=None):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(8 + sum(16 + 4 * m.shape[1] for m in keep[:n]) + min(max_entries, 1024) * (6 + 18 * min(max_rows_per_entry, 4096)), np.uint32)
    got = emu.emu_rank_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(rows_per_wave), ctypes.c_uint32(max_entries), ctypes.c_uint32(max_rows_per_entry), ctypes.c_uint32(sum(1 << c for c in chips) if chips else 0),
        out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """Counting pass, scan and listing pass of rank_audit.hip with its wave primitives in their emulation forms (a wave is a 64-thread
    workgroup): the compiled chip templates, the interpreted dual register programs and the bus-only chips; the assembled report is the host
    audit's, word for word.  fib(1) without mul (1024 rows; the emulated ballots are slow): every other chip, bitwise with its 79 columns (more
    than one word per lane), the height-1 chips, rows that end early at full rank (cpu, range) and rows that do not.  With 3 rows per
    workgroup cpu (32 rows), mem (64) and add (16) span many workgroups: the r - 1 halo, the wrap between row 0 and row n - 1 and the rank
    scan cross workgroup boundaries (mem's columns 7 and 8 have 23 coupled rows: lists of 20 run over several workgroups).
    NOT covered here: a workgroup is one wave under emulation (NW = 1), so the listing pass's exchange BETWEEN the waves of a workgroup — the
    coupled bits cb[wave][column], rank += cb[k][column] for the waves k before, the running[] update between the three __syncthreads() —
    never runs on the CPU with more than one wave.  Only tests/test_rank_audit_gpu.py covers it, where NW is 2 or 4 (fib(582), lists of 300)."""
    mt, prep = witness("fib1")
    chips = [c for c in range(14) if c != MUL]
    host = va.rank_audit_host(machines["basic"], mt, prep, chips=chips)
    assert host.chips[CPU]["nullity"] < 26 * 32 and host.chips[RANGE]["max_nullity"] == 1
    assert np.array_equal(emulated(emu, mt, prep, interpret, chips=chips), host.words)
    some = [CPU, MEM, ADD, BITWISE, RANGE]
    host = va.rank_audit_host(machines["basic"], mt, prep, chips=some, max_rows_per_entry=20, max_entries=9)
    assert host.truncated and any(len(e["rows"]) == 20 and e["rows"][-1]["row"] - e["rows"][0]["row"] > 6 for e in host.entries if e["chip"] == MEM)
    assert np.array_equal(emulated(emu, mt, prep, interpret, rows_per_wave=3, chips=some, max_rows_per_entry=20, max_entries=9), host.words)


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_rank_on_the_host(tmp_path, machines):
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out, "--host")
    plain_json = json.loads(out.read_text())
    r = _cli("check", bl, out, "--host", "--rank")
    assert r.returncode == plain.returncode == 0, r.stderr  # a coupled column is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.rank_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    chips = [c for c in rep.chips if c["coupled_columns"]]
    assert chips and len(lines) == len(before) + len(chips)
    for line, c in zip(lines[len(before):], chips):
        cols = rep.coupled_columns(c["chip"])
        assert line.startswith("%s: %d coupled column%s: %d" % (va.CHIP_NAMES[c["chip"]], len(cols), "" if len(cols) == 1 else "s", cols[0]))
        assert ("max nullity %d; %d coupled row" % (c["max_nullity"], c["coupled_rows"])) in line
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"rank"} and {k: v for k, v in j.items() if k not in ("rank", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["rank"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--rank", "--chips=add,4")
    assert r.returncode == 0 and [c["chip"] for c in json.loads(out.read_text())["rank"]["chips"] if c["audited"]] == [ADD, SUB]


# ---- 6. C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_rank_audit", "vgpu_rank_audit_host", "vgpu_rank_report_len", "vgpu_rank_report_words", "vgpu_rank_report_timing", "vgpu_rank_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Rank audit" in header and "vgpu_rank_audit_opts_t" in header
