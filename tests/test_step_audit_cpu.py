"""The step audit without a GPU: the host implementation of the contract (vgpu_step_audit_host) against the restatement of
tests/step_audit_ref.py (the rank audit reference's directions, the mutation audit reference's judgement) word for word, for both machine kinds;
the analytic AIRs of tests/test_rank_audit_cpu.py with their closed forms; certificates (a listed exact row applied to the trace leaves the
constraint audit and the bus audit as they were, a listed curved row makes a constraint fail); options; the device kernels' very source under
tools/hipemu; `check --steps` on the command line; the C ABI's new symbols; the host audit under AddressSanitizer and UBSan as a stand-alone
program.  The reference of each input is computed once per module and cut to the limits a test asks for.  The confirmed and refuted columns
pinned here are the reference's, not the code under test's."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import step_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import (ADD, BITWISE, BUS, COM, CPU, DIV, LT, MEM, MUL, PROD, RANGE, SQUARE, STEP, SUB, SUM3, WIDE, analytic_machine, analytic_traces)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
ALL_ROWS = 4096
INPUTS = {"fib1": lambda: va.Workload.fib(1), "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50)}
# fib(25), every chip, default steps: the columns the reference finds confirmed (coupled and exact on some row) and refuted (curved on some
# row).  Confirmed: exactly the rank audit's coupled columns of the ALU chips and mem — the limb trades are real.  Refuted: cpu's
# memory-value columns on the rows where a quadratic selector product makes them look free, and com's operand bytes on its one dummy row.
_BYTES = [0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14]
FIB25_CONFIRMED = {CPU: [], 1: [], MEM: [7, 8], ADD: _BYTES, SUB: _BYTES, MUL: [8, 9, 10, 11, 12, 13, 14, 15, 16], DIV: [12, 13], 7: [], LT: [1, 2, 3, 5, 6, 7], COM: [], BITWISE: [], 11: [],
                   RANGE: [], 13: []}
FIB25_REFUTED = {CPU: [5, 6, 7, 8, 32, 33, 34, 35, 39, 40, 41, 42], COM: [0, 1, 2, 3, 4, 5, 6, 7]}
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
    """The reference's report and the host audit's under both machine kinds: equal word for word; the bus rule never detects."""
    want = reference(machines, name, **limits)
    mt, prep = witness(name)
    reps = {k: va.step_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
        assert all(c["bus"] == 0 for c in rep.chips)
    return want, reps["basic"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
def test_fib1_every_chip(machines):
    mt, prep = witness("fib1")
    four = (1, P - 1, 2, P - 2)  # four steps, p - 2 among them
    want4 = ref.audit(machines["basic"], mt, prep, steps=four)
    for m in machines.values():
        assert np.array_equal(va.step_audit_host(m, mt, prep, steps=four).words, ref.words(want4))
    want, rep = both(machines, "fib1")
    assert all(c["audited"] and c["line_exact"] for c in rep.chips) and rep.total_entries == rep.reported > 0 and rep.steps == [1, P - 1, 2]
    for c in rep.chips:
        assert c["max_degree"] <= 3 and c["zero_cells"] <= c["loose_cells"] and c["coupled_exact_cells"] <= c["exact_cells"] <= c["loose_cells"]
        assert c["passes"][0] >= c["exact_cells"] and c["confirmed_rows"] <= c["height"] and c["refuted_rows"] <= c["height"]


def test_fib25_pinned_confirmed_and_refuted_columns(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20)
    assert not rep.truncated
    for chip in range(14):
        assert ref.confirmed_columns(want, chip) == FIB25_CONFIRMED[chip], va.CHIP_NAMES[chip]
        assert ref.refuted_columns(want, chip) == FIB25_REFUTED.get(chip, []), va.CHIP_NAMES[chip]
        assert rep.confirmed_columns(chip) == FIB25_CONFIRMED[chip] and rep.refuted_columns(chip) == FIB25_REFUTED.get(chip, [])
    # the pair audit's trade, now with a certificate: the carry sum binds each byte only together with its partner, at every step
    e = [e for e in rep.entries if e["chip"] == ADD and e["column"] == 0][0]
    assert e["rows"][0]["terms"] == [(0, P - 1), (4, 1)] and e["rows"][0]["pass_mask"] == 7 and e["rows"][0]["exact"] and not e["rows"][0]["zero"]
    for e in rep.entries:
        rows = [r["row"] for r in e["rows"]]
        assert rows == sorted(set(rows)) and len(rows) == min(e["coupled_exact"] + e["curved"], 4) and e["coupled_exact"] + e["curved"] > 0
        assert all(not r["zero"] or not r["exact"] for r in e["rows"])  # zero-and-exact rows are counted, never listed


def test_alu50(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20, max_rows_per_entry=7)
    assert {c: rep.chips[c]["height"] for c in (CPU, MEM, ADD, SUB, LT)} == {CPU: 512, MEM: 2048, ADD: 256, SUB: 64, LT: 64}
    assert rep.confirmed_columns(ADD) == _BYTES and rep.chips[ADD]["confirmed_rows"] > 0


# ---- 2. analytic AIRs through the capture interface ------------------------------------------------------------------------------------------
def check_step_analytic(rep, n, steps=3):
    """The closed forms of the six analytic AIRs at height n (every listable row listed: call with max_rows_per_entry >= n)."""
    by = {(e["chip"], e["column"]): e for e in rep.entries}
    full = (1 << steps) - 1
    inv3 = pow(3, P - 2, P)

    def rows(chip, col):
        return {r["row"]: r for r in by[(chip, col)]["rows"]} if (chip, col) in by else {}

    c = rep.chips[SUM3]
    assert c["loose"] == c["exact"] == c["coupled_exact"] == [n] * 3 and c["zeros"] == [0] * 3 and (c["confirmed_rows"], c["refuted_rows"]) == (n, 0)
    assert c["passes"] == [3 * n] * steps and c["max_degree"] == 1
    assert all(r["pass_mask"] == full and r["terms"] == [(0, 1), (2, 1)] for r in rows(SUM3, 2).values()) and len(rows(SUM3, 2)) == n
    # PROD: row 0 (0, 1, 0): column 1 zero and exact, columns 0 and 2 exact; rows >= 1 (2, 3, 6): columns 0 and 1 share [(0, -2/3), (1, 1)] and
    # are curved at every step (residue -2 t^2 / 3), column 2 with [(0, 1/3), (2, 1)] is exact
    c = rep.chips[PROD]
    assert c["loose"] == [n] * 3 and c["zeros"] == [0, 1, 0] and c["exact"] == [1, 1, n] and c["coupled_exact"] == [1, 0, n]
    assert [c["loose"][k] - c["exact"][k] for k in range(3)] == [n - 1, n - 1, 0] and (c["confirmed_rows"], c["refuted_rows"]) == (n, n - 1) and c["max_degree"] == 2
    assert 0 not in rows(PROD, 1) and rows(PROD, 0)[0]["pass_mask"] == full and rows(PROD, 0)[0]["terms"] == [(0, 1), (2, 1)]
    for r in range(1, n):
        for col in (0, 1):
            assert rows(PROD, col)[r]["pass_mask"] == 0 and rows(PROD, col)[r]["terms"] == [(0, (P - 2 * inv3 % P) % P), (1, 1)] and not rows(PROD, col)[r]["zero"]
        assert rows(PROD, 2)[r]["pass_mask"] == full and rows(PROD, 2)[r]["terms"] == [(0, inv3), (2, 1)]
    # STEP: n = 1 zero and exact (is_transition is 0); n > 1 no loose column
    c = rep.chips[STEP]
    assert (c["loose"], c["zeros"], c["exact"], c["coupled_exact"]) == (([1], [1], [1], [0]) if n == 1 else ([0], [0], [0], [0])) and (STEP, 0) not in by
    # BUS: exact = loose = [n, n, n - live, 0]; no evaluation
    live = len([r for r in range(n) if (r + 1) % 2])
    c = rep.chips[BUS]
    assert c["loose"] == c["exact"] == [n, n, n - live, 0] and c["coupled_exact"] == [live, live, 0, 0] and c["max_degree"] == 0 and (c["confirmed_rows"], c["refuted_rows"]) == (live, 0)
    # SQUARE at x = 0: the rank audit's documented false positive, now refuted on every row
    c = rep.chips[SQUARE]
    assert (c["loose"], c["zeros"], c["exact"], c["refuted_rows"], c["passes"]) == ([n], [n], [0], n, [0] * steps)
    assert sorted(rows(SQUARE, 0)) == list(range(n)) and all(r["pass_mask"] == 0 and r["zero"] and r["terms"] == [(0, 1)] and r["n_support"] == 1 for r in rows(SQUARE, 0).values())
    # WIDE: 69 non-pivot columns, 207 items per row at three steps; columns beyond lane 63
    c = rep.chips[WIDE]
    assert c["loose"] == c["exact"] == [n] * 70 and sum(c["zeros"]) == 67 * n and rep.confirmed_columns(WIDE) == [0, 35, 69] and c["passes"] == [70 * n] * steps
    assert all(r["terms"] == [(0, 1), (69, 1)] and r["pass_mask"] == full for r in rows(WIDE, 69).values()) and len(rows(WIDE, 69)) == n
    assert all(ch["line_exact"] == (steps >= ch["max_degree"]) for ch in rep.chips) and all(ch["bus"] == 0 for ch in rep.chips)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(n):
    rep = va.step_audit_host(analytic_machine(), analytic_traces(n), [], max_rows_per_entry=8)
    check_step_analytic(rep, n)
    assert all(c["line_exact"] for c in rep.chips)
    one = va.step_audit_host(analytic_machine(), analytic_traces(n), [], steps=[1], max_rows_per_entry=8)
    assert not one.chips[PROD]["line_exact"] and not one.chips[SQUARE]["line_exact"] and one.chips[SUM3]["line_exact"] and one.chips[BUS]["line_exact"]


# ---- 3. certificates --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib25", "alu50"])
def test_certificates(machines, name):
    """A listed exact row applied at each step: a different trace on which the constraint audit and the bus audit say what they said before.  A
    listed curved row applied at a failing step: a constraint of that chip fails at row r or r - 1."""
    m = machines["basic"]
    mt, prep = witness(name)
    rep = va.step_audit_host(m, mt, prep, max_entries=1 << 20, max_rows_per_entry=2)
    c0, b0 = va.constraint_audit_host(m, mt, prep, max_constraints=4096, max_rows_per_constraint=64).words, va.bus_audit_host(m, mt, prep).words
    exact = [(e, k) for e in rep.entries for k, r in enumerate(e["rows"]) if r["exact"] and r["n_support"] <= 8][:64]
    curved = [(e, k) for e in rep.entries for k, r in enumerate(e["rows"]) if not r["exact"] and r["n_support"] <= 8][:64]
    assert exact and curved
    for e, k in exact:
        for s in range(len(rep.steps)):
            moved = list(mt)
            moved[e["chip"]] = rep.apply(mt, e, k, s)
            assert not np.array_equal(moved[e["chip"]], mt[e["chip"]])
            assert np.array_equal(va.constraint_audit_host(m, moved, prep, max_constraints=4096, max_rows_per_constraint=64).words, c0), (e["chip"], e["column"], e["rows"][k], s)
            assert np.array_equal(va.bus_audit_host(m, moved, prep).words, b0)
    for e, k in curved:
        row = e["rows"][k]
        s = [s for s in range(len(rep.steps)) if not (row["pass_mask"] >> s) & 1][0]
        moved = list(mt)
        moved[e["chip"]] = rep.apply(mt, e, k, s)
        got = va.constraint_audit_host(m, moved, prep, max_constraints=4096, max_rows_per_constraint=64)
        n = mt[e["chip"]].shape[0]
        assert any(c["chip"] == e["chip"] and any(r in (row["row"], (row["row"] - 1) % n) for r, _ in c["rows"]) for c in got.constraints), (e["chip"], e["column"], row)


def test_apply_refuses_a_cut_vector(machines):
    mt, prep = witness("fib25")
    rep = va.step_audit_host(machines["basic"], mt, prep, max_entries=1 << 20)
    e = dict(chip=ADD, column=0, rows=[dict(row=0, n_support=9, terms=[(k, 1) for k in range(8)])])
    with pytest.raises(va.VgpuError, match="is cut"):
        rep.apply(mt, e, 0, 0)


# ---- 4. options -------------------------------------------------------------------------------------------------------------------------------
def _opts(max_entries=0, rows=0, mask=0, steps=(), reserved=(0, 0, 0)):
    return va.StepAuditOpts(max_entries, rows, mask, len(steps), (ctypes.c_uint32 * 4)(*steps), (ctypes.c_uint32 * 3)(*reserved))


def _host_raw(machine, mt, opts):
    """vgpu_step_audit_host with a raw options pointer (None: NULL); (status, words)."""
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    n = len(mains)
    h = ctypes.c_void_p()
    rc = L.vgpu_step_audit_host(machine._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * 1)(), (ctypes.c_void_p * 1)(), (ctypes.c_uint64 * 1)(),
                                (ctypes.c_uint64 * 1)(), ctypes.c_uint32(0), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
    return rc, (va._step_report(h).words if rc == 0 else None)


def test_limits_and_truncation_keep_exact_totals(machines):
    full, _ = both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=ALL_ROWS)
    want, rep = both(machines, "fib25", max_entries=5, max_rows_per_entry=2)
    assert rep.truncated and rep.reported == 5 and rep.total_entries == full["total_entries"] > 5
    assert rep.chips == ref.recut(full)["chips"] and all(len(e["rows"]) == min(2, e["coupled_exact"] + e["curved"]) for e in rep.entries)
    assert [(e["chip"], e["column"]) for e in rep.entries] == sorted((e["chip"], e["column"]) for e in full["entries"])[:5]
    both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=300)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    full = reference(machines, "fib25")
    rep = va.step_audit_host(machines["basic"], mt, prep, chips=[ADD, LT])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [ADD, LT]
    for c in rep.chips:
        if c["audited"]:
            assert c == full["chips"][c["chip"]]
        else:  # a zero block that keeps the shape
            assert (c["loose_cells"], c["exact_cells"], c["confirmed_rows"], c["refuted_rows"], c["line_exact"]) == (0, 0, 0, 0, False) and not any(c["loose"]) and not any(c["passes"])
            assert (c["width"], c["height"], c["max_degree"]) == tuple(full["chips"][c["chip"]][k] for k in ("width", "height", "max_degree"))
    assert rep.entries == [e for e in full["entries"] if e["chip"] in (ADD, LT)]
    with pytest.raises(va.VgpuError, match="step_audit: chip_mask names a chip") as e:
        va.step_audit_host(machines["basic"], mt, prep, chips=[20])
    assert e.value.code == -1


def test_steps_reserved_null_and_defaults():
    machine, mt = analytic_machine(), analytic_traces(8)
    want = va.step_audit_host(machine, mt, []).words
    rc, words = _host_raw(machine, mt, None)  # NULL opts: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = _host_raw(machine, mt, _opts())  # zero fields select the defaults
    assert rc == 0 and np.array_equal(words, want)
    assert np.array_equal(va.step_audit_host(machine, mt, [], steps=[1, P - 1, 2]).words, want)
    for bad, match in ((_opts(reserved=(1, 0, 0)), b"reserved"), (_opts(reserved=(0, 0, 7)), b"reserved"), (_opts(max_entries=(1 << 24) + 1), b"max_entries"), (_opts(rows=4097), b"max_rows_per_entry"),
                       (_opts(mask=1 << 6), b"chip_mask"), (_opts(steps=(1, 1)), b"distinct"), (_opts(steps=(1, 0)), b"1..p-1"), (_opts(steps=(P,)), b"1..p-1")):
        rc, _ = _host_raw(machine, mt, bad)
        assert rc == -1 and va.lib().vgpu_last_error().startswith(b"step_audit:") and match in va.lib().vgpu_last_error(), va.lib().vgpu_last_error()
    bad = _opts(steps=(1, 2, 3, 4))
    bad.n_steps = 5
    rc, _ = _host_raw(machine, mt, bad)
    assert rc == -1 and b"at most 4 steps" in va.lib().vgpu_last_error()
    with pytest.raises(va.VgpuError, match="at least 1"):
        va.step_audit_host(machine, mt, [], max_entries=0)
    with pytest.raises(va.VgpuError, match="1 to 4 steps"):
        va.step_audit_host(machine, mt, [], steps=[])
    four = va.step_audit_host(machine, mt, [], steps=[1, P - 1, 2, P - 2], max_rows_per_entry=8)
    check_step_analytic(four, 8, steps=4)
    assert four.steps == [1, P - 1, 2, P - 2] and four.chips[PROD]['passes'][3] == four.chips[PROD]['passes'][0]
    assert np.array_equal(va.step_audit_host(machine, mt, []).words, want)  # the same words run after run


def test_shape_errors_carry_the_audits_name(machines):
    mt, prep = witness("fib25")
    for match, kw in (("one main trace per chip", dict(mt=mt[:-1])), ("needs its preprocessed trace", dict(prep=prep[:1]))):
        with pytest.raises(va.VgpuError, match="step_audit: .*" + match) as e:
            va.step_audit_host(machines["basic"], kw.get("mt", mt), kw.get("prep", prep))
        assert e.value.code == -1
    with pytest.raises(va.VgpuError, match="step_audit: traces are two-dimensional"):
        va.step_audit_host(machines["basic"], [m.ravel() for m in mt], prep)


# ---- 5. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "step_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libstepauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "step_audit.hpp"), os.path.join(csrc, "host", "rank_audit.hpp"),
            os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("step_audit.hip", "rank_elim.hpp", "rank_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_step_audit.restype = ctypes.c_int64
    return L


def emulated(emu, machine_kind, mt, prep, interpret, rows_per_wave=0, max_entries=1024, max_rows_per_entry=4, chips=None, steps=()):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(14 + sum(30 + 8 * m.shape[1] for m in keep[:n]) + min(max_entries, 1024) * (8 + 20 * min(max_rows_per_entry, 4096)), np.uint32)
    got = emu.emu_step_audit(
        ctypes.c_uint32(machine_kind), (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]),
        (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]), ctypes.c_uint32(n), (ctypes.c_uint32 * max(1, k))(*[c for c, _ in prep]), (ctypes.c_void_p * max(1, k))(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * max(1, k))(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * max(1, k))(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(rows_per_wave), ctypes.c_uint32(max_entries), ctypes.c_uint32(max_rows_per_entry), ctypes.c_uint32(sum(1 << c for c in chips) if chips else 0),
        (ctypes.c_uint32 * 4)(*steps), ctypes.c_uint32(len(steps)), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """Counting pass, scan and listing pass of step_audit.hip (with rank_elim.hpp and the rank audit's scan kernel) with the wave primitives in
    their emulation forms (a wave is a 64-thread workgroup): the compiled chip templates, the interpreted register programs and the bus-only
    chips; the assembled report is the host audit's, word for word.  fib(1) without mul (1024 rows; the emulated ballots are slow): cpu's
    curved columns (pass masks below all-ones), bitwise with its 79 columns (more than one word per lane), the height-1 chips (one evaluation,
    the moved row local and next at once), rows that end early at full rank (no item) and rows that do not.  With 3 rows per workgroup cpu
    (32 rows), mem (64) and add (16) span many workgroups: the r - 1 halo, the wrap between row 0 and row n - 1 and the rank scan cross
    workgroup boundaries (cpu's twelve refuted columns, then mem's column 7 with a list of 20 rows over several workgroups; the list is cut there).
    NOT covered here: a workgroup is one wave under emulation (NW = 1), so the listing pass's exchange BETWEEN the waves of a workgroup — the
    listable bits cb[wave][column], rank += cb[k][column] for the waves k before, the running[] update between the __syncthreads() — never
    runs on the CPU with more than one wave.  Only tests/test_step_audit_gpu.py covers it, where NW is 2 or 4 (fib(582), lists of 300)."""
    mt, prep = witness("fib1")
    chips = [c for c in range(14) if c != MUL]
    host = va.step_audit_host(machines["basic"], mt, prep, chips=chips)
    assert host.refuted_columns(CPU) and host.confirmed_columns(MEM) == [7, 8]
    assert np.array_equal(emulated(emu, 0, mt, prep, interpret, chips=chips), host.words)
    some = [CPU, MEM, ADD, BITWISE, RANGE]
    host = va.step_audit_host(machines["basic"], mt, prep, chips=some, max_rows_per_entry=20, max_entries=13)
    assert host.truncated and any(len(e["rows"]) == 20 and e["rows"][-1]["row"] - e["rows"][0]["row"] > 6 for e in host.entries if e["chip"] in (CPU, MEM))
    assert np.array_equal(emulated(emu, 0, mt, prep, interpret, rows_per_wave=3, chips=some, max_rows_per_entry=20, max_entries=13), host.words)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs_under_emulation(emu, n):
    """The six analytic AIRs through the interpreted register program: WIDE has 207 items per row (four passes of 64 lanes) and columns
    beyond lane 63; SQUARE and PROD have curved cells; BUS evaluates nothing.  n = 8 with 3 rows per workgroup; four steps too."""
    machine, mt = analytic_machine(), analytic_traces(n)
    host = va.step_audit_host(machine, mt, [], max_rows_per_entry=8)
    got = emulated(emu, 1, mt, [], 1, rows_per_wave=3 if n == 8 else 0, max_rows_per_entry=8)
    assert np.array_equal(got, host.words)
    check_step_analytic(va.StepReport(got), n)
    st = [1, P - 1, 2, P - 2]
    assert np.array_equal(emulated(emu, 1, mt, [], 1, max_rows_per_entry=8, steps=st), va.step_audit_host(machine, mt, [], steps=st, max_rows_per_entry=8).words)
    assert np.array_equal(emulated(emu, 1, mt, [], 1, max_rows_per_entry=8, steps=[5]), va.step_audit_host(machine, mt, [], steps=[5], max_rows_per_entry=8).words)


# ---- 6. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_steps_on_the_host(tmp_path, machines):
    from valida_amd.cli import index_ranges

    bl, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out_plain, "--host")
    r = _cli("check", bl, out, "--host", "--steps")
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.step_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    expect = []
    for c in rep.chips:
        conf, refuted = rep.confirmed_columns(c["chip"]), rep.refuted_columns(c["chip"])
        parts = []
        if conf:
            parts.append("confirmed columns %s on %d rows" % (index_ranges(conf), c["confirmed_rows"]) + (" (whole lines: degree %d <= 3 steps)" % c["max_degree"] if c["line_exact"] else ""))
        if refuted:
            parts.append("refuted columns %s on %d rows" % (index_ranges(refuted), c["refuted_rows"]))
        if parts:
            expect.append("%s: %s" % (va.CHIP_NAMES[c["chip"]], "; ".join(parts)))
    assert expect and lines[len(before):] == expect and any("(whole lines: degree" in x for x in expect) and any("refuted" in x for x in expect)
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    # without the flag `check` prints and writes what it did before: the plain run's lines come first unchanged, its keys and values are all there
    assert set(j) == set(plain_json) | {"steps"} and "steps" not in plain_json and "confirmed" not in plain.stdout and {k: v for k, v in j.items() if k not in ("steps", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["steps"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--steps", "--step-sizes=1", "--chips=add,4")
    j = json.loads(out.read_text())["steps"]
    assert r.returncode == 0 and [c["chip"] for c in j["chips"] if c["audited"]] == [ADD, SUB] and j["steps"] == [1]
    assert "whole lines" not in r.stdout and "sub: confirmed columns 0-7, 11-14 on 1 rows\n" in r.stdout  # sub has degree 3: one step does not give the line


# ---- 7. C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_step_audit", "vgpu_step_audit_host", "vgpu_step_report_len", "vgpu_step_report_words", "vgpu_step_report_timing", "vgpu_step_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Step audit" in header and "vgpu_step_audit_opts_t" in header and ctypes.sizeof(va.StepAuditOpts) == 48


# ---- 8. the host audit under the sanitizers, as a program of its own ----------------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path, machines):
    """tests/emu/step_audit_host.cpp: fib(25) on the host VM and the host step audit, built with AddressSanitizer and UBSan and run as a
    subprocess (nothing sanitized is loaded into this interpreter).  Its word count is the library's for the same limits."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "step_audit_host")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "emu", "step_audit_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe, "25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    mt, prep = witness("fib25")
    rep = va.step_audit_host(machines["basic"], mt, prep, max_entries=1 << 20, max_rows_per_entry=64)
    assert ("fib(25): %d words, %d entries, %d loose cells, %d exact cells, 0 bus-detected" % (
        len(rep.words), rep.total_entries, sum(c["loose_cells"] for c in rep.chips), sum(c["exact_cells"] for c in rep.chips))) in r.stdout, r.stdout
