"""The field audit without a GPU: the host implementation of the contract (vgpu_field_audit_host) against the restatement of
tests/field_audit_ref.py (exact interpolation of the oracle's own chip transcription, one numpy RREF per field) word for word, for both machine
kinds; analytic AIRs captured through vgpu_air_* whose answers are known in closed form; options; the device kernels' very source under
tools/hipemu; `check --fields` on the command line; the C ABI's new symbols.  The reference of each input is computed once per module and cut
to the limits a test asks for (counts do not depend on them).  The floating fields pinned here are the reference's, not the code under test's."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_pair_audit_cpu import Interaction, Vcol, VcolTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
ALL_ROWS = 4096  # the option's largest row limit: no trace of a reference input is higher (mem of alu(50): 2048 rows)
INPUTS = {"fib1": lambda: va.Workload.fib(1), "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "mixed_ops": lambda: va.Workload.named("mixed_ops:3")}
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
    reps = {k: va.field_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


def floating_of(want, chip):
    """{(interaction, field): rows} of the reference's dict."""
    return {(r["interaction"], j): n for r in want["chips"][chip]["records"] for j, n in enumerate(r["floating"]) if n}


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
def test_fib1_every_chip(machines):
    mt, _ = witness("fib1")
    assert sum(1 for m in mt if m.shape[0] == 1) >= 8  # the height-1 chips: one evaluation, local and next at once
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and rep.total_entries == rep.reported > 0
    for c in rep.chips:
        assert c["floating_rows"] <= c["height"] and c["floating_fields"] == sum(sum(r["floating"]) for r in c["records"]) and c["live_records"] == sum(r["live_rows"] for r in c["records"])


def test_fib25(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20)
    assert not rep.truncated and rep.chips[CPU]["height"] == 256
    for e in rep.entries:
        rec = rep.chips[e["chip"]]["records"][e["interaction"]]
        assert 0 < e["floating"] == rec["floating"][e["field"]] <= rec["live_rows"] and not rec["constant"][e["field"]]
        assert [r["row"] for r in e["rows"]] == sorted(set(r["row"] for r in e["rows"])) and len(e["rows"]) == min(e["floating"], 4)


def test_alu50(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20, max_rows_per_entry=7)
    assert {c: rep.chips[c]["height"] for c in (CPU, MEM, ADD, SUB, LT)} == {CPU: 512, MEM: 2048, ADD: 256, SUB: 64, LT: 64}


def test_mixed_ops_what_the_reference_finds(machines):
    """The chips the reference leaves as `// TODO` or without constraints, as the reference of this audit sees them."""
    want, rep = both(machines, "mixed_ops", max_entries=1 << 20)
    chips = want["chips"]
    # div: no constraints; the opcode row 103 e12 + 110 e13 is independent of the count row e12 + e13: all 13 fields of its receive float
    d = chips[DIV]
    assert d["constraints"] == 0 and len(d["records"]) == 1 and d["records"][0]["fields"] == 13 and not d["records"][0]["is_send"]
    assert d["records"][0]["live_rows"] == 12 and d["records"][0]["floating"] == [12] * 13 and d["floating_rows"] == 12
    # mem: no constraints: all 8 fields of its receive float on every live row
    m = chips[MEM]
    assert m["constraints"] == 0 and m["records"][0]["fields"] == 8 and m["records"][0]["floating"] == [m["records"][0]["live_rows"]] * 8 and m["records"][0]["live_rows"] > 0
    # range: the counter of its receive floats wherever the multiplicity is non-zero
    g = chips[RANGE]
    assert g["constraints"] == 0 and g["records"][0]["fields"] == 1 and g["records"][0]["floating"] == [g["records"][0]["live_rows"]] and g["records"][0]["live_rows"] > 0
    # add and sub: no field of the general-bus record floats (overflow and carry constraints pin each output byte given the operands, and each
    # operand byte given the rest).  What floats is the single field of each of the four range SENDS of the output bytes: the general record is
    # another interaction, deliberately not held fixed, and an output byte can move together with an operand byte.
    for chip in (ADD, SUB):
        recs = chips[chip]["records"]
        assert [(r["is_send"], va.BUS_NAMES[(1, r["bus_index"])], r["fields"]) for r in recs] == [(True, "range", 1)] * 4 + [(False, "general", 13)]
        assert recs[4]["live_rows"] > 0 and recs[4]["floating"] == [0] * 13
        assert floating_of(want, chip) == {(k, 0): recs[4]["live_rows"] for k in range(4)}
    assert rep.floating(DIV) == {(0, j): 12 for j in range(13)} and rep.floating(ADD) == floating_of(want, ADD)
    # lt's operands float (inputs are not functions of outputs), its output does not
    assert floating_of(want, LT) and all(j not in (0, 1, 5) for _, j in floating_of(want, LT))


# ---- 2. analytic AIRs through the capture interface ------------------------------------------------------------------------------------------
PRODF, FREE, LIN2, LIN3, TRANS, WIDEF = range(6)


def analytic_machine():
    """Six captured AIRs, each with one receive:
    PRODF (x, y, z, s: z - x y; fields (x, y, z), count s), FREE (a, b: no constraint; fields (a, 7, b)), LIN2 (a, b: fields (a, 2a + 3b)),
    LIN3 (a, b: fields (a, b, 2a + 3b)), TRANS (s, x: when_transition next.s - s - x; field (s)) and WIDEF (140 columns: x_0 + x_70 - x_139;
    fields (x_0, x_70, x_139, x_100 + x_130)).  Counts other than PRODF's are the constant 1."""
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def new(name, width):
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
        return air

    def push(air):
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)

    def var(air, col, is_next=0):
        return L.vgpu_air_variable(air, u(0), u(col), u(is_next))

    def vcol(terms, constant=0):
        t = (VcolTerm * max(1, len(terms)))(*[VcolTerm(0, c, wt) for c, wt in terms])
        return Vcol(t, len(terms), constant)

    def receive(air, fields, count):
        f = (Vcol * len(fields))(*fields)
        it = Interaction(f, len(fields), count, 1, 0, 0)
        assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()

    one = vcol([], 1)
    air = new(b"prodf", 4)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(var(air, 2)), u(L.vgpu_air_mul(air, u(var(air, 0)), u(var(air, 1)))))))
    receive(air, [vcol([(0, 1)]), vcol([(1, 1)]), vcol([(2, 1)])], vcol([(3, 1)]))
    push(air)
    air = new(b"free", 2)
    receive(air, [vcol([(0, 1)]), vcol([], 7), vcol([(1, 1)])], one)
    push(air)
    air = new(b"lin2", 2)
    receive(air, [vcol([(0, 1)]), vcol([(0, 2), (1, 3)])], one)
    push(air)
    air = new(b"lin3", 2)
    receive(air, [vcol([(0, 1)]), vcol([(1, 1)]), vcol([(0, 2), (1, 3)])], one)
    push(air)
    air = new(b"trans", 2)
    step = L.vgpu_air_sub(air, u(L.vgpu_air_sub(air, u(var(air, 0, 1)), u(var(air, 0)))), u(var(air, 1)))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_mul(air, u(L.vgpu_air_is_transition(air)), u(step))))
    receive(air, [vcol([(0, 1)])], one)
    push(air)
    air = new(b"widef", 140)
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_add(air, u(var(air, 0)), u(var(air, 70)))), u(var(air, 139)))))
    receive(air, [vcol([(0, 1)]), vcol([(70, 1)]), vcol([(139, 1)]), vcol([(100, 1), (130, 1)])], one)
    push(air)
    return va.Machine(m)


def analytic_traces(n):
    r = np.arange(n, dtype=np.uint32)
    x, y = r + 1, r % 2                                # y = 0 on the even rows, x never 0
    s = np.where(r == 1, 0, 3)                         # row 1 sends nothing
    sx = np.stack([r * (r + 1) // 2 + 5, r + 1], axis=1)  # s_{r+1} = s_r + x_r
    wide = (np.arange(140, dtype=np.uint32)[None, :] * 3 + r[:, None] + 1)
    wide[:, 139] = wide[:, 0] + wide[:, 70]
    return [np.stack([x, y, x * y, s], axis=1).astype(np.uint32), np.stack([r + 2, 5 * r + 1], axis=1).astype(np.uint32), np.stack([r + 1, r + 4], axis=1).astype(np.uint32),
            np.stack([r + 1, r + 4], axis=1).astype(np.uint32), sx.astype(np.uint32), wide.astype(np.uint32)]


def check_analytic(rep, n):
    """The closed forms of the six analytic AIRs at height n (every row listed: call with max_rows_per_entry >= n)."""
    by = {(e["chip"], e["interaction"], e["field"]): e for e in rep.entries}

    def rows(chip, field):
        return {r["row"]: (r["n_support"], r["terms"]) for r in by[(chip, 0, field)]["rows"]} if (chip, 0, field) in by else {}

    inv3 = pow(3, P - 2, P)
    # PRODF: C = [-y, -x, 1, 0].  z never floats; x floats exactly where y = 0 (the even rows), y never (x != 0); row 1 has count 0
    live = [r for r in range(n) if r != 1]
    even = [r for r in live if r % 2 == 0]
    c = rep.chips[PRODF]
    assert (c["live_records"], c["floating_fields"], c["floating_rows"]) == (len(live), len(even), len(even))
    assert c["records"][0]["live_rows"] == len(live) and c["records"][0]["floating"] == [len(even), 0, 0] and c["records"][0]["constant"] == [False] * 3
    assert rows(PRODF, 0) == {r: (1, [(0, 1)]) for r in even} and not rows(PRODF, 1) and not rows(PRODF, 2)
    assert rep.floating(PRODF) == ({(0, 0): len(even)} if even else {})
    # FREE: everything non-constant floats; the constant field is flagged and never counted
    c = rep.chips[FREE]
    assert c["constraints"] == 0 and c["records"][0]["constant"] == [False, True, False] and c["records"][0]["floating"] == [n, 0, n]
    assert (c["live_records"], c["floating_fields"], c["floating_rows"]) == (n, 2 * n, n)
    assert rows(FREE, 0) == {r: (1, [(0, 1)]) for r in range(n)} and rows(FREE, 2) == {r: (1, [(1, 1)]) for r in range(n)} and (FREE, 0, 1) not in by
    # LIN2 (a, 2a + 3b): the second floats along b; so does the first, along (1, -2/3)
    c = rep.chips[LIN2]
    assert c["records"][0]["floating"] == [n, n]
    assert rows(LIN2, 1) == {r: (1, [(1, inv3)]) for r in range(n)} and rows(LIN2, 0) == {r: (2, [(0, 1), (1, (P - 2 * inv3 % P) % P)]) for r in range(n)}
    # LIN3 (a, b, 2a + 3b): none floats
    c = rep.chips[LIN3]
    assert c["records"][0]["floating"] == [0, 0, 0] and (c["live_records"], c["floating_fields"], c["floating_rows"]) == (n, 0, 0) and not rep.floating(LIN3)
    # TRANS: s of row r >= 1 is determined through the evaluation at q = r - 1 (next.s); row 0 has only [-1, -1] from q = 0 (n = 1: nothing)
    c = rep.chips[TRANS]
    assert c["records"][0]["floating"] == [1] and c["floating_rows"] == 1
    assert rows(TRANS, 0) == {0: (1, [(0, 1)]) if n == 1 else (2, [(0, 1), (1, P - 1)])}
    # WIDEF: fields beyond lane 63 and beyond 128: x_0, x_70, x_139 are each fixed by the other two, x_100 + x_130 floats along x_100
    c = rep.chips[WIDEF]
    assert c["width"] == 140 and c["records"][0]["floating"] == [0, 0, 0, n] and rows(WIDEF, 3) == {r: (1, [(100, 1)]) for r in range(n)}
    assert rep.total_entries == len(rep.entries) == (1 if even else 0) + 2 + 2 + 1 + 1


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(n):
    rep = va.field_audit_host(analytic_machine(), analytic_traces(n), [], max_rows_per_entry=8)
    check_analytic(rep, n)


# ---- 3. options -------------------------------------------------------------------------------------------------------------------------------
def _host_raw(machine, mt, opts):
    """vgpu_field_audit_host with a raw options pointer (None: NULL); (status, words)."""
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    n = len(mains)
    h = ctypes.c_void_p()
    rc = L.vgpu_field_audit_host(machine._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                 (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * 1)(), (ctypes.c_void_p * 1)(), (ctypes.c_uint64 * 1)(),
                                 (ctypes.c_uint64 * 1)(), ctypes.c_uint32(0), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
    return rc, (va._field_report(h).words if rc == 0 else None)


def test_limits_and_truncation_keep_exact_totals(machines):
    full, _ = both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=ALL_ROWS)
    want, rep = both(machines, "fib25", max_entries=5, max_rows_per_entry=2)
    assert rep.truncated and rep.reported == 5 and rep.total_entries == full["total_entries"] > 5
    assert rep.chips == [c for c in ref.recut(full)["chips"]] and all(len(e["rows"]) == min(2, e["floating"]) for e in rep.entries)
    assert [(e["chip"], e["interaction"], e["field"]) for e in rep.entries] == sorted((e["chip"], e["interaction"], e["field"]) for e in full["entries"])[:5]
    both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=300)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    full = reference(machines, "fib25")
    rep = va.field_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD]
    for c in rep.chips:
        if c["audited"]:
            assert c == full["chips"][c["chip"]]
        else:  # a zero block that keeps the shape
            assert (c["live_records"], c["floating_fields"], c["floating_rows"]) == (0, 0, 0) and not any(r["live_rows"] or any(r["floating"]) for r in c["records"])
            assert (c["width"], c["height"], [r["constant"] for r in c["records"]]) == (
                full["chips"][c["chip"]]["width"], full["chips"][c["chip"]]["height"], [r["constant"] for r in full["chips"][c["chip"]]["records"]])
    assert rep.entries == [e for e in full["entries"] if e["chip"] in (ADD, MEM)]
    with pytest.raises(va.VgpuError, match="field_audit: chip_mask names a chip") as e:
        va.field_audit_host(machines["basic"], mt, prep, chips=[20])
    assert e.value.code == -1


def test_reserved_null_and_defaults():
    machine, mt = analytic_machine(), analytic_traces(8)
    want = va.field_audit_host(machine, mt, []).words
    rc, words = _host_raw(machine, mt, None)  # NULL opts: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = _host_raw(machine, mt, va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(0, 0)))  # zero fields select the defaults
    assert rc == 0 and np.array_equal(words, want)
    for bad in (va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(1, 0)), va.RankAuditOpts(0, 0, 0, (ctypes.c_uint32 * 2)(0, 7)), va.RankAuditOpts((1 << 24) + 1, 0, 0, (ctypes.c_uint32 * 2)(0, 0)),
                va.RankAuditOpts(0, 4097, 0, (ctypes.c_uint32 * 2)(0, 0)), va.RankAuditOpts(0, 0, 1 << 6, (ctypes.c_uint32 * 2)(0, 0))):
        rc, _ = _host_raw(machine, mt, bad)
        assert rc == -1 and b"field_audit" in va.lib().vgpu_last_error()
    with pytest.raises(va.VgpuError, match="field_audit: max_entries and max_rows_per_entry must be at least 1"):
        va.field_audit_host(machine, mt, [], max_entries=0)
    with pytest.raises(va.VgpuError, match="field_audit: chips is a non-empty list"):
        va.field_audit_host(machine, mt, [], chips=[])
    with pytest.raises(va.VgpuError, match="field_audit: .*one main trace per chip"):
        va.field_audit_host(machine, mt[:-1], [])
    with pytest.raises(va.VgpuError, match="two-dimensional"):
        va.field_audit_host(machine, [m.ravel() for m in mt], [])
    with pytest.raises(ValueError, match="not a field report image"):
        va.FieldReport(va.rank_audit_host(machine, mt, []).words)
    assert np.array_equal(va.field_audit_host(machine, mt, []).words, want)  # the same words run after run


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "field_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libfieldauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "field_audit.hpp"), os.path.join(csrc, "host", "rank_audit.hpp"),
            os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("field_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_field_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, rows_per_workgroup=0, max_entries=1024, max_rows_per_entry=4, chips=None):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(1 << 20, np.uint32)
    got = emu.emu_field_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(rows_per_workgroup), ctypes.c_uint32(max_entries), ctypes.c_uint32(max_rows_per_entry), ctypes.c_uint32(sum(1 << c for c in chips) if chips else 0),
        out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """Counting pass, scan and listing pass of field_audit.hip with its wave primitives in their emulation forms (a wave is a 64-thread
    workgroup, as on the device: the kernel runs one wave per workgroup): the compiled chip templates, the interpreted dual register programs
    and the bus-only chips; the assembled report is the host audit's, word for word.  fib(1) without mul (1024 rows; the emulated ballots are
    slow): every other chip, the height-1 chips, bus-only chips that keep the row before's answer (mem, range).  mixed_ops with 3 rows per
    workgroup on the chips that fib leaves idle — div, shift with its two records, lt, com, bitwise with its 79 columns (more than one word
    per lane), output — and on cpu and mem: the r - 1 halo, the wrap between row 0 and row n - 1 and the rank scan cross workgroup boundaries
    (lists of 20 rows run over several workgroups), and the listing pass rebuilds the base between the listed fields of a row.
    NOT covered here: the hardware's own ballot and wave barrier, the opt-in to more than 64 KB of LDS, and the launch shapes of
    tall traces; tests/test_field_audit_gpu.py covers those."""
    mt, prep = witness("fib1")
    chips = [c for c in range(14) if c != MUL]
    host = va.field_audit_host(machines["basic"], mt, prep, chips=chips)
    assert host.floating(CPU) and host.floating(MEM) and host.floating(RANGE)
    assert np.array_equal(emulated(emu, mt, prep, interpret, chips=chips), host.words)
    mt, prep = witness("mixed_ops")
    some = [CPU, MEM, DIV, SHIFT, LT, COM, BITWISE, OUTPUT]
    host = va.field_audit_host(machines["basic"], mt, prep, chips=some, max_rows_per_entry=20, max_entries=60)
    assert host.truncated and any(len(e["rows"]) == 20 and e["rows"][-1]["row"] - e["rows"][0]["row"] > 6 for e in host.entries if e["chip"] == MEM)
    assert host.floating(DIV) and host.floating(SHIFT) and mt[BITWISE].shape[1] == 79
    assert np.array_equal(emulated(emu, mt, prep, interpret, rows_per_workgroup=3, chips=some, max_rows_per_entry=20, max_entries=60), host.words)


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_fields_on_the_host(tmp_path, machines):
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out, "--host")
    plain_json, plain_text = json.loads(out.read_text()), out.read_text()
    again = _cli("check", bl, out, "--host")  # without the flag: what it did before (the timing key aside)
    assert again.stdout == plain.stdout and again.returncode == plain.returncode and set(json.loads(out.read_text())) == set(plain_json) and "fields" not in plain_text
    r = _cli("check", bl, out, "--host", "--fields")
    assert r.returncode == plain.returncode == 0, r.stderr  # a floating field is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.field_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    recs = [(c, r_) for c in rep.chips for r_ in c["records"] if any(r_["floating"])]
    assert recs and len(lines) == len(before) + len(recs)
    for line, (c, r_) in zip(lines[len(before):], recs):
        assert line.startswith("%s: interaction %d (%s on the %s bus): field" % (va.CHIP_NAMES[c["chip"]], r_["interaction"], "sends" if r_["is_send"] else "receives",
                                                                                 va.BUS_NAMES[(1, r_["bus_index"])]))
        assert line.endswith("on %d of %d live row%s" % (max(r_["floating"]), r_["live_rows"], "" if r_["live_rows"] == 1 else "s"))
    n_mem = rep.chips[MEM]["records"][0]["live_rows"]
    assert "mem: interaction 0 (receives on the memory bus): fields 0-7 float on %d of %d live rows" % (n_mem, n_mem) in lines
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"fields"} and {k: v for k, v in j.items() if k not in ("fields", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["fields"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--fields", "--chips=add,4")
    assert r.returncode == 0 and [c["chip"] for c in json.loads(out.read_text())["fields"]["chips"] if c["audited"]] == [ADD, SUB]
    help_text = _cli("check", "--help").stdout
    assert "--fields" in help_text and "usually means" in help_text and "does not depend on this flag" in help_text


# ---- 6. C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_field_audit", "vgpu_field_audit_host", "vgpu_field_report_len", "vgpu_field_report_words", "vgpu_field_report_timing", "vgpu_field_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Field audit" in header and "VFA1" in header and "deliberately" in header
