"""The mutation audit without a GPU: the host implementation of the contract (vgpu_mutation_audit_host) against the brute-force restatement of
tests/mutation_audit_ref.py (the oracle's own chip transcription, cell by cell) on whole witnesses, word for word, for both machine kinds;
delta sets; truncation; argument validation; the device kernels' very source under tools/hipemu; `check --mutations` on the command line.
The literals pinned here (unbound columns and free cells per chip) are those of a prototype over the oracle's transcription, not of the code
under test; the reference of each input is computed once per module and cut to the limits a test asks for (counts do not depend on them)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mutation_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
ALL_ROWS = 1 << 30  # a row limit no trace reaches: the reference is made with it and cut afterwards


def exe(prog, advice=b""):
    return va.Workload.from_executable(vp.machine_code(prog), advice=advice)


INPUTS = {
    "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "static_data": lambda: va.Workload.named("static_data"),
    "left_imm_ops": lambda: va.Workload.named("left_imm_ops"), "byte_loop50": lambda: exe(vp.byte_loop_program(50), bytes(range(30))),
    "mixed_ops:40": lambda: va.Workload.named("mixed_ops:40"),  # a FAILING witness: "newly failing", not "non-zero"
}
_witness, _reference = {}, {}


def witness(name):
    if name not in _witness:
        w = INPUTS[name]()
        _witness[name] = (w.main_traces(), w.preprocessed())
    return _witness[name]


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def reference(machines, name, deltas=(1, P - 1), **limits):
    """The reference's report of a named input, computed once per (input, deltas) with every free row listed, cut to `limits`."""
    key = (name, tuple(deltas))
    if key not in _reference:
        mt, prep = witness(name)
        _reference[key] = ref.audit(machines["basic"], mt, prep, deltas=deltas, max_entries=1 << 30, max_rows_per_entry=ALL_ROWS)
    return ref.recut(_reference[key], **limits) if limits else ref.recut(_reference[key], 1024, 4)


def both(machines, name, deltas=(1, P - 1), **limits):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, deltas, **limits)
    mt, prep = witness(name)
    reps = {k: va.mutation_audit_host(m, mt, prep, deltas=deltas, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    assert np.array_equal(reps["basic"].words, reps["ffi"].words)
    return want, reps["basic"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
def test_fib25_is_the_issues_table(machines):
    want, rep = both(machines, "fib25")
    assert rep.deltas == [1, P - 1] and not rep.truncated and rep.total_entries == rep.reported
    table = {  # chip: (height, unbound columns, free cells at +1, at -1)
        CPU: (256, [14, 15, 17], 3131, 3047), PROGRAM: (32, [0], 32, 32), MEM: (512, [9, 10, 11, 12, 13], 3337, 3337), ADD: (128, [], 0, 0), SUB: (1, [], 0, 0),
        MUL: (1024, list(range(8)), 8192, 8192), DIV: (1, list(range(12)), 12, 12), SHIFT: (1, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11], 11, 11), LT: (1, [21, 27], 4, 2),
        COM: (1, [9], 1, 1), BITWISE: (1, [72, 73, 74, 75], 4, 4), OUTPUT: (1, [0, 1, 3, 4, 5, 6], 6, 6), RANGE: (256, [], 207, 207), STATIC_DATA: (1, [0, 1, 2, 3, 4], 5, 5)}
    for chip, (height, unbound, plus, minus) in table.items():
        c = rep.chips[chip]
        assert (c["height"], rep.unbound_columns(chip), c["unbound"], c["free"]) == (height, unbound, len(unbound), [plus, minus]), va.CHIP_NAMES[chip]
        assert ref.unbound_columns(want, chip) == unbound
    # the report is per delta because these cpu columns give different counts for +1 and -1
    by = {(e["column"], e["delta"]): e["free"] for e in rep.entries if e["chip"] == CPU}
    assert [c for c in range(51) if by.get((c, 0), 0) != by.get((c, 1), 0)] == [11, 12, 18, 22]
    for e in rep.entries:
        n = rep.chips[e["chip"]]["height"]
        assert 0 < e["free"] <= n and e["air"] + e["bus"] + e["free"] >= n and e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(4, e["free"])


def test_alu50(machines):
    want, rep = both(machines, "alu50")
    assert {c: rep.chips[c]["height"] for c in (CPU, MEM, ADD, SUB, LT, BITWISE)} == {CPU: 512, MEM: 2048, ADD: 256, SUB: 64, LT: 64, BITWISE: 256}
    assert {c: rep.chips[c]["free"] for c in (CPU, MEM, ADD, SUB, LT, BITWISE)} == {CPU: [4299, 4235], MEM: [16498, 16498], ADD: [0, 0], SUB: [0, 0], LT: [56, 28], BITWISE: [424, 424]}
    assert rep.chips[LT]["unbound"] == 0 and rep.unbound_columns(LT) == []


@pytest.mark.parametrize("name", ["static_data", "left_imm_ops", "byte_loop50"])
def test_clean_witnesses(machines, name):
    want, rep = both(machines, name)
    assert not rep.truncated and rep.unbound_columns(MUL) == list(range(8))


def test_failing_witness_counts_newly_failing_constraints(machines):
    """mixed_ops:40 fails 13 constraints already (tests/test_constraint_audit_cpu.py): a mutation is detected only by a constraint that did not
    fail at that row before, so the rows that fail anyway do not make every cell of theirs 'detected'."""
    mt, prep = witness("mixed_ops:40")
    assert not va.constraint_audit_host(machines["basic"], mt, prep).satisfied
    want, rep = both(machines, "mixed_ops:40")
    assert rep.chips[MUL]["height"] == 1024 and rep.chips[MUL]["free"][0] > 0


@pytest.mark.parametrize("deltas", [(1,), (1, P - 1), (2, 1, P - 1, 12345)], ids=["+1", "+1,-1", "four"])
def test_delta_sets(machines, deltas):
    want, rep = both(machines, "static_data", deltas)
    assert rep.deltas == list(deltas) and all(len(c["free"]) == len(deltas) for c in rep.chips)
    # delta index i of any set is that delta's report: +1 is index 0 of the pair and index 1 of the four
    pair = reference(machines, "static_data")
    at = list(deltas).index(1)
    assert [c["free"][at] for c in rep.chips] == [c["free"][0] for c in pair["chips"]]


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------------
def test_truncation(machines):
    full_want, full = both(machines, "fib25")
    want, rep = both(machines, "fib25", max_entries=3)
    assert rep.truncated and rep.reported == 3 and rep.total_entries == full.total_entries > 3 and rep.chips == full.chips
    assert [(e["chip"], e["column"], e["delta"]) for e in rep.entries] == [(e["chip"], e["column"], e["delta"]) for e in full.entries[:3]]
    want, one = both(machines, "fib25", max_rows_per_entry=1)
    want, every = both(machines, "fib25", max_rows_per_entry=1000)
    assert not one.truncated and not every.truncated and one.chips == every.chips == full.chips
    for a, b in zip(one.entries, every.entries):
        assert (a["free"], a["air"], a["bus"]) == (b["free"], b["air"], b["bus"]) and len(a["rows"]) == 1 and a["rows"][0] == b["rows"][0]
        assert len(b["rows"]) == min(b["free"], 1000) and b["rows"] == sorted(set(b["rows"]))


# ---- 3. argument validation -------------------------------------------------------------------------------------------------------------------
def test_argument_validation(machines):
    m = machines["basic"]
    mt, prep = witness("static_data")

    def refused(match, main=mt, pre=prep, **kw):
        with pytest.raises(va.VgpuError, match=match) as e:
            va.mutation_audit_host(m, main, pre, **kw)
        assert e.value.code == -1  # VGPU_ERR_INVALID_ARG

    refused("mutation_audit: need one main trace per chip", main=mt[:-1])
    refused("width mismatch for chip add", main=mt[:ADD] + [mt[ADD][:, :-1]] + mt[ADD + 1:])
    refused("powers of two", main=mt[:MUL] + [mt[MUL][:-1]] + mt[MUL + 1:])
    refused("chip add has no preprocessed columns", pre=prep + [(ADD, mt[ADD])])
    refused("needs its preprocessed trace", pre=prep[:1])
    refused("repeated preprocessed chip", pre=prep + prep[:1])
    refused("preprocessed trace shape mismatch", pre=[prep[0], (prep[1][0], prep[1][1][:128])])
    refused("max_entries", max_entries=0)  # an explicit zero passed through Python
    refused("max_rows_per_entry", max_rows_per_entry=0)
    refused("1 to 4 deltas", deltas=())
    refused("1 to 4 deltas", deltas=(1, 2, 3, 4, 5))
    refused("a delta must be a canonical value in 1..p-1", deltas=(1, 0))
    refused("a delta must be a canonical value in 1..p-1", deltas=(P,))
    refused("the deltas must be distinct", deltas=(5, 7, 5))
    # the C entry point itself: reserved != 0, too many deltas and null arguments are refused with a code and a message; a zeroed struct (or
    # NULL) means the defaults
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[x.ctypes.data for x in mt])
    hs, ws = (ctypes.c_uint64 * 14)(*[x.shape[0] for x in mt]), (ctypes.c_uint64 * 14)(*[x.shape[1] for x in mt])
    pa = (ctypes.c_void_p * 2)(*[x.ctypes.data for _, x in prep])
    ph, pw = (ctypes.c_uint64 * 2)(*[x.shape[0] for _, x in prep]), (ctypes.c_uint64 * 2)(*[x.shape[1] for _, x in prep])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in prep])
    L = va.lib()

    def opts(max_entries=0, rows=0, n=0, deltas=(0, 0, 0, 0), reserved=(0, 0)):
        return ctypes.byref(va.MutationAuditOpts(max_entries, rows, n, (ctypes.c_uint32 * 4)(*deltas), (ctypes.c_uint32 * 2)(*reserved)))

    assert ctypes.sizeof(va.MutationAuditOpts) == 40
    assert L.vgpu_mutation_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(reserved=(0, 1)), ctypes.byref(h)) == -1 and b"reserved" in L.vgpu_last_error()
    assert L.vgpu_mutation_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(n=5), ctypes.byref(h)) == -1 and b"at most 4 deltas" in L.vgpu_last_error()
    assert L.vgpu_mutation_audit_host(m._h, None, hs, ws, 14, chips, pa, ph, pw, 2, None, ctypes.byref(h)) == -1 and b"null" in L.vgpu_last_error()
    L.vgpu_mutation_report_len.restype = ctypes.c_uint64
    L.vgpu_mutation_report_words.restype = ctypes.POINTER(ctypes.c_uint32)
    L.vgpu_mutation_report_len.argtypes = L.vgpu_mutation_report_words.argtypes = L.vgpu_mutation_report_free.argtypes = [ctypes.c_void_p]
    want = va.mutation_audit_host(m, mt, prep).words
    for o in (opts(), None):
        assert L.vgpu_mutation_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, o, ctypes.byref(h)) == 0
        n = L.vgpu_mutation_report_len(h)
        assert np.array_equal(np.ctypeslib.as_array(L.vgpu_mutation_report_words(h), shape=(n,)), want)
        L.vgpu_mutation_report_free(h)


def test_report_image_and_json(machines):
    mt, prep = witness("static_data")
    rep = va.mutation_audit_host(machines["basic"], mt, prep)
    w = [int(x) for x in rep.words]
    assert w[0] == 0x31524D56 and bytes(rep.words[:1].tobytes()) == b"VMR1" and w[1] == len(w) and w[2:4] == [2, 0] and w[6:12] == [rep.reported, 14, 1, P - 1, 0, 0]
    assert rep.device_ms == 0.0 and rep.host_ms > 0 and rep.evaluations > 0
    again = va.MutationReport(rep.words)
    assert again.entries == rep.entries and again.chips == rep.chips and again.deltas == rep.deltas
    j = json.loads(rep.to_json())
    assert j["deltas"] == [1, P - 1] and j["total_entries"] == rep.total_entries and j["device_ms"] == 0.0 and j["entries"][0] == rep.entries[0] and j["chips"] == rep.chips
    assert np.array_equal(va.mutation_audit_host(machines["basic"], mt, prep).words, rep.words)  # the same words run after run


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "mutation_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libmutationauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"),
            os.path.join(csrc, "host", "machine.hpp")] + [os.path.join(csrc, "kernels", f) for f in ("mutation_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_mutation_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, block_threads=0, deltas=(1, P - 1), max_entries=1024, max_rows_per_entry=4, column_slices=0, bus_walk=0):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(12 + 14 * 30 + min(max_entries, 2048) * (10 + min(max_rows_per_entry, 2048)), np.uint32)
    got = emu.emu_mutation_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(block_threads), ctypes.c_uint32(column_slices), ctypes.c_uint32(bus_walk), (ctypes.c_uint32 * len(deltas))(*deltas), ctypes.c_uint32(len(deltas)), ctypes.c_uint32(max_entries), ctypes.c_uint32(max_rows_per_entry),
        out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
@pytest.mark.parametrize("name", ["fib25", "mixed_ops:40", "static_data"])
def test_kernel_source_under_emulation(machines, emu, name, interpret):
    """Counting pass, scan and listing pass of mutation_audit.hip, the compiled chip templates, the interpreted programs and the bus-only chips:
    the assembled report is the reference's, word for word.  In the device's launch shape fib25's mul (1024 rows) and mem (512) span several
    workgroups; with 64-row workgroups its cpu trace (256 rows) does too, so the r - 1 halo, the wrap between row 0 and row n - 1 and the rank
    scan all cross workgroup boundaries."""
    mt, prep = witness(name)
    assert np.array_equal(emulated(emu, mt, prep, interpret), ref.words(reference(machines, name)))
    if name == "fib25":
        assert mt[CPU].shape[0] == 256 and mt[MUL].shape[0] == 1024
        for kw in (dict(max_entries=3), dict(max_rows_per_entry=1), dict(max_rows_per_entry=300)):
            assert np.array_equal(emulated(emu, mt, prep, interpret, **kw), ref.words(reference(machines, name, **dict(dict(max_entries=1024, max_rows_per_entry=4), **kw))))
        # one workgroup walks every column / three column slices / the interactions evaluated per mutation instead of the bus masks
        for kw in (dict(column_slices=1), dict(column_slices=3, block_threads=64, max_rows_per_entry=100), dict(bus_walk=1)):
            assert np.array_equal(emulated(emu, mt, prep, interpret, **kw), ref.words(reference(machines, name, max_entries=1024, max_rows_per_entry=kw.get("max_rows_per_entry", 4))))
        for rows in (3, 100):  # a cut list ends inside a workgroup (3) and runs over several (100)
            assert np.array_equal(emulated(emu, mt, prep, interpret, block_threads=64, max_rows_per_entry=rows), ref.words(reference(machines, name, max_entries=1024, max_rows_per_entry=rows)))
    if name == "static_data":
        deltas = (2, 1, P - 1, 12345)
        assert np.array_equal(emulated(emu, mt, prep, interpret, deltas=deltas), ref.words(reference(machines, name, deltas)))


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_mutations_on_the_host(tmp_path, machines):
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out, "--host")
    assert plain.returncode == 0, plain.stderr
    plain_json = json.loads(out.read_text())
    r = _cli("check", bl, out, "--host", "--mutations")
    assert r.returncode == 0, r.stderr  # an unbound column is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = exe(vp.byte_loads_program())
    rep = va.mutation_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    chips = [c for c in rep.chips if any(c["free"])]
    assert len(lines) == len(before) + len(chips)
    for line, c in zip(lines[len(before):], chips):
        assert line.startswith(va.CHIP_NAMES[c["chip"]] + ": ") and line.endswith("free cells %d (+1), %d (-1) of %d" % (c["free"][0], c["free"][1], c["height"] * c["width"]))
    assert any(line.startswith("mul: unbound columns 0-7; free cells 8192 (+1), 8192 (-1) of 18432") for line in lines)
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"mutations"} and {k: v for k, v in j.items() if k not in ("mutations", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    m = j["mutations"]
    assert m["deltas"] == [1, P - 1] and m["chips"] == rep.chips and m["entries"] == rep.entries and not m["truncated"]
    r = _cli("check", bl, out, "--host", "--mutations", "--deltas=2")
    assert r.returncode == 0 and json.loads(out.read_text())["mutations"]["deltas"] == [2] and "(+2)" in r.stdout
    r = _cli("check", bl, out, "--host", "--mutations", "--deltas=1,1")
    assert r.returncode != 0 and "distinct" in r.stderr + r.stdout
