"""The constraint audit without a GPU: the host implementation of the contract (vgpu_constraint_audit_host) against the independent restatement
of tests/constraint_audit_ref.py (the oracle's own chip transcription, row by row) on every input of the issue's tables, word for word, for both
machine kinds; truncation; argument validation; the device kernels' very source under tools/hipemu; `check --constraints` on the command line.
The literals pinned here (constraints per chip, failing constraints, row counts, first rows and values) were obtained from the reference
(oracle.pyoracle.eval_constraints) alone, not from the code under test."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, ADD, SUB, MUL, SHIFT, LT, COM, BITWISE, OUTPUT, STATIC_DATA = 0, 3, 4, 5, 7, 8, 9, 10, 11, 13
N_CONSTRAINTS = [53, 0, 0, 10, 7, 5, 0, 18, 60, 8, 88, 3, 0, 1]  # per chip, in machine order


def exe(prog, advice=b""):
    return va.Workload.from_executable(vp.machine_code(prog), advice=advice)


def witness(w, faults=()):
    mt, prep = w.main_traces(), w.preprocessed()
    for chip, row, col in faults:
        mt[chip][row, col] = (int(mt[chip][row, col]) + 1) % P
    return mt, prep


def every_50th(w, height=None):
    """The witness of `w` with column 1 (pc) of the cpu trace corrupted on every 50th row: failing rows spread over all workgroups."""
    mt, prep = witness(w)
    if height is not None:
        assert mt[CPU].shape[0] == height
    mt[CPU][::50, 1] = (mt[CPU][::50, 1].astype(np.uint64) + 1) % P
    return mt, prep


CLEAN = {
    "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "static_data": lambda: va.Workload.named("static_data"),
    "signed_inequality": lambda: va.Workload.named("signed_inequality"), "left_imm_ops": lambda: va.Workload.named("left_imm_ops"),
    "loadfp": lambda: va.Workload.named("loadfp"), "store_byte": lambda: exe(vp.store_byte_program()), "byte_loads": lambda: exe(vp.byte_loads_program()),
    "advice": lambda: exe(vp.advice_program(5), b"\x01\x80\xff"), "byte_loop50": lambda: exe(vp.byte_loop_program(50), bytes(range(30))),
    "fib9359": lambda: va.Workload.fib(9359),
}
FAILING = {"mixed_ops:40": lambda: va.Workload.named("mixed_ops:40"), "echo3": lambda: exe(vp.echo_program(3), b"abc")}
# (chip, row, col) + 1 mod P on fib25 -> exactly these (chip, constraint, [(row, value)])
FAULTS = [
    ((CPU, 10, 1), [(CPU, 1, [(9, 24)])]),
    ((ADD, 5, 11), [(ADD, 3, [(5, 257)])]),
    ((ADD, 5, 0), [(ADD, 3, [(5, 2013265666)])]),
    ((CPU, 255, 2), [(CPU, 7, [(254, 1)])]),
    ((LT, 0, 0), [(LT, 1, [(0, P - 1)]), (LT, 18, [(0, P - 1)])]),
]


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def both(machines, mt, prep, **kw):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = ref.audit(mt, prep, **kw)
    reps = {k: va.constraint_audit_host(m, mt, prep, **kw) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    assert np.array_equal(reps["basic"].words, reps["ffi"].words)
    return want, reps["basic"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLEAN))
def test_clean_witnesses(machines, name):
    w = CLEAN[name]()
    if name == "fib9359":
        assert w.cpu_height == 1 << 16
    want, rep = both(machines, *witness(w))
    assert want["total_failing"] == 0 and rep.satisfied and not rep.truncated and rep.constraints == [] and rep.reported == 0
    assert [c["constraints"] for c in rep.chips] == N_CONSTRAINTS and all(c["failing_rows"] == 0 and c["failing_constraints"] == 0 for c in rep.chips)


def test_store_byte_is_clean_here_and_unbalanced_on_the_bus(machines):
    """The STOREU8 program every verifier rejects: its AIR is clean on all 14 chips, only its memory bus is unbalanced — the two audits side by side."""
    mt, prep = witness(exe(vp.store_byte_program()))
    assert va.constraint_audit_host(machines["basic"], mt, prep).satisfied
    assert va.bus_audit_host(machines["basic"], mt, prep).total_unbalanced == 5


def entry(rep, chip, k):
    (e,) = [e for e in rep.constraints if (e["chip"], e["constraint"]) == (chip, k)]
    return e


def test_mixed_ops(machines):
    mt, prep = witness(FAILING["mixed_ops:40"]())
    # (the mul trace of this workload is 1024 rows high — mul rows are not one per multiplication — and 235 / 233 of them fail)
    assert [mt[c].shape[0] for c in (CPU, MUL, SHIFT, COM, OUTPUT)] == [1024, 1024, 256, 128, 64]
    want, rep = both(machines, mt, prep)
    assert not rep.satisfied and rep.total_failing == 13 == rep.reported and not rep.truncated
    assert [(e["chip"], e["constraint"], e["failing_rows"]) for e in rep.constraints] == [
        (CPU, 32, 41), (CPU, 33, 41), (CPU, 35, 41), (CPU, 42, 41), (MUL, 0, 235), (MUL, 1, 233), (SHIFT, 9, 160), (SHIFT, 10, 160), (SHIFT, 13, 160),
        (COM, 7, 40), (OUTPUT, 0, 1), (OUTPUT, 1, 63), (OUTPUT, 2, 41)]
    for k in (32, 33, 35, 42):
        assert [r for r, _ in entry(rep, CPU, k)["rows"][:2]] == [21, 41]
    assert entry(rep, CPU, 32)["rows"][0] == (21, 2013261825)
    assert entry(rep, MUL, 0)["rows"][0] == (0, 805305946) and entry(rep, MUL, 1)["rows"][0] == (0, 12124160)
    assert entry(rep, SHIFT, 9)["rows"][0] == (0, 5) and entry(rep, SHIFT, 10)["rows"][0] == (0, P - 5) and entry(rep, SHIFT, 13)["rows"][0] == (0, 32)
    assert entry(rep, COM, 7)["rows"][0] == (1, P - 1)
    assert entry(rep, OUTPUT, 0)["rows"] == [(40, 805)] and entry(rep, OUTPUT, 1)["rows"][0][0] == 0 and entry(rep, OUTPUT, 2)["rows"][0] == (0, 2013265621)
    assert {c["chip"]: c["failing_constraints"] for c in rep.chips if c["failing_constraints"]} == {CPU: 4, MUL: 2, SHIFT: 3, COM: 1, OUTPUT: 3}


def test_echo(machines):
    want, rep = both(machines, *witness(FAILING["echo3"]()))
    assert [(e["chip"], e["constraint"], e["failing_rows"]) for e in rep.constraints] == [
        (CPU, 32, 3), (CPU, 33, 3), (CPU, 35, 3), (CPU, 42, 3), (OUTPUT, 0, 1), (OUTPUT, 1, 3), (OUTPUT, 2, 3)]
    for k in (32, 33, 35, 42):
        assert [r for r, _ in entry(rep, CPU, k)["rows"][:2]] == [1, 3]
    assert entry(rep, OUTPUT, 0)["rows"] == [(2, 5)]


@pytest.mark.parametrize("fault,failures", FAULTS)
def test_single_cell_faults(machines, fib25, fault, failures):
    """Each fault gives exactly the listed failures and nothing else; (cpu, 255, 2) is on the LAST row: it shows through the row before it (whose
    `next` it is) and not through `next` of the last row, where is_transition is 0."""
    want, rep = both(machines, *witness(fib25, [fault]))
    assert [(e["chip"], e["constraint"], e["rows"]) for e in rep.constraints] == failures
    assert all(e["failing_rows"] == 1 for e in rep.constraints) and rep.total_failing == len(failures)
    assert [c["failing_rows"] for c in rep.chips if c["failing_rows"]] == [1]


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------------
def test_truncation(machines):
    mt, prep = witness(FAILING["mixed_ops:40"]())
    full = va.constraint_audit_host(machines["basic"], mt, prep, max_rows_per_constraint=1000)
    want, rep = both(machines, mt, prep, max_constraints=3)
    assert rep.truncated and rep.total_failing == 13 and rep.reported == 3 and [(e["chip"], e["constraint"]) for e in rep.constraints] == [(CPU, 32), (CPU, 33), (CPU, 35)]
    assert rep.chips == full.chips
    want, one = both(machines, mt, prep, max_rows_per_constraint=1)
    want, every = both(machines, mt, prep, max_rows_per_constraint=1000)
    assert not one.truncated and not every.truncated
    for a, b in zip(one.constraints, every.constraints):
        assert a["failing_rows"] == b["failing_rows"] == len(b["rows"]) and len(a["rows"]) == 1 and a["rows"][0] == b["rows"][0]
        assert [r for r, _ in b["rows"]] == sorted(set(r for r, _ in b["rows"]))


# ---- 3. argument validation -------------------------------------------------------------------------------------------------------------------
def test_argument_validation(machines, fib25):
    m = machines["basic"]
    mt, prep = witness(fib25)

    def refused(match, main=mt, pre=prep, **kw):
        with pytest.raises(va.VgpuError, match=match) as e:
            va.constraint_audit_host(m, main, pre, **kw)
        assert e.value.code == -1  # VGPU_ERR_INVALID_ARG

    refused("one main trace per chip", main=mt[:-1])
    refused("width mismatch for chip add", main=mt[:ADD] + [mt[ADD][:, :-1]] + mt[ADD + 1:])
    refused("powers of two", main=mt[:ADD] + [mt[ADD][:-1]] + mt[ADD + 1:])
    refused("chip add has no preprocessed columns", pre=prep + [(ADD, mt[ADD])])
    refused("needs its preprocessed trace", pre=prep[:1])
    refused("repeated preprocessed chip", pre=prep + prep[:1])
    refused("preprocessed trace shape mismatch", pre=[prep[0], (prep[1][0], prep[1][1][:128])])
    refused("max_constraints", max_constraints=0)  # an explicit zero passed through Python
    refused("max_rows_per_constraint", max_rows_per_constraint=0)
    # the C entry point itself: reserved != 0 and null arguments are refused with a code and a message, a zeroed struct (or NULL) means the defaults
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[x.ctypes.data for x in mt])
    hs, ws = (ctypes.c_uint64 * 14)(*[x.shape[0] for x in mt]), (ctypes.c_uint64 * 14)(*[x.shape[1] for x in mt])
    pa = (ctypes.c_void_p * 2)(*[x.ctypes.data for _, x in prep])
    ph, pw = (ctypes.c_uint64 * 2)(*[x.shape[0] for _, x in prep]), (ctypes.c_uint64 * 2)(*[x.shape[1] for _, x in prep])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in prep])
    L = va.lib()
    assert L.vgpu_constraint_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, ctypes.byref(va.ConstraintAuditOpts(0, 0, 1)), ctypes.byref(h)) == -1
    assert b"reserved" in L.vgpu_last_error()
    assert L.vgpu_constraint_audit_host(m._h, None, hs, ws, 14, chips, pa, ph, pw, 2, None, ctypes.byref(h)) == -1 and b"null" in L.vgpu_last_error()
    L.vgpu_constraint_report_len.restype = ctypes.c_uint64
    L.vgpu_constraint_report_len.argtypes = L.vgpu_constraint_report_free.argtypes = [ctypes.c_void_p]
    for opts in (ctypes.byref(va.ConstraintAuditOpts(0, 0, 0)), None):
        assert L.vgpu_constraint_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts, ctypes.byref(h)) == 0
        assert L.vgpu_constraint_report_len(h) == 8 + 14 * 6
        L.vgpu_constraint_report_free(h)


def test_report_image_and_json(machines):
    mt, prep = witness(FAILING["echo3"]())
    rep = va.constraint_audit_host(machines["basic"], mt, prep)
    w = [int(x) for x in rep.words]
    assert w[0] == 0x31524356 and bytes(rep.words[:1].tobytes()) == b"VCR1" and w[1] == len(w) and w[2:8] == [0, 0, 7, 0, 7, 14]
    again = va.ConstraintReport(rep.words)
    assert again.constraints == rep.constraints and again.chips == rep.chips
    j = json.loads(rep.to_json())
    assert j["total_failing"] == 7 and not j["satisfied"] and j["device_ms"] == 0.0 and j["constraints"][4] == dict(chip=OUTPUT, constraint=0, failing_rows=1, rows=[[2, 5]])
    assert np.array_equal(va.constraint_audit_host(machines["basic"], mt, prep).words, rep.words)  # the same words run after run


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "constraint_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libconstraintauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
        os.path.join(csrc, "kernels", f) for f in ("constraint_audit.hip", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_constraint_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, block_threads=0, max_constraints=64, max_rows_per_constraint=4):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(8 + 14 * 6 + max_constraints * (5 + 2 * max_rows_per_constraint), np.uint32)
    got = emu.emu_constraint_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(block_threads), ctypes.c_uint32(max_constraints), ctypes.c_uint32(max_rows_per_constraint), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


EMU_INPUTS = {"mixed_ops:40": lambda: witness(FAILING["mixed_ops:40"]()), "echo3": lambda: witness(FAILING["echo3"]()), "clean fib25": lambda: witness(va.Workload.fib(25)),
              "clean byte_loop50": lambda: witness(CLEAN["byte_loop50"]())}
EMU_INPUTS.update({"fault %s" % (f,): (lambda f=f: witness(va.Workload.fib(25), [f])) for f, _ in FAULTS})


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
@pytest.mark.parametrize("name", list(EMU_INPUTS))
def test_kernel_source_under_emulation(emu, name, interpret):
    """Counting pass, scan, listing pass and value pass of constraint_audit.hip, the compiled chip templates and the interpreted programs: the
    assembled report is the reference's, word for word."""
    mt, prep = EMU_INPUTS[name]()
    assert np.array_equal(emulated(emu, mt, prep, interpret), ref.words(ref.audit(mt, prep)))
    if name == "mixed_ops:40":
        for kw in (dict(max_constraints=3), dict(max_rows_per_constraint=1), dict(max_rows_per_constraint=300)):
            assert np.array_equal(emulated(emu, mt, prep, interpret, **kw), ref.words(ref.audit(mt, prep, **kw)))
        # 64-row workgroups: the mul chip's 235 failing rows lie in 16 workgroups, the first 100 in several
        assert np.array_equal(emulated(emu, mt, prep, interpret, block_threads=64, max_rows_per_constraint=100), ref.words(ref.audit(mt, prep, max_rows_per_constraint=100)))


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
@pytest.mark.parametrize("block_threads,rows", [(0, 4), (0, 2), (64, 4), (64, 3), (64, 1000)])
def test_ranks_cross_workgroups_under_emulation(emu, fib25, interpret, block_threads, rows):
    """fib25's cpu trace (256 rows) with pc corrupted on every 50th row (rows 0, 50, .., 250: the fault on row r fails constraints on rows r - 1 and
    r, where the selectors of those rows let it): with 64-row workgroups the failing rows of a constraint lie in several workgroups and a cut list ends inside one; the listed rows are the first in
    ascending order, the reference's."""
    mt, prep = every_50th(fib25, 256)
    want = ref.audit(mt, prep, max_rows_per_constraint=rows)
    full = ref.audit(mt, prep, max_rows_per_constraint=1000)["constraints"]
    assert [[r for r, _ in e["rows"]] for e in full] == [[0, 50, 99], [49, 149], [199, 200, 249, 250]]  # constraints 0, 1, 51: in 64-row workgroups 0 and 1, 0 and 2, 3
    assert np.array_equal(emulated(emu, mt, prep, interpret, block_threads=block_threads, max_rows_per_constraint=rows), ref.words(want))


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_constraints_on_the_host(tmp_path, machines):
    echo, adv, bl, out = tmp_path / "echo.bin", tmp_path / "advice", tmp_path / "byte_loads.bin", tmp_path / "report.json"
    echo.write_bytes(vp.machine_code(vp.echo_program(3)))
    adv.write_bytes(b"abc")
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    r = _cli("check", echo, out, adv, "--host", "--constraints")
    assert r.returncode == 1, r.stderr
    lines = r.stdout.strip().split("\n")
    bus = [k for k, line in enumerate(lines) if line.startswith("unbalanced: ")]
    assert bus == [6] and len(lines) == 7 + 7 + 1  # six tuples and the bus summary, then seven constraints and their summary
    mt, prep = witness(exe(vp.echo_program(3), b"abc"))
    want = ref.audit(mt, prep)
    for line, e in zip(lines[7:14], want["constraints"]):
        assert line.startswith("%s constraint %d fails on %d rows: row %d = %d" % (va.CHIP_NAMES[e["chip"]], e["constraint"], e["failing_rows"], e["rows"][0][0], e["rows"][0][1]))
    assert lines[7].startswith("cpu constraint 32 fails on 3 rows: row 1 = ") and "(pc 1 WRITE)" in lines[7] and lines[11] == "output constraint 0 fails on 1 rows: row 2 = 5"
    assert lines[14].startswith("violated: 7 constraints of 2 chips")
    j = json.loads(out.read_text())
    assert j["total_unbalanced"] == 6 and set(j) == {"balanced", "truncated", "total_unbalanced", "reported", "device_ms", "host_ms", "buses", "tuples", "constraints"}
    c = j["constraints"]
    assert not c["satisfied"] and c["total_failing"] == 7 and c["chips"] == want["chips"]
    assert [dict(e, rows=[tuple(x) for x in e["rows"]]) for e in c["constraints"]] == want["constraints"]
    r = _cli("check", echo, out, adv, "--host", "--constraints", "--max-constraints", 2)
    assert r.returncode == 1 and r.stdout.strip().split("\n")[-1].endswith("(the first 2 are listed)") and json.loads(out.read_text())["constraints"]["truncated"]
    r = _cli("check", bl, out, "--host", "--constraints")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("balanced: ") and lines[1].startswith("satisfied: ") and json.loads(out.read_text())["constraints"]["satisfied"]


def test_cli_check_without_the_flag_is_what_it_was(tmp_path):
    """`check` without --constraints on store_byte: the six lines, the key set and the exit status that tests/test_bus_audit_cpu.py pins."""
    sb, out = tmp_path / "store_byte.bin", tmp_path / "report.json"
    sb.write_bytes(vp.machine_code(vp.store_byte_program()))
    r = _cli("check", sb, out, "--host")
    assert r.returncode == 1, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 6 and lines[-1].startswith("unbalanced: 5 tuples")
    for line, clk in zip(lines, (4, 6, 8, 10, 13)):
        assert line.startswith("memory bus [1, %d, " % clk) and line.endswith("cycle %d: pc %d STOREU8" % (clk, clk)) and "mem row" in line and "net -1" in line
    j = json.loads(out.read_text())
    assert set(j) == {"balanced", "truncated", "total_unbalanced", "reported", "device_ms", "host_ms", "buses", "tuples"}
    assert j["total_unbalanced"] == 5 and not j["balanced"] and not j["truncated"]
    # with the flag the same witness: the bus lines unchanged, the AIR clean, still exit 1
    r2 = _cli("check", sb, out, "--host", "--constraints")
    assert r2.returncode == 1 and r2.stdout.strip().split("\n")[:6] == lines and r2.stdout.strip().split("\n")[6].startswith("satisfied: ")
