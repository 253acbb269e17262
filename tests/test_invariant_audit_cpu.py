"""The invariant audit without a GPU: the host implementation of the contract (vgpu_invariant_audit_host) against the restatement of
tests/invariant_audit_ref.py (numpy RREF of the augmented rows; enforcement judged on the null-space side, the Jacobian by the rank audit
reference's interpolation of the oracle's chips) word for word, for both machine kinds; the facts the reference finds on fib(25) and alu(50);
holds() as a certificate; captured analytic AIRs with closed forms (width 5 and the lane-word boundary 63 / 64 / 65); the needle traces;
limits, chip mask, the cut at max_terms; the API edges of tests/test_audit_api_cpu.py applied to this audit; `check --host --invariants`; the
device kernels' very source under tools/hipemu; the C ABI's new symbols; the host audit under AddressSanitizer and UBSan as a stand-alone
program.  The reference of each input is computed once per module and cut to the limits a test asks for.  The figures pinned here are the
reference's, not the code under test's."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import invariant_audit_cases as cases
import invariant_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, BITWISE, CPU, MEM, MUL, RANGE, SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
PROGRAM = 1
ALL = dict(max_entries=1 << 20, max_rows_per_entry=4096, max_terms=256)
INPUTS = {"fib1": lambda: va.Workload.fib(1), "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50)}
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
        _reference[name] = ref.audit(machines["basic"], mt, prep, **ALL)
    return ref.recut(_reference[name], **limits) if limits else ref.recut(_reference[name], 1024, 4, 8)


def both(machines, name, **limits):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, **limits)
    mt, prep = witness(name)
    reps = {k: va.invariant_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


def relations_of(rep, chip):
    return {e["column"]: e for e in rep.entries if e["chip"] == chip and e["kind"] == "relation"}


# ---- 1. the host audit equals the reference; the facts the reference finds ----------------------------------------------------------------------
def test_fib1_every_chip(machines):
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and not rep.truncated and rep.total_entries == rep.reported > 0
    for c in rep.chips:
        assert c["rank"] + c["invariants"] == c["width"] + 1 and c["constant_columns"] + c["relations"] == c["invariants"] == c["every"] + c["some"] + c["never"]
        if c["height"] == 1:  # one row: every column is a constant column
            assert (c["rank"], c["constant_columns"]) == (1, c["width"])
    both(machines, "fib1", max_entries=1 << 20, max_rows_per_entry=64, max_terms=3)


def test_fib25_pinned_facts(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=4, max_terms=16)
    c = rep.chips[ADD]
    assert (c["height"], c["width"], c["invariants"], c["constant_columns"], c["relations"], c["every"]) == (128, 16, 7, 4, 3, 7 - c["some"] - c["never"])
    rel = relations_of(rep, ADD)
    # the carry chain: -c1 - c5 - c9 + c12, -c2 - c6 - c8 + 256 c9 + c13, -c3 - c7 + 256 c8 + c14, each enforced on every row
    assert sorted(rel) == [12, 13, 14] and all(e["enforced_rows"] == 128 and e["free_rows"] == 0 and e["rows"] == [] and e["l0"] == 0 for e in rel.values())
    assert rel[12]["terms"] == [(1, P - 1), (5, P - 1), (9, P - 1), (12, 1)]
    assert rel[13]["terms"] == [(2, P - 1), (6, P - 1), (8, P - 1), (9, 256), (13, 1)]
    assert rel[14]["terms"] == [(3, P - 1), (7, P - 1), (8, 256), (14, 1)]
    c = rep.chips[CPU]
    assert (c["height"], c["width"], c["invariants"], c["constant_columns"]) == (256, 51, 23, 17)
    assert {k: e["enforced_rows"] for k, e in relations_of(rep, CPU).items()} == {22: 105, 24: 105, 29: 256, 36: 256, 38: 104, 43: 105}
    c = rep.chips[MEM]
    assert (c["invariants"], c["constant_columns"], c["relations"]) == (6, 6, 0)
    assert rep.chips[RANGE]["invariants"] == rep.chips[PROGRAM]["invariants"] == 0 and rep.relations(ADD) == [12, 13, 14] and len(rep.constant_columns(ADD)) == 4
    for e in rep.entries:
        n = rep.chips[e["chip"]]["height"]
        assert e["enforced_rows"] + e["free_rows"] == n and e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(4, e["free_rows"])
        assert e["terms"][-1] == (e["column"], 1) or e["support"] > len(e["terms"])


def test_alu50_pinned_facts(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20, max_rows_per_entry=7, max_terms=32)
    c = rep.chips[BITWISE]
    assert (c["height"], c["width"], c["relations"], c["constant_columns"]) == (256, 79, 14, 0)
    rel = relations_of(rep, BITWISE)
    assert sorted(rel) == [15, 23, 31, 39, 47, 55, 63, 71, 73, 74, 75, 76, 77, 78]
    assert all(rel[k]["enforced_rows"] == 256 for k in (15, 23, 31, 39, 47, 55, 63, 71, 78)) and all(rel[k]["enforced_rows"] == 150 for k in (73, 74, 75, 76, 77))
    assert rel[78]["terms"] == [(32, 1), (64, P - 1), (78, 1)] and rel[78]["l0"] == 0
    # the line this audit exists to print: a relation of cpu's column 38 that no row enforces
    e = relations_of(rep, CPU)[38]
    assert rep.chips[CPU]["height"] == 512 and (e["enforced_rows"], e["free_rows"], e["rows"]) == (0, 512, list(range(7))) and e["support"] + int(e["l0"] != 0) == 13
    assert 38 in rep.never_enforced(CPU) and 38 in ref_never(want, CPU)


def ref_never(want, chip):
    return [e["column"] for e in want["entries"] if e["chip"] == chip and e["enforced_rows"] == 0]


# ---- 2. holds() ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib25", "alu50"])
def test_holds_on_the_audited_traces_and_names_a_broken_entry(machines, name):
    mt, prep = witness(name)
    rep = va.invariant_audit_host(machines["basic"], mt, prep, **ALL)
    assert rep.holds(mt) == []
    e = [e for e in rep.entries if e["chip"] == ADD and e["kind"] == "relation"][-1]
    broken = [m.copy() for m in mt]
    broken[ADD][3, e["column"]] = (int(broken[ADD][3, e["column"]]) + 1) % P  # column f occurs in its own invariant only (the others are pivots or not in it)
    assert rep.holds(broken) == [(ADD, e["column"])]
    # one witness's invariants against another program's traces: which of cpu's, mem's and add's do not survive the other program.  Of add's
    # carry chain under fib(25), columns 13 and 14 also hold on alu(50); column 12's form there was an accident of small addends.
    other = witness("alu50" if name == "fib25" else "fib25")[0]
    failing = CROSS_FAILING[name]
    assert [x for x in rep.holds(other) if x[0] in (CPU, MEM, ADD)] == failing
    want = reference(machines, name, **ALL)  # the same from the reference's vectors, evaluated here
    got = []
    for e in want["entries"]:
        if e["chip"] in (CPU, MEM, ADD):
            m = other[e["chip"]].astype(object)
            if any((e["l0"] + sum(int(c) * int(row[k]) for k, c in e["terms"])) % P for row in m):
                got.append((e["chip"], e["column"]))
    assert got == failing


CROSS_FAILING = {"fib25": [(CPU, 7), (CPU, 22), (CPU, 24), (CPU, 32), (CPU, 38), (CPU, 39), (CPU, 43), (CPU, 46), (MEM, 1), (ADD, 0), (ADD, 4), (ADD, 10), (ADD, 11), (ADD, 12)],
                 "alu50": [(CPU, 2), (CPU, 18), (CPU, 20), (CPU, 21), (CPU, 24), (CPU, 29), (CPU, 36), (CPU, 38), (CPU, 43), (CPU, 45), (ADD, 5), (ADD, 12), (ADD, 15)]}


# ---- 3. captured analytic AIRs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 8])
def test_affine_air_width_5(n):
    machine, t = cases.affine_machine(), cases.affine_trace(n)
    rep = va.invariant_audit_host(machine, [t], [], max_rows_per_entry=8)
    want = ref.audit(machine, [t], [], max_rows_per_entry=8, jacobians=cases.affine_jacobians())
    ref.assert_report_equals(rep, want)
    assert np.array_equal(rep.words, ref.words(want)) and rep.holds([t]) == []
    if n == 8:
        c = rep.chips[0]
        assert (c["rank"], c["invariants"], c["constant_columns"], c["relations"], c["every"], c["some"], c["never"]) == (3, 3, 1, 2, 1, 0, 2)
        assert [(e["column"], e["kind"], e["l0"], e["terms"], e["enforced_rows"], e["rows"]) for e in rep.entries] == [
            (2, "relation", P - 7, [(0, P - 3), (2, 1)], 8, []), (3, "relation", 0, [(0, P - 1), (1, P - 1), (3, 1)], 0, list(range(8))),
            (4, "constant", P - 5, [(4, 1)], 0, list(range(8)))]


@pytest.mark.parametrize("width", [63, 64, 65])
def test_affine_air_at_the_lane_word_boundary(width):
    """Augmented widths 64, 65 and 66: the last invariant sits in the last lane of the first word, in the first lane of the second, and one beyond."""
    n = 128
    machine, t = cases.affine_machine(width), cases.affine_trace(n, width)
    rep = va.invariant_audit_host(machine, [t], [], max_rows_per_entry=2, max_terms=4)
    want = ref.audit(machine, [t], [], max_rows_per_entry=2, max_terms=4, jacobians=cases.affine_jacobians(width))
    assert np.array_equal(rep.words, ref.words(want))
    assert [(e["column"], e["enforced_rows"]) for e in rep.entries] == [(2, n), (3, 0), (4, 0), (width - 1, 0)] and rep.chips[0]["rank"] == width - 3
    assert rep.entries[-1]["terms"] == [(0, P - 2), (width - 2, P - 1), (width - 1, 1)] and rep.entries[-1]["l0"] == P - 1


# ---- 4. needle traces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["first", "last", "stairs"])
def test_needle_traces(kind):
    machine, t = cases.free_machine(cases.NEEDLE_W), cases.needle(kind)
    rep = va.invariant_audit_host(machine, [t], [])
    want = ref.audit(machine, [t], [], jacobians=cases.free_jacobians(cases.NEEDLE_W))
    assert np.array_equal(rep.words, ref.words(want))
    assert rep.relations(0) == cases.NEEDLE_INVARIANTS[kind] and rep.constant_columns(0) == []
    assert all(e["enforced_rows"] == 0 and e["rows"] == [0, 1, 2, 3] for e in rep.entries)  # nothing is constrained: free on every row
    by = {e["column"]: e for e in rep.entries}
    assert by[68]["terms"] == [(5, P - 2), (68, 1)] and by[68]["l0"] == P - 7
    if kind == "stairs":
        assert by[69]["terms"] == [(0, P - 1), (67, P - 1), (69, 1)]
    else:  # without the one row the relation of column 69 would hold
        row = 0 if kind == "first" else cases.NEEDLE_N - 1
        healed = t.copy()
        healed[row, 69] = (int(healed[row, 69]) + P - 1) % P
        assert va.invariant_audit_host(machine, [healed], []).relations(0) == [68, 69]


# ---- 5. limits, chip mask, max_terms ----------------------------------------------------------------------------------------------------------------
def test_limits_keep_totals_exact(machines):
    want, rep = both(machines, "fib25", max_entries=9, max_rows_per_entry=2, max_terms=2)
    full = reference(machines, "fib25", **ALL)
    assert rep.truncated and rep.reported == 9 and rep.total_entries == full["total_entries"] > 9
    assert rep.chips == [dict(c) for c in full["chips"]]  # per-chip counts do not depend on the limits
    assert all(len(e["rows"]) <= 2 and len(e["terms"]) <= 2 for e in rep.entries)
    with pytest.raises(va.VgpuError):
        va.invariant_audit_host(machines["basic"], *witness("fib25"), max_entries=0)
    with pytest.raises(va.VgpuError):
        va.invariant_audit_host(machines["basic"], *witness("fib25"), max_terms=0)
    with pytest.raises(va.VgpuError, match="max_terms is at most 4096"):
        va.invariant_audit_host(machines["basic"], *witness("fib25"), max_terms=5000)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    rep = va.invariant_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM])
    want = ref.audit(machines["basic"], mt, prep, chips=[ADD, MEM])
    assert np.array_equal(rep.words, ref.words(want))
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and {e["chip"] for e in rep.entries} == {MEM, ADD}
    for c in rep.chips:
        if not c["audited"]:  # a zero block that keeps the chip's shape
            assert c["width"] > 0 and c["height"] > 0 and (c["rank"], c["invariants"], c["constant_columns"], c["relations"], c["every"], c["some"], c["never"]) == (0,) * 7
    with pytest.raises(va.VgpuError, match="chip_mask names a chip the machine does not have"):
        va.invariant_audit_host(machines["basic"], mt, prep, chips=[20])


def test_max_terms_cut_and_holds_refuses(machines):
    mt, prep = witness("fib25")
    rep = va.invariant_audit_host(machines["basic"], mt, prep, max_terms=3)
    e = [e for e in rep.entries if e["chip"] == ADD and e["column"] == 13][0]
    assert (e["support"], e["terms"]) == (5, [(2, P - 1), (6, P - 1), (8, P - 1)])  # the first three, ascending; the support stays exact
    with pytest.raises(va.VgpuError, match="is cut"):
        rep.holds(mt)
    assert va.invariant_audit_host(machines["basic"], mt, prep, max_terms=3, chips=[MEM]).holds(mt) == []  # constant columns have one term


# ---- 6. the API edges of tests/test_audit_api_cpu.py, for this audit ------------------------------------------------------------------------------
def test_signatures():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_entries", 1024, kind), ("max_rows_per_entry", 4, kind), ("max_terms", 8, kind), ("chips", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.invariant_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.invariant_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert signature_of(va.InvariantReport.holds) == [("self", empty, kind), ("main_matrices", empty, kind)]


def test_a_trace_is_a_matrix(machines):
    for args in (([np.zeros(4, dtype=np.uint32)], []), ([], [(0, np.zeros(4, dtype=np.uint32))])):
        with pytest.raises(va.VgpuError) as e:
            va.invariant_audit_host(machines["basic"], *args)
        assert e.value.code == -1 and str(e.value) == "vgpu error -1: invariant_audit: traces are two-dimensional matrices"


@pytest.mark.parametrize("chips", [[], [32]])
def test_chip_lists(machines, chips):
    with pytest.raises(va.VgpuError) as e:
        va.invariant_audit_host(machines["basic"], [], [], chips=chips)
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: invariant_audit: chips is a non-empty list of chip indices below 32"


def test_null_out_and_null_report_handle(machines):
    L = ctypes.CDLL(va.lib()._name)  # a handle of its own: the restypes set here are not the package's
    f = L.vgpu_invariant_audit_host
    f.restype = ctypes.c_int32
    L.vgpu_last_error.restype = ctypes.c_char_p
    assert f(machines["basic"]._h, None, None, None, ctypes.c_uint32(0), None, None, None, None, ctypes.c_uint32(0), None, None) == -1
    assert L.vgpu_last_error()
    length, words, timing, free = (getattr(L, "vgpu_invariant_report_%s" % x) for x in ("len", "words", "timing", "free"))
    length.restype, words.restype, timing.restype, free.restype = ctypes.c_uint64, ctypes.c_void_p, None, None
    assert length(None) == 0 and words(None) is None
    tm = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    timing(None, tm)
    assert list(tm) == [0.0, 0.0, 0.0]
    free(None)


def test_reserved_fields_and_null_options(machines):
    mt, prep = witness("fib1")
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    n, k = len(mains), len(preps)

    def call(opts):
        h = ctypes.c_void_p()
        rc = L.vgpu_invariant_audit_host(machines["basic"]._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                         (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in preps]),
                                         (ctypes.c_void_p * k)(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * k)(*[m.shape[0] for _, m in preps]),
                                         (ctypes.c_uint64 * k)(*[m.shape[1] for _, m in preps]), ctypes.c_uint32(k), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
        return rc, (va._audit_report("invariant", va.InvariantReport, h).words if rc == 0 else None)

    want = va.invariant_audit_host(machines["basic"], mt, prep).words
    rc, words = call(None)  # NULL options: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = call(va.InvariantAuditOpts(0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 0, 0)))  # zero fields: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, _ = call(va.InvariantAuditOpts(0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 1, 0)))
    assert rc == -1  # reserved != 0 is refused


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_invariants_on_the_host(tmp_path, machines):
    from valida_amd.cli import index_ranges

    bl, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out_plain, "--host")
    r = _cli("check", bl, out, "--host", "--invariants")
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.invariant_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20, max_terms=256)
    expect = []
    for c in rep.chips:
        if not c["invariants"]:
            continue
        mine = [e for e in rep.entries if e["chip"] == c["chip"]]
        head = "%d invariant%s" % (c["invariants"], "" if c["invariants"] == 1 else "s")
        if c["constant_columns"]:
            loose = len([e for e in mine if e["kind"] == "constant" and e["enforced_rows"] == 0])
            head += " (%d constant column%s%s)" % (c["constant_columns"], "" if c["constant_columns"] == 1 else "s", ", %d never enforced" % loose if loose else "")
        parts = [head]
        rel = [e for e in mine if e["kind"] == "relation"]
        for label, cols in (("enforced on every row", [e["column"] for e in rel if not e["free_rows"]]),
                            ("enforced on some rows", [e["column"] for e in rel if e["free_rows"] and e["enforced_rows"]]),
                            ("never enforced", [e["column"] for e in rel if not e["enforced_rows"]])):
            if cols:
                parts.append("%s: columns %s" % (label, index_ranges(cols)))
        expect.append("%s: %s" % (va.CHIP_NAMES[c["chip"]], "; ".join(parts)))
    assert expect and lines[len(before):] == expect and any("enforced on every row: columns" in x for x in expect)
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    assert set(j) == set(plain_json) | {"invariants"} and "invariants" not in plain.stdout
    assert {k: v for k, v in j.items() if k not in ("invariants", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["invariants"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--invariants", "--chips=add,4")
    j = json.loads(out.read_text())["invariants"]
    assert r.returncode == 0 and [c["chip"] for c in j["chips"] if c["audited"]] == [ADD, SUB]
    help_text = _cli("--help").stdout
    assert "--invariants" in help_text and "never changes the exit status" in help_text


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "invariant_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libinvariantauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "invariant_audit.hpp"), os.path.join(csrc, "host", "rank_audit.hpp"),
            os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("invariant_audit.hip", "rank_elim.hpp", "rank_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_invariant_audit.restype = ctypes.c_int64
    return L


def emulated(emu, machine_kind, mt, prep, interpret, rows_per_wave=0, rows_per_basis=0, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(8 + 14 * n + sum(m.shape[1] for m in keep[:n]) * (12 + 2 * min(max_terms, 256) + min(max_rows_per_entry, 4096)), np.uint32)
    got = emu.emu_invariant_audit(
        ctypes.c_uint32(machine_kind), (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]),
        (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]), ctypes.c_uint32(n), (ctypes.c_uint32 * max(1, k))(*[c for c, _ in prep]), (ctypes.c_void_p * max(1, k))(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * max(1, k))(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * max(1, k))(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(rows_per_wave), ctypes.c_uint32(rows_per_basis), ctypes.c_uint32(max_entries), ctypes.c_uint32(max_rows_per_entry), ctypes.c_uint32(max_terms),
        ctypes.c_uint32(sum(1 << c for c in chips) if chips else 0), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """k_ia_basis, k_ia_merge, the counting pass, the scan and the listing pass of invariant_audit.hip (with rank_elim.hpp and the rank audit's
    scan kernel) with the wave primitives in their emulation forms (a wave is a 64-thread workgroup): the compiled chip templates, the
    interpreted register programs and the bus-only chips; the assembled report is the host audit's, word for word.  fib(1) without mul (1024
    rows; the emulated ballots are slow), then with 3 rows per workgroup in both phases: the merge eliminates many partial bases
    (mem: 22 of them, two levels of the tree), and the r - 1 halo, the wrap and the rank scan of the lists cross workgroup boundaries; bitwise has 79 columns (80
    augmented: two words per lane).  NOT covered here: more than one wave per workgroup in the listing pass (the GPU tests: fib(582))."""
    mt, prep = witness("fib1")
    chips = [c for c in range(14) if c != MUL]
    host = va.invariant_audit_host(machines["basic"], mt, prep, chips=chips)
    assert host.relations(CPU) and host.chips[BITWISE]["invariants"] == 79
    assert np.array_equal(emulated(emu, 0, mt, prep, interpret, chips=chips), host.words)
    some = [CPU, MEM, ADD, BITWISE, RANGE]
    host = va.invariant_audit_host(machines["basic"], mt, prep, chips=some, max_rows_per_entry=20, max_entries=30, max_terms=3)
    assert host.truncated and any(len(e["rows"]) == 20 and e["rows"][-1] - e["rows"][0] > 6 for e in host.entries)
    assert np.array_equal(emulated(emu, 0, mt, prep, interpret, rows_per_wave=3, rows_per_basis=3, chips=some, max_rows_per_entry=20, max_entries=30, max_terms=3), host.words)


def test_the_79_column_chip_under_emulation(machines, emu):
    """alu(50)'s bitwise trace (79 columns, relations of up to 21 terms, some of them enforced on some rows only), 7 rows per phase-1 workgroup."""
    mt, prep = witness("alu50")
    mt = [np.ascontiguousarray(m[128:192]) if c == BITWISE else m for c, m in enumerate(mt)]  # 64 rows, operations and padding: the emulated ballots are slow
    host = va.invariant_audit_host(machines["basic"], mt, prep, chips=[BITWISE], max_terms=32, max_rows_per_entry=120)
    assert host.chips[BITWISE]["relations"] >= 14 and host.chips[BITWISE]["some"] > 0
    assert np.array_equal(emulated(emu, 0, mt, prep, 0, rows_per_wave=5, rows_per_basis=7, chips=[BITWISE], max_terms=32, max_rows_per_entry=120), host.words)


@pytest.mark.parametrize("n,width", [(1, 5), (2, 5), (8, 5), (128, 63), (128, 64), (128, 65)])
def test_affine_airs_under_emulation(emu, n, width):
    machine, t = cases.affine_machine(width), cases.affine_trace(n, width)
    host = va.invariant_audit_host(machine, [t], [], max_rows_per_entry=8)
    assert np.array_equal(emulated(emu, 3, [t], [], 1, rows_per_wave=3 if n > 2 else 0, rows_per_basis=3 if n == 8 else (40 if n > 8 else 0), max_rows_per_entry=8), host.words)


@pytest.mark.parametrize("kind", ["first", "last", "stairs"])
def test_needle_traces_under_emulation(emu, kind):
    """The needle traces' first 512 rows (the emulated ballots are slow; 'last' keeps its broken row as the last one), 16 rows per phase-1
    workgroup: 32 partial bases for the merge (two levels of its tree), with other pivots from block to block of the staircase."""
    t = cases.needle(kind)
    t = np.ascontiguousarray(t[-512:] if kind == "last" else t[:512])
    host = va.invariant_audit_host(cases.free_machine(cases.NEEDLE_W), [t], [])
    # stairs: of the staircase's 58-row blocks only nine begin in these rows, so columns 9..67 are still zero (constant columns) and column
    # 69 = c67 + c0 reads as c0
    assert host.relations(0) == ([68, 69] if kind == "stairs" else [68]) and host.constant_columns(0) == (list(range(9, 68)) if kind == "stairs" else [])
    assert np.array_equal(emulated(emu, 2, [t], [], 1, rows_per_basis=16), host.words)


def ia_shape(emu, w, K, d, n=1 << 20, prep_width=0, n_regs=0, interpret=0):
    out = (ctypes.c_uint64 * 6)()
    emu.emu_ia_shape.restype = ctypes.c_int32
    rc = emu.emu_ia_shape(ctypes.c_uint32(w), ctypes.c_uint32(prep_width), ctypes.c_uint32(K), ctypes.c_uint32(n_regs), ctypes.c_uint32(interpret), ctypes.c_uint64(n), ctypes.c_uint32(d), out)
    return rc, dict(zip(("NW", "RPW", "T", "NB", "bytes", "rank_bytes"), [int(x) for x in out]))


def test_a_shape_the_audit_accepts_is_one_the_listing_pass_accepts(emu):
    """The listing pass goes through the rank audit's scan launcher, which checks the rank audit's LDS bytes for the shape it is given.  With
    few invariants this audit's own bytes are the smaller of the two (it keeps (3 + NW + w) d words where the rank audit keeps (5 + NW) w), so
    the shape function must fit both: a chip is refused by ia_shape, with the arithmetic, or passes every later check.  w = 40, K = 192,
    n = 2^20, d = 1 is a chip whose own bytes fit NW = 4, RPW = 16 (162684) where the rank audit's do not (163936); the sweep covers the
    widths and constraint counts around the LDS limit, captured (interpreted, 40 registers) and compiled, with and without preprocessed columns."""
    LDS = 160 * 1024
    rc, sh = ia_shape(emu, 40, 192, 1)
    assert rc == 0 and sh["rank_bytes"] <= sh["bytes"] <= LDS and sh["T"] == sh["NW"] * sh["RPW"] and sh["NB"] == ((1 << 20) + sh["T"] - 1) // sh["T"], sh
    seen = {0: 0, 1: 0}
    for w in list(range(8, 150, 3)) + [1, 2, 191]:
        for K in range(0, 200, 3):
            for d in {1, 2, 4, w} if w > 4 else {1, w}:
                for extra in (dict(), dict(interpret=1, n_regs=40, prep_width=3)):
                    if extra and not K:
                        continue
                    rc, sh = ia_shape(emu, w, K, d, **extra)
                    assert rc in (0, 1), (w, K, d, extra, sh)  # never a shape that a later launcher throws on
                    seen[rc] += 1
                    if rc == 0:
                        assert sh["NW"] in (1, 2, 4) and sh["rank_bytes"] <= sh["bytes"] <= LDS, (w, K, d, extra, sh)
    assert seen[0] > 1000 and seen[1] > 0  # both sides of the limit were visited


# ---- 9. C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_invariant_audit", "vgpu_invariant_audit_host", "vgpu_invariant_report_len", "vgpu_invariant_report_words", "vgpu_invariant_report_timing",
             "vgpu_invariant_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Invariant audit" in header and "vgpu_invariant_audit_opts_t" in header and ctypes.sizeof(va.InvariantAuditOpts) == 32


# ---- 10. the host audit under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path, machines):
    """tests/emu/invariant_audit_host.cpp: fib(25) on the host VM and the host invariant audit, built with AddressSanitizer and UBSan and run
    as a subprocess (nothing sanitized is loaded into this interpreter).  Its figures are the library's for the same limits."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "invariant_audit_host")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "emu", "invariant_audit_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe, "25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    mt, prep = witness("fib25")
    rep = va.invariant_audit_host(machines["basic"], mt, prep, max_entries=1 << 20, max_rows_per_entry=64, max_terms=16)
    assert ("fib(25): %d words, %d entries, %d relations, %d enforced on every row, %d on none" % (
        len(rep.words), rep.total_entries, sum(c["relations"] for c in rep.chips), sum(c["every"] for c in rep.chips), sum(c["never"] for c in rep.chips))) in r.stdout, r.stdout
