"""The product audit without a GPU: the host implementation of the contract (vgpu_product_audit_host) against the restatement of
tests/product_audit_ref.py (per pair the numpy RREF of the pivot columns and the product column; enforcement judged on the null-space side, the
Jacobian by the rank audit reference's interpolation of the oracle's chips) word for word, for both machine kinds; the facts the reference finds
on fib(25) and alu(50); holds() as a certificate; the captured analytic AIR "quad" with closed forms (n = 1, 2, 8, 16 and the lane-word boundary
63 / 64 / 65); the needle traces; limits, chip mask, the cut at max_terms; the API edges of tests/test_audit_api_cpu.py applied to this audit;
`check --host --products`; the device kernels' very source under tools/hipemu; the C ABI's new symbols; the host audit under AddressSanitizer
and UBSan as a stand-alone program.  The reference of each input is computed once per module and cut to the limits a test asks for.  The
figures pinned here are the reference's, not the code under test's."""
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

import product_audit_cases as cases
import product_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, BITWISE, CPU, MEM, SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
LT = 8
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
    reps = {k: va.product_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


def counts(c):
    return (c["rank"], c["pairs"], c["relations"], c["boolean"], c["zero"])


def entry(rep, chip, i, j):
    return [e for e in rep.entries if (e["chip"], e["i"], e["j"]) == (chip, i, j)][0]


# ---- 1. the host audit equals the reference; the facts the reference finds ----------------------------------------------------------------------
def test_fib1_every_chip(machines):
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and not rep.truncated and rep.total_entries == rep.reported > 0
    for c in rep.chips:
        q = c["independent"]
        assert c["rank"] == q + 1 and c["pairs"] == q * (q + 1) // 2 and c["boolean"] + c["zero"] + c["select"] + c["other"] == c["relations"] == c["every"] + c["some"] + c["never"]
        if c["height"] == 1:  # one row: no independent column
            assert (c["rank"], q, c["pairs"], c["relations"]) == (1, 0, 0, 0)
    both(machines, "fib1", max_entries=1 << 20, max_rows_per_entry=64, max_terms=3)


def test_fib25_pinned_facts(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20, max_rows_per_entry=4, max_terms=16)
    assert counts(rep.chips[CPU]) == (29, 406, 213, 10, 65) and counts(rep.chips[MEM]) == (9, 36, 4, 3, 1) and counts(rep.chips[ADD]) == (10, 45, 29, 5, 7)
    # enforced on every row: the opcode flags cpu's eval hands to assert_bool (IS_BUS_OP 9, IS_IMM_OP 11, IS_BEQ 18, IS_BNE 19, IS_JAL 20, IS_JALV 21,
    # NOT_EQUAL 28), add's two used carries 8, 9 and IS_REAL 15
    for chip, n, cols in ((CPU, 256, (9, 11, 18, 19, 20, 21, 28)), (ADD, 128, (8, 9, 15))):
        for k in cols:
            e = entry(rep, chip, k, k)
            assert (e["kind"], e["b0"], e["terms"], e["enforced_rows"], e["free_rows"], e["flat_rows"], e["rows"]) == ("boolean", 0, [(k, 1)], n, 0, 0, [])
    # mem: IS_READ IS_WRITE = 0 holds by the chip's constraints on every row, 111 of them flat (padding: both flags 0); the flags' own booleanity
    # is enforced on the 401 real rows only
    e = entry(rep, MEM, 7, 8)
    assert (e["kind"], e["support"], e["enforced_rows"], e["flat_rows"]) == ("zero", 0, 512, 111)
    assert [(e["i"], e["enforced_rows"], e["rows"]) for e in rep.entries if e["chip"] == MEM and e["kind"] == "boolean"] == [(k, 401, [401, 402, 403, 404]) for k in (2, 7, 8)]
    # enforced on no row: IS_BUS_OP times column 49 is a five-term affine function on this witness, and nothing in cpu's eval says so
    e = entry(rep, CPU, 9, 49)
    assert (e["kind"], e["terms"], e["enforced_rows"], e["free_rows"], e["rows"]) == ("other", [(8, P - 1), (11, 1), (20, P - 120), (21, P - 40), (49, 1)], 0, 256, [0, 1, 2, 3])
    assert (9, 49) in rep.never_enforced(CPU) and rep.chips[CPU]["never"] == 6 and len(rep.relations(ADD)) == 29
    for e in rep.entries:
        n = rep.chips[e["chip"]]["height"]
        assert e["enforced_rows"] + e["free_rows"] == n and e["flat_rows"] <= e["enforced_rows"] and e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(4, e["free_rows"])
        assert e["i"] <= e["j"] and len(e["terms"]) == min(e["support"], 16)


def test_alu50_pinned_facts(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20, max_rows_per_entry=7, max_terms=32)
    assert counts(rep.chips[CPU])[1:] == (406, 136, 5, 45) and counts(rep.chips[SUB])[:3] == (6, 15, 5) and counts(rep.chips[LT])[:3] == (25, 300, 91)
    assert counts(rep.chips[BITWISE]) == (66, 2145, 301, 56, 10) and rep.chips[BITWISE]["never"] == 0 and rep.chips[CPU]["never"] == 31


# ---- 2. holds() ------------------------------------------------------------------------------------------------------------------------------
def test_holds_on_the_audited_traces_and_names_a_broken_entry(machines):
    mt, prep = witness("fib25")
    rep = va.product_audit_host(machines["basic"], mt, prep, **ALL)
    assert rep.holds(mt) == []
    broken = [m.copy() for m in mt]
    broken[MEM][3, 7] = 2  # IS_READ = 2 on one row: its booleanity and its product with IS_WRITE's complement break, nothing else of mem's
    bad = rep.holds(broken)
    assert (MEM, 7, 7) in bad and all(x[0] == MEM and 7 in x[1:] for x in bad)
    other = witness("alu50")[0]  # one witness's relations against another program's traces
    failing = rep.holds(other)
    want = reference(machines, "fib25", **ALL)  # the same from the reference's betas, evaluated here
    got = []
    for e in want["entries"]:
        m = other[e["chip"]].astype(object)
        if any((e["b0"] + sum(int(c) * int(row[k]) for k, c in e["terms"]) - int(row[e["i"]]) * int(row[e["j"]])) % P for row in m):
            got.append((e["chip"], e["i"], e["j"]))
    assert got == failing and 0 < len(failing) < rep.total_entries and (MEM, 7, 8) not in failing


# ---- 3. the captured analytic AIR ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 8, 16])
def test_quad_air_width_7(n):
    machine, t = cases.quad_machine(), cases.quad_trace(n)
    rep = va.product_audit_host(machine, [t], [], max_rows_per_entry=8)
    want = ref.audit(machine, [t], [], max_rows_per_entry=8, jacobians=cases.quad_jacobians(t))
    ref.assert_report_equals(rep, want)
    assert np.array_equal(rep.words, ref.words(want)) and rep.holds([t]) == []
    c = want["chips"][0]
    if n == 1:
        assert (c["rank"], c["independent"], c["pairs"], want["entries"]) == (1, 0, 0, [])
    if n == 2:  # c0 = 0, 1: the one independent column is its own square
        assert (c["rank"], c["pairs"]) == (2, 1) and [(e["i"], e["j"], e["b0"], e["terms"]) for e in want["entries"]] == [(0, 0, 0, [(0, 1)])]
    if n == 16:
        assert {(e["i"], e["j"]): e["terms"] for e in want["entries"]} == {k: [(col, 1)] for k, col in cases.QUAD_RELATIONS.items()} and c["rank"] == 7
        by = {(e["i"], e["j"]): e for e in want["entries"]}
        assert (by[(1, 1)]["kind"], by[(1, 1)]["enforced_rows"], by[(1, 2)]["enforced_rows"], by[(2, 2)]["kind"], by[(2, 2)]["enforced_rows"]) == ("boolean", n, n, "boolean", 0)
        assert (by[(1, 3)]["kind"], by[(1, 3)]["flat_rows"]) == ("select", n // 4) and all(e["b0"] == 0 for e in want["entries"])


@pytest.mark.parametrize("width", [63, 64, 65])
def test_quad_air_at_the_lane_word_boundary(width):
    """rho = width (c5 is no pivot): 63, 64 and 65 compacted columns, one lane word and one column into the second."""
    n = 128
    machine, t = cases.quad_machine(width), cases.quad_trace(n, width)
    rep = va.product_audit_host(machine, [t], [], max_rows_per_entry=2, max_terms=4)
    want = ref.audit(machine, [t], [], max_rows_per_entry=2, max_terms=4, jacobians=cases.quad_jacobians(t))
    assert np.array_equal(rep.words, ref.words(want))
    q = width - 1
    assert (rep.chips[0]["rank"], rep.chips[0]["pairs"]) == (width, q * (q + 1) // 2) and rep.relations(0) == sorted(cases.QUAD_RELATIONS)
    assert rep.never_enforced(0) == [(0, 0), (0, 1), (2, 2)]


# ---- 4. needle traces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["first", "last", "clean"])
def test_needle_traces(kind):
    machine, t = cases.free_machine(cases.NEEDLE_W), cases.needle(kind)
    rep = va.product_audit_host(machine, [t], [])
    want = ref.audit(machine, [t], [], jacobians=cases.free_jacobians(cases.NEEDLE_W))
    assert np.array_equal(rep.words, ref.words(want))
    assert [(e["i"], e["j"]) for e in want["entries"]] == cases.NEEDLE_RELATIONS[kind] and want["chips"][0]["rank"] == 41
    # nothing is constrained: free wherever the gradient is not zero (c1 c2 = c3 is never flat; c1 c3 = c3 is flat where c1 = 1 and c3 = 0 .. )
    by = {(e["i"], e["j"]): e for e in rep.entries}
    assert all(e["enforced_rows"] == e["flat_rows"] for e in rep.entries) and by[(1, 2)]["free_rows"] == cases.NEEDLE_N and by[(4, 4)]["terms"] == [(5, 1)]
    if kind == "clean":
        assert by[(0, 6)]["terms"] == [(7, 1)]


# ---- 5. limits, chip mask, max_terms ----------------------------------------------------------------------------------------------------------------
def test_limits_keep_totals_exact(machines):
    want, rep = both(machines, "fib25", max_entries=9, max_rows_per_entry=2, max_terms=2)
    full = reference(machines, "fib25", **ALL)
    assert rep.truncated and rep.reported == 9 and rep.total_entries == full["total_entries"] == 246
    assert rep.chips == [dict(c) for c in full["chips"]]  # per-chip counts do not depend on the limits
    assert all(len(e["rows"]) <= 2 and len(e["terms"]) <= 2 for e in rep.entries)
    with pytest.raises(va.VgpuError):
        va.product_audit_host(machines["basic"], *witness("fib25"), max_entries=0)
    with pytest.raises(va.VgpuError):
        va.product_audit_host(machines["basic"], *witness("fib25"), max_terms=0)
    with pytest.raises(va.VgpuError, match="product_audit: max_terms is at most 4096"):
        va.product_audit_host(machines["basic"], *witness("fib25"), max_terms=5000)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    rep = va.product_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM])
    want = ref.audit(machines["basic"], mt, prep, chips=[ADD, MEM])
    assert np.array_equal(rep.words, ref.words(want))
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and {e["chip"] for e in rep.entries} == {MEM, ADD}
    for c in rep.chips:
        if not c["audited"]:  # a zero block that keeps the chip's shape
            assert c["width"] > 0 and c["height"] > 0 and all(c[k] == 0 for k in ("rank", "independent", "pairs", "relations", "boolean", "zero", "select", "other", "every", "some", "never"))
    with pytest.raises(va.VgpuError, match="product_audit: chip_mask names a chip the machine does not have"):
        va.product_audit_host(machines["basic"], mt, prep, chips=[20])


def test_max_terms_cut_and_holds_refuses(machines):
    mt, prep = witness("fib25")
    rep = va.product_audit_host(machines["basic"], mt, prep, max_terms=3)
    e = entry(rep, CPU, 9, 49)
    assert (e["support"], e["terms"]) == (5, [(8, P - 1), (11, 1), (20, P - 120)])  # the first three, ascending; the support stays exact
    with pytest.raises(va.VgpuError, match="is cut"):
        rep.holds(mt)
    assert va.product_audit_host(machines["basic"], mt, prep, max_terms=3, chips=[MEM]).holds(mt) == []  # mem's relations have one term at most


# ---- 6. the API edges of tests/test_audit_api_cpu.py, for this audit ------------------------------------------------------------------------------
def test_signatures():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_entries", 1024, kind), ("max_rows_per_entry", 4, kind), ("max_terms", 8, kind), ("chips", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.product_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.product_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert signature_of(va.ProductReport.holds) == [("self", empty, kind), ("main_matrices", empty, kind)]


def test_a_trace_is_a_matrix(machines):
    for args in (([np.zeros(4, dtype=np.uint32)], []), ([], [(0, np.zeros(4, dtype=np.uint32))])):
        with pytest.raises(va.VgpuError) as e:
            va.product_audit_host(machines["basic"], *args)
        assert e.value.code == -1 and str(e.value) == "vgpu error -1: product_audit: traces are two-dimensional matrices"


@pytest.mark.parametrize("chips", [[], [32]])
def test_chip_lists(machines, chips):
    with pytest.raises(va.VgpuError) as e:
        va.product_audit_host(machines["basic"], [], [], chips=chips)
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: product_audit: chips is a non-empty list of chip indices below 32"


def test_null_out_and_null_report_handle(machines):
    L = ctypes.CDLL(va.lib()._name)  # a handle of its own: the restypes set here are not the package's
    f = L.vgpu_product_audit_host
    f.restype = ctypes.c_int32
    L.vgpu_last_error.restype = ctypes.c_char_p
    assert f(machines["basic"]._h, None, None, None, ctypes.c_uint32(0), None, None, None, None, ctypes.c_uint32(0), None, None) == -1
    assert L.vgpu_last_error()
    length, words, timing, free = (getattr(L, "vgpu_product_report_%s" % x) for x in ("len", "words", "timing", "free"))
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
        rc = L.vgpu_product_audit_host(machines["basic"]._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                       (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in preps]),
                                       (ctypes.c_void_p * k)(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * k)(*[m.shape[0] for _, m in preps]),
                                       (ctypes.c_uint64 * k)(*[m.shape[1] for _, m in preps]), ctypes.c_uint32(k), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
        return rc, (va._audit_report("product", va.ProductReport, h).words if rc == 0 else None)

    want = va.product_audit_host(machines["basic"], mt, prep).words
    rc, words = call(None)  # NULL options: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = call(va.ProductAuditOpts(0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 0, 0)))  # zero fields: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, _ = call(va.ProductAuditOpts(0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 1, 0)))
    assert rc == -1  # reserved != 0 is refused


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_products_on_the_host(tmp_path, machines):
    bl, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out_plain, "--host")
    r = _cli("check", bl, out, "--host", "--products")
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.product_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20, max_terms=256)
    expect = []
    for c in rep.chips:
        if not c["relations"]:
            continue
        mine = [e for e in rep.entries if e["chip"] == c["chip"]]
        kinds = [len([e for e in mine if e["kind"] == k]) for k in ("boolean", "zero", "select", "other")]
        verdicts = (len([e for e in mine if not e["free_rows"]]), len([e for e in mine if e["free_rows"] and e["enforced_rows"]]), len([e for e in mine if not e["enforced_rows"]]))
        expect.append("%s: %d product relation%s of %d pair%s (%d boolean, %d zero, %d select, %d other); enforced on every row %d, on some rows %d, never %d" % (
            (va.CHIP_NAMES[c["chip"]], len(mine), "" if len(mine) == 1 else "s", c["pairs"], "" if c["pairs"] == 1 else "s") + tuple(kinds) + verdicts))
    assert expect and lines[len(before):] == expect and any(x.startswith("cpu: ") for x in expect)
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    assert set(j) == set(plain_json) | {"products"} and "product" not in plain.stdout
    assert {k: v for k, v in j.items() if k not in ("products", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["products"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--products", "--chips=add,4")
    j = json.loads(out.read_text())["products"]
    assert r.returncode == 0 and [c["chip"] for c in j["chips"] if c["audited"]] == [ADD, SUB]
    help_text = _cli("--help").stdout
    assert "--products" in help_text and "never changes the exit status" in help_text


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "product_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libproductauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "product_audit.hpp"), os.path.join(csrc, "host", "invariant_audit.hpp"),
            os.path.join(csrc, "host", "rank_audit.hpp"), os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"),
            os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("product_audit.hip", "invariant_audit.hip", "rank_elim.hpp", "rank_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_product_audit.restype = ctypes.c_int64
    return L


SMALL = dict(rows_per_wave=3, rows_per_slice=16, prefix_rows=64, group_entries=7, group_words=40)  # 3 rows per wave, 16 per slice, small entry groups


def emulated(emu, machine_kind, mt, prep, interpret, rows_per_wave=0, rows_per_slice=0, prefix_rows=0, group_entries=0, group_words=0, max_entries=1024, max_rows_per_entry=4, max_terms=8,
             chips=None):
    """The report image of the emulated device pass and its statistics: the most slices of basis rows of a chip, the pairs, the survivors of the
    prefix sweeps, the relations, the most entry groups of a chip."""
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k, u = len(mt), len(prep), ctypes.c_uint32
    out = np.zeros(1 << 21, np.uint32)
    stats = (ctypes.c_uint64 * 8)()
    got = emu.emu_product_audit(
        u(machine_kind), (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]),
        (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]), u(n), (u * max(1, k))(*[c for c, _ in prep]), (ctypes.c_void_p * max(1, k))(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * max(1, k))(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * max(1, k))(*[m.shape[1] for m in keep[n:]]), u(k), u(interpret),
        u(rows_per_wave), u(rows_per_slice), u(prefix_rows), u(group_entries), u(group_words), u(max_entries), u(max_rows_per_entry), u(max_terms),
        u(sum(1 << c for c in chips) if chips else 0), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size), stats)
    assert got > 0
    return out[:got], dict(zip(("slices", "pairs", "survivors", "relations", "groups"), [int(x) for x in stats]))


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """Every kernel of product_audit.hip (with rank_elim.hpp, the invariant audit's basis and merge kernels and the rank audit's scan kernel) with
    the wave primitives in their emulation forms (a wave is a 64-thread workgroup) on fib(25): the compiled chip templates, the interpreted
    register programs and the bus-only chips; the assembled report is the host audit's, word for word.  Every chip but cpu at its full height
    with 3 rows per wave, 16 rows per slice (mem: 32 slices, two levels of the row merge; its last basis row is row 401), a prefix sweep of 64
    rows whose survivors the second launch thins, and entry groups of at most 7 relations and 40 words; cpu (213 relations, the emulated ballots
    are slow) on its first 64 rows with the default sizes.  NOT covered here: more than one wave per workgroup (the GPU tests)."""
    mt, prep = witness("fib25")
    chips = [c for c in range(14) if c != CPU]
    host = va.product_audit_host(machines["basic"], mt, prep, chips=chips, max_rows_per_entry=20)
    assert host.chips[MEM]["relations"] == 4 and any(len(e["rows"]) == 20 for e in host.entries)
    got, st = emulated(emu, 0, mt, prep, interpret, chips=chips, max_rows_per_entry=20, **SMALL)
    assert np.array_equal(got, host.words)
    assert st["slices"] == 64 and st["groups"] > 4 and st["pairs"] > st["survivors"] > st["relations"] == host.total_entries, st
    head = [np.ascontiguousarray(m[:64]) if c == CPU else m for c, m in enumerate(mt)]
    host = va.product_audit_host(machines["basic"], head, prep, chips=[CPU], max_terms=16)
    assert host.chips[CPU]["relations"] > 64 and host.chips[CPU]["some"] > 0  # more relations than a wave has lanes: the lane-strided loops over them wrap
    got, st = emulated(emu, 0, head, prep, interpret, chips=[CPU], max_terms=16)
    assert np.array_equal(got, host.words)


def test_the_79_column_chip_under_emulation(machines, emu):
    """64 rows of alu(50)'s bitwise trace (79 columns: the pivots are compacted from two lane words of augmented columns), 7 rows per slice, a
    prefix sweep of 16 rows, entry groups of 33 relations and 300 words."""
    mt, prep = witness("alu50")
    mt = [np.ascontiguousarray(m[128:192]) if c == BITWISE else m for c, m in enumerate(mt)]  # 64 rows, operations and padding: the emulated ballots are slow
    host = va.product_audit_host(machines["basic"], mt, prep, chips=[BITWISE], max_terms=32, max_rows_per_entry=120)
    assert host.chips[BITWISE]["relations"] > 64  # more relations than a wave has lanes, several entry groups
    got, st = emulated(emu, 0, mt, prep, 0, rows_per_wave=5, rows_per_slice=7, prefix_rows=16, group_entries=33, group_words=300, chips=[BITWISE], max_terms=32, max_rows_per_entry=120)
    assert np.array_equal(got, host.words) and st["groups"] > 1 and st["slices"] == 10, st


@pytest.mark.parametrize("n,width", [(1, 7), (2, 7), (8, 7), (128, 63), (128, 64), (128, 65)])
def test_quad_airs_under_emulation(emu, n, width):
    machine, t = cases.quad_machine(width), cases.quad_trace(n, width)
    host = va.product_audit_host(machine, [t], [], max_rows_per_entry=8)
    got, st = emulated(emu, 1, [t], [], 1, rows_per_wave=3 if n > 2 else 0, rows_per_slice=16 if n > 8 else 0, prefix_rows=64 if n > 64 else 0, group_entries=2, max_rows_per_entry=8)
    assert np.array_equal(got, host.words)
    if n == 128:
        assert st["slices"] == 8 and st["groups"] == 5 and st["relations"] == 9, st


@pytest.mark.parametrize("kind", ["first", "last", "clean"])
def test_needle_traces_under_emulation(emu, kind):
    """The needle traces' first 512 rows with the break moved to row 511 (the emulated ballots are slow), 16 rows per slice: 32 slices for the
    row merge (two levels of its tree), the columns of the staircase that have begun each with a basis row in another slice, and a prefix sweep
    of 64 rows that the broken product survives."""
    t = np.ascontiguousarray(cases.needle("clean")[:512])
    if kind != "clean":
        row = 0 if kind == "first" else 511
        t[row, 7] = (int(t[row, 7]) + 1) % P
    host = va.product_audit_host(cases.free_machine(cases.NEEDLE_W), [t], [])
    # columns 8 + 6 .. 39 begin at row 600 or later: constant zero here, no pivots
    assert host.chips[0]["rank"] == 1 + 8 + 6 and ((0, 6) in host.relations(0)) == (kind == "clean")
    got, st = emulated(emu, 2, [t], [], 1, rows_per_slice=16, prefix_rows=64, group_entries=3)
    assert np.array_equal(got, host.words) and st["slices"] == 32, st
    if kind == "last":
        assert st["survivors"] > st["relations"], st  # (0, 6) holds on the prefix's rows: it dies in the second launch only


# ---- 9. C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_product_audit", "vgpu_product_audit_host", "vgpu_product_report_len", "vgpu_product_report_words", "vgpu_product_report_timing", "vgpu_product_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Product audit" in header and "vgpu_product_audit_opts_t" in header and ctypes.sizeof(va.ProductAuditOpts) == 32


# ---- 10. the host audit under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path, machines):
    """tests/emu/product_audit_host.cpp: fib(25) on the host VM and the host product audit, built with AddressSanitizer and UBSan and run as a
    subprocess (nothing sanitized is loaded into this interpreter).  Its figures are the library's for the same limits."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "product_audit_host")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "emu", "product_audit_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe, "25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    mt, prep = witness("fib25")
    rep = va.product_audit_host(machines["basic"], mt, prep, max_entries=1 << 20, max_rows_per_entry=64, max_terms=16)
    assert ("fib(25): %d words, %d relations of %d pairs, %d enforced on every row, %d on none, %d flat rows" % (
        len(rep.words), rep.total_entries, sum(c["pairs"] for c in rep.chips), sum(c["every"] for c in rep.chips), sum(c["never"] for c in rep.chips),
        sum(e["flat_rows"] for e in rep.entries))) in r.stdout, r.stdout
