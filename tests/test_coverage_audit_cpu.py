"""The coverage audit without a GPU: the host implementation of the contract (vgpu_coverage_audit_host) against the brute-force restatement of
tests/coverage_audit_ref.py (the oracle's own chip transcription, mutation by mutation) on whole witnesses, word for word, for both machine
kinds; the pinned figures of a prototype over the oracle's transcription; invariants against the mutation audit; delta sets; the max_cells cut;
argument validation; merge; the device kernels' very source under tools/hipemu; `check --coverage` and coverage_merge on the command line.
The reference of each input is computed once per module and cut to the limit a test asks for (the counts do not depend on it)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coverage_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
NO_ROW = 0xFFFFFFFF


def exe(prog, advice=b""):
    return va.Workload.from_executable(vp.machine_code(prog), advice=advice)


INPUTS = {
    "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "static_data": lambda: va.Workload.named("static_data"),
    "byte_loop50": lambda: exe(vp.byte_loop_program(50), bytes(range(30))),
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


def reference(machines, name, deltas=(1, P - 1), max_cells=8192):
    """The reference's report of a named input, computed once per (input, deltas) with every cell listed, cut to max_cells."""
    key = (name, tuple(deltas))
    if key not in _reference:
        mt, prep = witness(name)
        _reference[key] = ref.audit(machines["basic"], mt, prep, deltas=deltas, max_cells=1 << 30)
    return ref.recut(_reference[key], max_cells)


def both(machines, name, deltas=(1, P - 1), max_cells=8192):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, deltas, max_cells)
    mt, prep = witness(name)
    reps = {k: va.coverage_audit_host(m, mt, prep, deltas=deltas, max_cells=max_cells) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    assert np.array_equal(reps["basic"].words, reps["ffi"].words)
    return want, reps["basic"]


def sums(c):
    return sum(map(sum, c["kills"])), sum(map(sum, c["sole"]))


# ---- 1. the host audit equals the reference; the prototype's figures -----------------------------------------------------------------------------
def test_fib25_is_the_prototypes_table(machines):
    want, rep = both(machines, "fib25")
    assert rep.deltas == [1, P - 1] and not rep.truncated and rep.total_cells == rep.reported == 1070
    cpu = want["chips"][CPU]
    assert (cpu["constraints"], cpu["interactions"], cpu["height"]) == (53, 4, 256) and sums(cpu) == (47174, 6483)
    assert sum(1 for e in want["cells"] if e["chip"] == CPU) == 396 and ref.classes(want, CPU)[:2] == ([], [])
    assert cpu["free"] == [3131, 3047]
    assert sums(want["chips"][ADD]) == (12448, 138) and sums(want["chips"][MUL]) == (24578, 16382)
    dead = {chip: ref.classes(want, chip)[0] for chip in range(14) if ref.classes(want, chip)[0]}
    assert dead == {LT: [21, 29, 30, 32, 34], BITWISE: [2, 3, 4, 23, 24, 25, 44, 45, 46, 65, 66, 67], OUTPUT: [0, 1], STATIC_DATA: [0]}
    # 26 of cpu's 53 constraints are never the sole detector of a mutation
    assert len(ref.classes(want, CPU)[2]) == 26
    for chip in range(14):
        dc, di, sc, si = ref.classes(want, chip)
        assert rep.dead(chip) == (dc, di) and rep.shadowed(chip) == (sc, si)
        c = rep.chips[chip]
        assert (c["dead_constraints"], c["dead_interactions"], c["shadowed_constraints"], c["shadowed_interactions"]) == (len(dc), len(di), len(sc), len(si))


def test_alu50_and_the_merged_corpus(machines):
    want, rep = both(machines, "alu50")
    assert sums(want["chips"][CPU]) == (104548, 11087) and want["chips"][CPU]["height"] == 512
    assert ref.classes(want, LT)[0] == [] and ref.classes(want, BITWISE)[0] == [] and ref.classes(want, CPU)[:2] == ([], [])
    assert len(ref.classes(want, CPU)[2]) == 28
    assert {chip: rep.dead(chip)[0] for chip in range(14) if rep.dead(chip)[0]} == {OUTPUT: [0, 1], STATIC_DATA: [0]}
    fib_want, fib = both(machines, "fib25")
    merged = va.CoverageReport.merge([fib, rep])
    assert {chip: merged.dead(chip)[0] for chip in range(14) if merged.dead(chip)[0]} == {OUTPUT: [0, 1], STATIC_DATA: [0]}
    for chip in range(14):
        a, b, m = fib.chips[chip], rep.chips[chip], merged.chips[chip]
        assert m["height"] == a["height"] + b["height"] and (m["width"], m["constraints"], m["interactions"]) == (a["width"], a["constraints"], a["interactions"])
        assert m["detected"] == [x + y for x, y in zip(a["detected"], b["detected"])] and m["free"] == [x + y for x, y in zip(a["free"], b["free"])]
        assert m["kills"] == [[x + y for x, y in zip(ka, kb)] for ka, kb in zip(a["kills"], b["kills"])]
        assert m["sole"] == [[x + y for x, y in zip(ka, kb)] for ka, kb in zip(a["sole"], b["sole"])]
    cells = {}
    for e in fib.cells + rep.cells:
        key = (e["chip"], e["detector"], e["column"], e["delta"])
        cells[key] = tuple(x + y for x, y in zip(cells.get(key, (0, 0)), (e["kills"], e["sole"])))
    assert [((e["chip"], e["detector"], e["column"], e["delta"]), (e["kills"], e["sole"])) for e in merged.cells] == sorted(cells.items())
    assert all(e["first_row"] == NO_ROW and e["first_sole_row"] == NO_ROW for e in merged.cells) and merged.total_cells == len(cells) and not merged.truncated
    assert np.array_equal(va.CoverageReport.merge([merged]).words, merged.words)
    with pytest.raises(ValueError, match="different deltas"):
        va.CoverageReport.merge([fib, va.coverage_audit_host(machines["basic"], *witness("static_data"), deltas=(2,))])
    with pytest.raises(ValueError, match="cut"):
        va.CoverageReport.merge([fib, va.coverage_audit_host(machines["basic"], *witness("static_data"), max_cells=5)])
    other = va.CoverageReport.from_dict(dict(fib.to_dict(), chips=fib.chips[:-1], cells=[e for e in fib.cells if e["chip"] < 13]))
    with pytest.raises(ValueError, match="different machines"):
        va.CoverageReport.merge([fib, other])


@pytest.mark.parametrize("name", ["static_data", "byte_loop50"])
def test_clean_witnesses(machines, name):
    want, rep = both(machines, name)
    assert not rep.truncated and rep.total_cells == rep.reported > 0


def test_failing_witness_counts_newly_failing_constraints(machines):
    """mixed_ops:40 fails constraints already: a constraint that failed at a row before the mutation kills nothing there."""
    mt, prep = witness("mixed_ops:40")
    assert not va.constraint_audit_host(machines["basic"], mt, prep).satisfied
    both(machines, "mixed_ops:40")


# ---- 2. invariants ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib25", "mixed_ops:40"])
def test_invariants_against_the_mutation_audit(machines, name):
    mt, prep = witness(name)
    m = machines["basic"]
    rep = va.coverage_audit_host(m, mt, prep, max_cells=1 << 20)
    mu = va.mutation_audit_host(m, mt, prep, max_entries=1 << 20)
    assert not rep.truncated and not mu.truncated
    for chip in range(14):
        c = rep.chips[chip]
        n, w = c["height"], c["width"]
        assert c["free"] == mu.chips[chip]["free"] and [d + f for d, f in zip(c["detected"], c["free"])] == [n * w] * 2
        mine = [e for e in rep.cells if e["chip"] == chip]
        assert set(range(w)) - set(e["column"] for e in mine) == set(mu.unbound_columns(chip))  # unbound there iff no cell here
        free = {(e["column"], e["delta"]): e["free"] for e in mu.entries if e["chip"] == chip}
        for col in range(w):
            for j in range(2):
                detected = n - free.get((col, j), 0)
                assert sum(e["sole"] for e in mine if (e["column"], e["delta"]) == (col, j)) <= detected <= sum(e["kills"] for e in mine if (e["column"], e["delta"]) == (col, j))
        for e in mine:
            assert 0 < e["kills"] <= n and e["sole"] <= e["kills"] and e["first_row"] < n
            assert (e["first_sole_row"] == NO_ROW) == (e["sole"] == 0) and e["first_sole_row"] >= e["first_row"]
            if c["constraints"] == 0 and c["interactions"] == 1:
                assert e["kills"] == e["sole"]  # a bus-only chip of one interaction: that interaction is always alone
        assert [sum(e["kills"] for e in mine if e["detector"] == t and e["delta"] == j) for t in range(len(c["kills"])) for j in range(2)] == [k for ks in c["kills"] for k in ks]
    assert any(c["constraints"] == 0 and c["interactions"] == 1 and any(c["detected"]) for c in rep.chips)


# ---- 3. reports and arguments ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deltas", [(1,), (1, P - 1), (2, 1, P - 1, 12345)], ids=["+1", "+1,-1", "four"])
def test_delta_sets(machines, deltas):
    want, rep = both(machines, "static_data", deltas)
    assert rep.deltas == list(deltas) and all(len(c["free"]) == len(deltas) and all(len(k) == len(deltas) for k in c["kills"]) for c in rep.chips)
    pair = reference(machines, "static_data")
    at = list(deltas).index(1)
    assert [c["free"][at] for c in rep.chips] == [c["free"][0] for c in pair["chips"]]
    assert [[k[at] for k in c["kills"]] for c in rep.chips] == [[k[0] for k in c["kills"]] for c in pair["chips"]]


def test_max_cells_cut(machines):
    full_want, full = both(machines, "fib25")
    want, rep = both(machines, "fib25", max_cells=400)  # the cut falls inside the second chip's cells
    assert rep.truncated and rep.reported == 400 and rep.total_cells == full.total_cells == 1070 and rep.chips == full.chips and rep.cells == full.cells[:400]
    want, rep = both(machines, "fib25", max_cells=3)
    assert rep.truncated and rep.reported == 3 and rep.chips == full.chips and rep.dead(LT) == full.dead(LT)


def test_argument_validation(machines):
    m = machines["basic"]
    mt, prep = witness("static_data")

    def refused(match, main=mt, pre=prep, **kw):
        with pytest.raises(va.VgpuError, match=match) as e:
            va.coverage_audit_host(m, main, pre, **kw)
        assert e.value.code == -1  # VGPU_ERR_INVALID_ARG

    refused("coverage_audit: need one main trace per chip", main=mt[:-1])
    refused("width mismatch for chip add", main=mt[:ADD] + [mt[ADD][:, :-1]] + mt[ADD + 1:])
    refused("powers of two", main=mt[:MUL] + [mt[MUL][:-1]] + mt[MUL + 1:])
    refused("needs its preprocessed trace", pre=prep[:1])
    refused("max_cells", max_cells=0)  # an explicit zero passed through Python
    refused("1 to 4 deltas", deltas=())
    refused("1 to 4 deltas", deltas=(1, 2, 3, 4, 5))
    refused("a delta must be a canonical value in 1..p-1", deltas=(1, 0))
    refused("a delta must be a canonical value in 1..p-1", deltas=(P,))
    refused("the deltas must be distinct", deltas=(5, 7, 5))
    # the C entry point itself: reserved != 0, too many deltas, a repeated delta and null arguments are refused with a code and a message; a
    # zeroed struct (or NULL) means the defaults
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[x.ctypes.data for x in mt])
    hs, ws = (ctypes.c_uint64 * 14)(*[x.shape[0] for x in mt]), (ctypes.c_uint64 * 14)(*[x.shape[1] for x in mt])
    pa = (ctypes.c_void_p * 2)(*[x.ctypes.data for _, x in prep])
    ph, pw = (ctypes.c_uint64 * 2)(*[x.shape[0] for _, x in prep]), (ctypes.c_uint64 * 2)(*[x.shape[1] for _, x in prep])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in prep])
    L = va.lib()

    def opts(max_cells=0, n=0, deltas=(0, 0, 0, 0), wgs=0, reserved=(0, 0)):
        return ctypes.byref(va.CoverageAuditOpts(max_cells, n, (ctypes.c_uint32 * 4)(*deltas), wgs, (ctypes.c_uint32 * 2)(*reserved)))

    assert ctypes.sizeof(va.CoverageAuditOpts) == 40
    assert L.vgpu_coverage_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(reserved=(0, 1)), ctypes.byref(h)) == -1 and b"reserved" in L.vgpu_last_error()
    assert L.vgpu_coverage_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(n=5), ctypes.byref(h)) == -1 and b"at most 4 deltas" in L.vgpu_last_error()
    assert L.vgpu_coverage_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(n=2, deltas=(3, 3, 0, 0)), ctypes.byref(h)) == -1 and b"distinct" in L.vgpu_last_error()
    assert L.vgpu_coverage_audit_host(m._h, None, hs, ws, 14, chips, pa, ph, pw, 2, None, ctypes.byref(h)) == -1 and b"null" in L.vgpu_last_error()
    assert L.vgpu_coverage_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, None, None) == -1 and b"null" in L.vgpu_last_error()
    L.vgpu_coverage_report_len.restype = ctypes.c_uint64
    L.vgpu_coverage_report_words.restype = ctypes.POINTER(ctypes.c_uint32)
    L.vgpu_coverage_report_len.argtypes = L.vgpu_coverage_report_words.argtypes = L.vgpu_coverage_report_free.argtypes = [ctypes.c_void_p]
    want = va.coverage_audit_host(m, mt, prep).words
    for o in (opts(), None, opts(wgs=7)):  # the host audit ignores max_workgroups
        assert L.vgpu_coverage_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, o, ctypes.byref(h)) == 0
        n = L.vgpu_coverage_report_len(h)
        assert np.array_equal(np.ctypeslib.as_array(L.vgpu_coverage_report_words(h), shape=(n,)), want)
        L.vgpu_coverage_report_free(h)


def test_report_image_and_json(machines):
    mt, prep = witness("static_data")
    rep = va.coverage_audit_host(machines["basic"], mt, prep)
    w = [int(x) for x in rep.words]
    assert w[0] == 0x31524B56 and bytes(rep.words[:1].tobytes()) == b"VKR1" and w[1] == len(w) and w[2:4] == [2, 0] and w[6:12] == [rep.reported, 14, 1, P - 1, 0, 0]
    assert w[4] | (w[5] << 32) == rep.total_cells == rep.reported
    assert len(w) == 12 + sum(10 + 8 + 8 * (c["constraints"] + c["interactions"]) for c in rep.chips) + 10 * rep.reported
    assert rep.device_ms == 0.0 and rep.host_ms > 0 and rep.evaluations > 0
    again = va.CoverageReport(rep.words)
    assert again.cells == rep.cells and again.chips == rep.chips and again.deltas == rep.deltas
    j = json.loads(rep.to_json())
    assert j["deltas"] == [1, P - 1] and j["total_cells"] == rep.total_cells and j["device_ms"] == 0.0 and j["cells"][0] == rep.cells[0] and j["chips"] == rep.chips
    back = va.CoverageReport.from_dict(j)
    assert np.array_equal(back.words, rep.words) and back.host_ms == rep.host_ms
    assert np.array_equal(va.coverage_audit_host(machines["basic"], mt, prep).words, rep.words)  # the same words run after run
    with pytest.raises(ValueError):
        va.CoverageReport(rep.words[:-1])


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "coverage_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libcoverageauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "coverage_audit.hpp"), os.path.join(csrc, "host", "mutation_audit.hpp"),
            os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("coverage_audit.hip", "mutation_audit.hip", "mutation_eval.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_coverage_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, block_threads=0, deltas=(1, P - 1), max_cells=8192, column_slices=0, max_workgroups=0, bus_walk=0):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(12 + 14 * (18 + 16 * 128) + 10 * min(max_cells, 1 << 16), np.uint32)
    got = emu.emu_coverage_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(block_threads), ctypes.c_uint32(column_slices), ctypes.c_uint32(max_workgroups), ctypes.c_uint32(bus_walk), (ctypes.c_uint32 * len(deltas))(*deltas),
        ctypes.c_uint32(len(deltas)), ctypes.c_uint32(max_cells), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
@pytest.mark.parametrize("name", ["fib25", "mixed_ops:40", "static_data"])
def test_kernel_source_under_emulation(machines, emu, name, interpret):
    """The audit pass and the pack of coverage_audit.hip with the evaluation code of mutation_eval.hpp, the compiled chip templates, the
    interpreted programs and the bus-only chips: the assembled report is the reference's, word for word.  In the device's launch shape fib25's
    mul (1024 rows) and mem (512) span several row tiles; with 64-row tiles its cpu trace (256 rows) does too, so the r - 1 halo and the wrap
    between row 0 and row n - 1 cross tiles; max_workgroups 1 and 3 make a workgroup keep its table over 4 (mul: 16 at 64 rows) tiles, unevenly
    for 3."""
    mt, prep = witness(name)
    assert np.array_equal(emulated(emu, mt, prep, interpret), ref.words(reference(machines, name)))
    if name == "fib25":
        assert mt[CPU].shape[0] == 256 and mt[MUL].shape[0] == 1024
        full = ref.words(reference(machines, name))
        for kw in (dict(block_threads=64), dict(max_workgroups=1), dict(max_workgroups=3), dict(block_threads=64, max_workgroups=3), dict(column_slices=1, block_threads=64),
                   dict(column_slices=3, block_threads=64, max_workgroups=5), dict(column_slices=1000), dict(bus_walk=1), dict(bus_walk=1, block_threads=64, max_workgroups=1)):
            assert np.array_equal(emulated(emu, mt, prep, interpret, **kw), full), kw
        for cut in (3, 400):
            assert np.array_equal(emulated(emu, mt, prep, interpret, max_cells=cut, max_workgroups=3), ref.words(reference(machines, name, max_cells=cut)))
    if name == "static_data":
        deltas = (2, 1, P - 1, 12345)
        assert np.array_equal(emulated(emu, mt, prep, interpret, deltas=deltas), ref.words(reference(machines, name, deltas)))


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _run(module, *args):
    return subprocess.run([sys.executable, "-m", module] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_coverage_on_the_host_and_merge(tmp_path, machines):
    from valida_amd import cli

    bl, out, out2, merged = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "report2.json", tmp_path / "merged.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _run("valida_amd.cli", "check", bl, out, "--host")
    assert plain.returncode == 0, plain.stderr
    plain_json = json.loads(out.read_text())
    r = _run("valida_amd.cli", "check", bl, out, "--host", "--coverage")
    assert r.returncode == 0, r.stderr  # a dead constraint is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = exe(vp.byte_loads_program())
    rep = va.coverage_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_cells=1 << 20)
    assert lines[len(before):] == cli.coverage_lines(rep)
    chips = [c["chip"] for c in rep.chips if any(rep.dead(c["chip"])) or any(rep.shadowed(c["chip"]))]
    assert [line.split(":")[0] for line in lines[len(before):]] == [va.CHIP_NAMES[c] for c in chips] and OUTPUT in chips
    assert any(line.startswith("output: dead constraints 0-1") for line in lines)
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"coverage"} and {k: v for k, v in j.items() if k not in ("coverage", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    cov = j["coverage"]
    assert cov["deltas"] == [1, P - 1] and cov["chips"] == rep.chips and cov["cells"] == rep.cells and not cov["truncated"]
    # with --mutations: both keys, the mutation lines first, one delta set for both
    r = _run("valida_amd.cli", "check", bl, out2, "--host", "--coverage", "--mutations", "--deltas=2")
    j2 = json.loads(out2.read_text())
    assert r.returncode == 0 and j2["coverage"]["deltas"] == [2] and j2["mutations"]["deltas"] == [2]
    assert [c["free"] for c in j2["coverage"]["chips"]] == [c["free"] for c in j2["mutations"]["chips"]]
    r = _run("valida_amd.cli", "check", bl, out2, "--host", "--coverage", "--deltas=1,1")
    assert r.returncode != 0 and "distinct" in r.stderr + r.stdout
    # the corpus: this report and fib25's
    fib = va.coverage_audit_host(machines["basic"], *witness("fib25"), max_cells=1 << 20)
    out2.write_text(json.dumps(dict(coverage=fib.to_dict())))
    r = _run("valida_amd.coverage_merge", merged, out, out2)
    assert r.returncode == 0, r.stderr
    want = va.CoverageReport.merge([rep, fib])
    got = va.CoverageReport.from_dict(json.loads(merged.read_text())["coverage"])
    assert np.array_equal(got.words, want.words) and r.stdout.strip().split("\n") == cli.coverage_lines(want)
    out2.write_text(json.dumps(dict(coverage=va.coverage_audit_host(machines["basic"], *witness("fib25"), deltas=(2,)).to_dict())))
    r = _run("valida_amd.coverage_merge", merged, out, out2)
    assert r.returncode != 0 and "different deltas" in r.stderr


def test_coverage_lines_notation():
    from valida_amd import cli

    assert cli.index_ranges([21, 29, 30, 32, 34]) == "21, 29-30, 32, 34" and cli.index_ranges([0, 1, 2]) == "0-2"
