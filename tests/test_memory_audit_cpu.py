"""The memory audit without a GPU: the host audit (vgpu_memory_audit_host) against the numpy reference (tests/memory_audit_ref.py) word for word
on every VM witness under both machine kinds, with the pinned counters; fib(25)'s mem trace tampered three ways; the edge traces on the captured
`ram` machine; a stale read planted at the order positions where its last write lies in another wave, workgroup, scan block and sort block; a
run of 3000 reads; a row permutation; same-cycle order; statics; the extreme keys and values; the limits; the refusals; determinism, signatures,
the JSON round trip; `check --memory --host`; the host audit under AddressSanitizer and UBSan as a stand-alone program; the device kernels' very
source under tools/hipemu.  The reference of each input is computed once per module."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import memory_audit_cases as cases
import memory_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
MEM = cases.MEM
_reference = {}


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


@pytest.fixture(scope="module")
def ram():
    return cases.ram_machine()


def reference(machines, name):
    if name not in _reference:
        _reference[name] = ref.audit(machines["basic"], *cases.witness(name))
    return _reference[name]


def on_ram(ram, t, **kw):
    """The host's report of a `ram` trace, held to the reference's."""
    want = ref.audit(ram, [t], [], **kw)
    rep = va.memory_audit_host(ram, [t], [], **kw)
    assert np.array_equal(rep.words, ref.words(want)), (rep.counters, want["counters"])
    return rep


def found(rep):
    return [(f["kind"], f["row"]) for f in rep.findings]


# ---- 1. the VM's witnesses: host = reference, clean, the pinned counters ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.VM))
def test_host_equals_reference_and_a_truthful_witness_is_clean(machines, name):
    want = reference(machines, name)
    for m in machines.values():
        rep = va.memory_audit_host(m, *cases.witness(name))
        assert np.array_equal(rep.words, ref.words(want))
    assert rep.total_findings == 0 and rep.findings == [] and not rep.truncated and rep.bus == (True, 2) and rep.receives == [(MEM, 0)]
    c = rep.counters
    assert c["live"] == c["reads"] + c["writes"] and c["slots"] == cases.witness(name)[0][MEM].shape[0] and rep.evaluations == c["slots"] and rep.device_ms == 0


def test_pinned_counters(machines):
    def counters(name):
        return va.memory_audit_host(machines["basic"], *cases.witness(name)).counters

    c = counters("fib25")
    assert (c["live"], c["reads"], c["addresses"], c["same_cycle_pairs"], c["max_clk_gap"]) == (401, 288, 13, 25, 185)
    c = counters("fib582")
    assert (c["live"], c["same_cycle_pairs"]) == (8756, 582)
    c = counters("static_data")
    assert (c["statics"], c["layout_descents"], c["dummy_reads_addr"], c["dummy_reads_clk"]) == (2, 1, 581, 0)
    assert va.memory_audit_host(machines["basic"], *cases.witness("static_data")).first_descent == (MEM, 1)  # the static prefix ends at row 1
    c = counters("store_byte")
    assert (c["uninit_zero_reads"], c["findings"]) == (1, 0)  # the read_or_init of STOREU8


# ---- 2. tampering with fib(25)'s mem trace ----------------------------------------------------------------------------------------------------------
def test_a_tampered_read_is_one_stale_read_at_that_row(machines):
    mt, prep, row = cases.tampered("read")
    want = ref.audit(machines["basic"], mt, prep)
    for m in machines.values():
        rep = va.memory_audit_host(m, mt, prep)
        assert np.array_equal(rep.words, ref.words(want))
    assert found(rep) == [("stale_read", row)] and rep.counters["stale_read"] == rep.total_findings == 1
    f = rep.findings[0]
    assert f["chip"] == MEM and f["value"] != f["expected"] and f["last_write"] is not None and f["last_write"][0] == MEM


def test_a_tampered_write_is_one_finding_per_read_up_to_the_next_write(machines):
    mt, prep, row = cases.tampered("write")
    want = ref.audit(machines["basic"], mt, prep)
    rep = va.memory_audit_host(machines["basic"], mt, prep)
    assert np.array_equal(rep.words, ref.words(want))
    assert rep.total_findings == want["counters"]["findings"] >= 1 and all(f["kind"] == "stale_read" and f["last_write"] == (MEM, 0, row) and f["row"] != row for f in rep.findings)


def test_a_read_of_an_unwritten_address(machines):
    mt, prep, row = cases.tampered("uninit")
    rep = va.memory_audit_host(machines["basic"], mt, prep)
    assert np.array_equal(rep.words, ref.words(ref.audit(machines["basic"], mt, prep)))
    assert found(rep) == [("uninit_read", row)] and rep.findings[0]["last_write"] is None and rep.findings[0]["expected"] == [0, 0, 0, 0] and rep.findings[0]["addr"] == 40000


# ---- 3. the `ram` machine ------------------------------------------------------------------------------------------------------------------------------
def test_edge_traces(ram):
    for name, t in cases.edge_traces():
        rep = on_ram(ram, t)
        n = t.shape[0]
        if name.endswith("all_dead"):
            assert rep.counters["live"] == 0 and rep.counters["slots"] == n and rep.total_findings == 0
        if name.endswith("one_write") or name.endswith("one_read_of_0"):
            assert rep.counters["live"] == 1 and rep.total_findings == 0 and rep.counters["uninit_zero_reads"] == int(name.endswith("0"))
        if name.endswith("one_read_of_7"):
            assert found(rep) == [("uninit_read", 0)]
        if name.endswith("alternating"):
            assert rep.counters["live"] == n and rep.counters["addresses"] == 1 and rep.total_findings == 0 and rep.counters["layout_descents"] == 0
        if name.endswith("own_address"):
            assert rep.counters["addresses"] == n and rep.counters["stale_read"] == 0 and rep.counters["uninit_read"] == len([k for k in range(n) if k % 3 and k % 2])


@pytest.mark.parametrize("position", cases.PLANT_POSITIONS)
def test_a_planted_stale_read(ram, position):
    rep = on_ram(ram, cases.planted(position))
    assert [(f["kind"], f["row"], f["position"]) for f in rep.findings] == [("stale_read", position, position)] and rep.total_findings == 1
    assert rep.findings[0]["last_write"] == (0, 0, 7 * (position // 7) if position % 7 else position - 7)


def test_a_run_of_3000_reads_and_a_row_permutation(ram):
    t, row = cases.long_run()
    rep = on_ram(ram, t)
    assert found(rep) == [("stale_read", row)] and rep.findings[0]["last_write"] == (0, 0, 2) and rep.findings[0]["expected"] == [0, 0, 0, 200]
    shuffled, perm = cases.permuted(t)
    other = on_ram(ram, shuffled)
    where = {int(p): i for i, p in enumerate(perm)}
    assert found(other) == [("stale_read", where[row])] and other.findings[0]["last_write"] == (0, 0, where[2])
    layout = ("layout_descents",)
    assert {k: v for k, v in other.counters.items() if k not in layout} == {k: v for k, v in rep.counters.items() if k not in layout}
    assert rep.counters["layout_descents"] == 0 and other.counters["layout_descents"] > 1 and other.first_descent is not None


def test_same_cycle_order_is_the_traces(ram):
    clean, stale = on_ram(ram, cases.same_cycle(read_first=False)), on_ram(ram, cases.same_cycle(read_first=True))
    assert clean.total_findings == 0 and found(stale) == [("stale_read", 2)] and stale.findings[0]["expected"] == [0, 0, 0, 5]
    assert clean.counters["same_cycle_pairs"] == stale.counters["same_cycle_pairs"] == 1


def test_two_receives_of_one_row(ram):
    m2 = cases.ram2_machine()
    t = cases.two_receive_trace()
    want = ref.audit(m2, [t], [])
    rep = va.memory_audit_host(m2, [t], [])
    assert np.array_equal(rep.words, ref.words(want)) and rep.receives == [(0, 0), (0, 1)] and rep.counters["slots"] == 128
    assert sorted((f["row"], f["kind"], f["interaction"]) for f in rep.findings) == [(r, "stale_read" if r else "uninit_read", 0) for r in range(0, 64, 8)]  # row 0 is the first record of its address


def test_statics(ram):
    reps = {name: on_ram(ram, t) for name, t in cases.static_traces()}
    assert reps["before_reads"].total_findings == 0 and reps["before_reads"].counters["statics"] == 2
    assert found(reps["duplicate"]) == [("duplicate_static", 1)]
    assert [(f["kind"], f["reason"]) for f in reps["clk_not_0"].findings] == [("malformed", 8)]
    r = reps["beside_an_operation_at_clk_0"]  # the static record comes first whatever its row: the write at clk 0 overwrites it
    assert r.total_findings == 0 and r.counters["same_cycle_pairs"] == 1
    assert [(f["kind"], f["reason"]) for f in reps["static_read"].findings] == [("malformed", 8)]


def test_extreme_keys_and_values(ram):
    reps = {name: on_ram(ram, t) for name, t in cases.extreme_traces()}
    r = reps["addr_clk_0_and_p_minus_1"]
    assert (r.counters["min_addr"], r.counters["max_addr"], r.counters["max_clk"], r.counters["max_clk_gap"]) == (0, P - 1, P - 1, P - 1) and found(r) == [("stale_read", 4)]
    assert r.counters["dummy_reads_clk"] == 2 * ((P - 1) // 5) and r.counters["dummy_reads_addr"] == (P - 1) // 5
    assert reps["top_byte_of_addr_varies"].total_findings == 0 and reps["top_byte_of_addr_varies"].counters["addresses"] == 4
    assert reps["no_byte_varies"].total_findings == 0 and reps["no_byte_varies"].counters["same_cycle_pairs"] == 63
    assert reps["no_byte_varies_all_live_reads"].counters["uninit_zero_reads"] == 64
    assert [(f["kind"], f["reason"]) for f in reps["values_256_and_p_minus_1"].findings] == [("malformed", 16)] * 4
    assert [(f["reason"], f["row"]) for f in reps["count_2_and_is_read_2"].findings] == [(1, 0), (2, 1), (4, 3)]  # is_read = 2 acts as a write: the reads after it are clean
    r = reps["clk_gap_and_addr_gap_above_L"]
    assert (r.counters["dummy_reads_clk"], r.counters["dummy_reads_addr"], r.total_findings) == (99 // 5, 996 // 5, 0)


def test_max_findings(ram):
    t = cases.many_findings()
    full = on_ram(ram, t, max_findings=1 << 20)
    assert full.total_findings == len(full.findings) == 300 and not full.truncated and [f["row"] for f in full.findings] == list(range(300))
    for k in (0, 1, 64):
        rep = on_ram(ram, t, max_findings=k)
        assert rep.total_findings == 300 and rep.findings == full.findings[:k] and rep.truncated and rep.counters == full.counters


def test_another_bus(ram):
    other = cases.ram_machine(bus=5)
    t = cases.same_cycle(read_first=True)
    rep = va.memory_audit_host(other, [t], [], bus=5)
    assert np.array_equal(rep.words, ref.words(ref.audit(other, [t], [], bus=(True, 5)))) and rep.bus == (True, 5) and rep.total_findings == 1


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(machines, ram):
    t = cases.same_cycle(True)
    for machine, kw, match in ((cases.ram_machine(fields=7), {}, "receives 7 fields on global bus 2; a memory record has exactly 8"),
                               (cases.no_receive_machine(), {}, "no chip receives on global bus 2"), (ram, dict(bus=3), "no chip receives on global bus 3"),
                               (ram, dict(bus=(False, 2)), "no chip receives on local bus 2"), (ram, dict(max_findings=(1 << 20) + 1), "max_findings is at most 2\\^20")):
        with pytest.raises(va.VgpuError, match="memory_audit: .*" + match) as e:
            va.memory_audit_host(machine, [t], [], **kw)
        assert e.value.code == -1
    mt, prep = cases.witness("fib25")
    for match, args in (("one main trace per chip", (mt[:-1], prep)), ("needs its preprocessed trace", (mt, prep[:1]))):
        with pytest.raises(va.VgpuError, match="memory_audit: .*" + match):
            va.memory_audit_host(machines["basic"], *args)
    with pytest.raises(va.VgpuError, match="memory_audit: traces are two-dimensional matrices"):
        va.memory_audit_host(ram, [np.zeros(4, dtype=np.uint32)], [])


def test_null_options_and_reserved(ram):
    t = np.ascontiguousarray(cases.planted(65, n=128))
    L = va.lib()

    def call(opts):
        h = ctypes.c_void_p()
        rc = L.vgpu_memory_audit_host(ram._h, (ctypes.c_void_p * 1)(t.ctypes.data), (ctypes.c_uint64 * 1)(t.shape[0]), (ctypes.c_uint64 * 1)(t.shape[1]), ctypes.c_uint32(1),
                                      (ctypes.c_uint32 * 1)(0), (ctypes.c_void_p * 1)(None), (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(0), ctypes.c_uint32(0),
                                      ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
        return rc, (va._audit_report("memory", va.MemoryReport, h) if rc == 0 else None)

    want = va.memory_audit_host(ram, [t], [])
    rc, rep = call(None)  # NULL options: 64 findings, global bus 2
    assert rc == 0 and np.array_equal(rep.words, want.words) and rep.max_findings == 64
    rc, rep = call(va.MemoryAuditOpts(0, 1, 2, 0))  # a struct is taken as given: 0 lists nothing
    assert rc == 0 and rep.findings == [] and rep.total_findings == 1 and rep.counters == want.counters
    assert call(va.MemoryAuditOpts(64, 1, 2, 1))[0] == -1 and call(va.MemoryAuditOpts(64, 2, 2, 0))[0] == -1
    M = ctypes.CDLL(va.lib()._name)
    length, words_of, timing, free = (getattr(M, "vgpu_memory_report_%s" % x) for x in ("len", "words", "timing", "free"))
    length.restype, words_of.restype, timing.restype, free.restype = ctypes.c_uint64, ctypes.c_void_p, None, None
    assert length(None) == 0 and words_of(None) is None
    tm = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    timing(None, tm)
    assert list(tm) == [0.0, 0.0, 0.0]
    free(None)


# ---- 5. determinism, signatures, JSON -----------------------------------------------------------------------------------------------------------------
def test_determinism(machines):
    mt, prep, _ = cases.tampered("write")
    assert np.array_equal(va.memory_audit_host(machines["basic"], mt, prep).words, va.memory_audit_host(machines["basic"], mt, prep).words)


def test_signatures():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_findings", 64, kind), ("bus", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.memory_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.memory_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert ctypes.sizeof(va.MemoryAuditOpts) == 16 and [f[0] for f in va.MemoryAuditOpts._fields_] == ["max_findings", "bus_is_global", "bus_index", "reserved"]


def test_json_round_trip(machines):
    mt, prep, _ = cases.tampered("write")
    rep = va.memory_audit_host(machines["basic"], mt, prep)
    d = json.loads(rep.to_json())
    assert d == json.loads(json.dumps(rep.to_dict())) and set(d) == {"words", "bus", "max_findings", "truncated", "receives", "counters", "first_descent", "findings", "device_ms",
                                                                      "host_ms", "evaluations"}
    again = va.MemoryReport.from_dict(d)
    assert again.to_dict() == rep.to_dict() and np.array_equal(again.words, rep.words) and again.findings == rep.findings
    with pytest.raises(ValueError):
        va.MemoryReport(rep.words[:-1])


# ---- 6. command line --------------------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_memory_on_the_host(tmp_path, machines):
    sb, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    sb.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", sb, out_plain, "--host")
    r = _cli("check", sb, out, "--host", "--memory")
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before and len(lines) == len(before) + 1  # a clean witness: nothing but the summary
    assert lines[-1].startswith("mem: 34 live records (20 reads, 14 writes, 0 static) of 11 addresses") and "laid out sorted" in lines[-1] and "no finding" in lines[-1]
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    assert set(j) == set(plain_json) | {"memory"} and "mem: " not in plain.stdout
    rep = va.memory_audit_host(machines["basic"], *cases.witness("byte_loads"))
    assert va.MemoryReport.from_dict(j["memory"]).counters == rep.counters
    help_text = _cli("--help").stdout
    assert "--memory" in help_text and "--max-findings" in help_text


def test_cli_lines_and_exit_status_of_a_tampered_witness(machines):
    """`check` audits the witness the VM generates, which is truthful: the tampered lines and the exit status are those of the functions it calls."""
    from valida_amd import cli

    mt, prep, row = cases.tampered("read")
    rep = va.memory_audit_host(machines["basic"], mt, prep)
    lines = cli.memory_lines(rep)
    f = rep.findings[0]
    assert lines[0] == "mem: 1 stale read (row %d, addr %d, clk %d: read %d, last write %d at row %d)" % (row, f["addr"], f["clk"], cli.memory_value(f["value"]), cli.memory_value(f["expected"]),
                                                                                                          f["last_write"][2])
    assert len(lines) == 2 and lines[1].startswith("mem: 401 live records") and lines[1].endswith("1 finding")
    assert cli.check_status(True, None, rep) == 1 and cli.check_status(True, None, None) == 0
    clean = va.memory_audit_host(machines["basic"], *cases.witness("fib25"))
    assert cli.check_status(True, None, clean) == 0 and len(cli.memory_lines(clean)) == 1
    mt, prep, row = cases.tampered("uninit")
    lines = cli.memory_lines(va.memory_audit_host(machines["basic"], mt, prep))
    assert lines[0] == "mem: 1 uninitialised read (row %d, addr 40000, clk %d: read %d, nothing written)" % (row, f["clk"], cli.memory_value([0, 0, 10, 9]))


# ---- 7. the host audit under AddressSanitizer and UBSan, as a stand-alone program ----------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "emu", "memory_audit_host.cpp")
    exe = str(tmp_path / "memory_audit_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("memory_audit_host: fib(25): 401 live, 0 findings") and "tampered: 1 finding" in r.stdout


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "memory_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libmemoryauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "host", "memory_audit.hpp"), os.path.join(csrc, "host", "bus_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("memory_audit.hip", "bus_records.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_memory_audit.restype = ctypes.c_int64
    return L


def emulated(emu, machine_kind, mt, prep, max_findings=64):
    """The report image of the emulated device pass (machine_kind 0: BasicMachine, 1: ram, 2: ram2)."""
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    n, k = len(mains), len(preps)
    u, cap = ctypes.c_uint32, 1 << 20
    out = np.zeros(cap, dtype=np.uint32)
    got = emu.emu_memory_audit(u(machine_kind), (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                               (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), u(n), (ctypes.c_uint32 * max(1, k))(*[c for c, _ in preps]),
                               (ctypes.c_void_p * max(1, k))(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * max(1, k))(*[m.shape[0] for _, m in preps]),
                               (ctypes.c_uint64 * max(1, k))(*[m.shape[1] for _, m in preps]), u(k), u(max_findings), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(cap))
    assert got > 0, got
    return out[:got]


def test_emulated_kernels_on_fib25_and_the_tampered_traces(emu, machines):
    for mt, prep in [cases.witness("fib25"), cases.witness("static_data"), cases.witness("store_byte")] + [cases.tampered(k)[:2] for k in ("read", "write", "uninit")]:
        assert np.array_equal(emulated(emu, 0, mt, prep), va.memory_audit_host(machines["basic"], mt, prep).words)


def test_emulated_kernels_on_the_edge_traces(emu, ram):
    named = cases.edge_traces() + cases.static_traces() + cases.extreme_traces() + [("same_cycle_%d" % k, cases.same_cycle(bool(k))) for k in (0, 1)] + [("long_run", cases.long_run()[0])]
    named += [("permuted", cases.permuted(cases.long_run()[0])[0])] + [("planted_%d" % k, cases.planted(k)) for k in (255, 2047, 2048, 4096)]
    for name, t in named:
        assert np.array_equal(emulated(emu, 1, [t], []), va.memory_audit_host(ram, [t], []).words), name
    t = cases.many_findings()
    for k in (0, 1, 300):
        assert np.array_equal(emulated(emu, 1, [t], [], max_findings=k), va.memory_audit_host(ram, [t], [], max_findings=k).words), k
    t = cases.two_receive_trace()
    assert np.array_equal(emulated(emu, 2, [t], []), va.memory_audit_host(cases.ram2_machine(), [t], []).words)
