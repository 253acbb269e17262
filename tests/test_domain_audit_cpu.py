"""The domain audit without a GPU: the host implementation of the contract (vgpu_domain_audit_host) against the numpy restatement of
tests/domain_audit_ref.py word for word, for both machine kinds, on fib(1), fib(25), alu(50), the captured needle machine and the edge traces;
the structure the reference finds (the lookup buses of the BasicMachine, add's guarded output bytes and unguarded input bytes on fib(25), the
range bus offering bytes); options and refusals; determinism; the API edges; `check --host --domains`; the host audit under AddressSanitizer and
UBSan as a stand-alone program; the device kernels' very source under tools/hipemu.  The reference of each input is computed once per module.
The figures pinned here are the reference's, not the code under test's: each is asserted on the reference's report as well.

Heights are powers of two by the machine's rule (a trace of 63 rows is refused by every audit and by prove), so the row counts 63 / 65 / 255 /
257 appear as the row at which a 512-row trace's patterns switch (tests/domain_audit_cases.py): one row before and behind a wave's and a tile's end."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import domain_audit_cases as cases
import domain_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, CPU, MEM, SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
RANGE = 12
ALL = dict(max_entries=1 << 20, max_rows_per_entry=4096)
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


def reference(machines, name):
    """The reference's report of a BasicMachine witness under the default options, once per module."""
    if name not in _reference:
        _reference[name] = ref.audit(machines["basic"], *witness(name))
    return _reference[name]


def both(machines, name):
    want = reference(machines, name)
    reps = {k: va.domain_audit_host(m, *witness(name)) for k, m in machines.items()}
    for rep in reps.values():
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


# ---- 1. the host audit equals the reference; the structure the reference finds -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib1", "fib25", "alu50"])
def test_host_equals_reference(machines, name):
    want, rep = both(machines, name)
    assert all(c["audited"] for c in rep.chips) and not rep.truncated and rep.total_entries == rep.reported == want["total_entries"] > 0
    for c in rep.chips:
        cols = rep.columns(c["chip"])
        assert len(cols) == c["width"] and c["narrow"] == sum(k["narrow"] for k in cols) and c["entries"] == len(rep.unguarded(c["chip"]))
        for k in cols:
            assert k["unguarded_rows"] == c["height"] - k["guarded_rows"] and k["unguarded_nonzero_rows"] <= k["nonzero_rows"] <= c["height"]
            assert k["dense"] == (k["wide_rows"] == 0 and k["distinct_narrow"] == k["max"] - k["min"] + 1) and k["bits"] == k["max"].bit_length()
            # every BOOLEAN and CONSTANT column is never an entry
            if k["cls"] in ("constant", "boolean", "wide"):
                assert not k["narrow"] and k["column"] not in rep.unguarded(c["chip"])


def test_lookup_buses_of_the_basic_machine(machines):
    """The structural rule on the transcribed chips gives the MEMORY bus (global 2) and the RANGE bus (global 3) and nothing else: the program
    chip has no interaction here (no chip sends to a program bus), the static-data chip SENDS its cells on the memory bus rather than owning a
    bus, and the memory chip's AIR has no constraint and no send, so that structurally it is a table like the range chip."""
    buses, table = ref.lookup_buses(machines["basic"])
    assert [(g, i) for g, i, lookup, _ in buses if lookup] == [(1, 2), (1, 3)]
    assert [c for c in range(va.NUM_CHIPS) if table[c]] == [MEM, 6, RANGE]  # mem, div (no constraints transcribed, one receive), range
    for m in machines.values():
        rep = va.domain_audit_host(m, *witness("fib1"))
        assert rep.lookup_buses() == [(True, 2), (True, 3)] and [b["bus_index"] for b in rep.buses] == [0, 2, 3] and rep.lookup_auto
        assert [c["chip"] for c in rep.chips if c["is_table"]] == [MEM, 6, RANGE]


def test_add_on_fib25(machines):
    """add sends its four output bytes to the range bus but not its eight input bytes (alu_u32/src/add/mod.rs:53-68): the outputs are guarded
    on exactly the rows add is real on, 105 (add's range sends), the inputs on none, and received on those same rows."""
    want, rep = both(machines, "fib25")
    for cols in (want["chips"][ADD]["cols"], [dict(k, guarded=k["guarded_rows"], received=k["received_rows"], ungnz=k["unguarded_nonzero_rows"], nonzero=k["nonzero_rows"],
                                                  cls=ref.CLASSES.index(k["cls"])) for k in rep.columns(ADD)]):
        assert [k["guarded"] for k in cols[11:15]] == [105] * 4 and [k["ungnz"] for k in cols[11:15]] == [0] * 4
        assert [k["guarded"] for k in cols[:8]] == [0] * 8 and [k["received"] for k in cols[:8]] == [105] * 8
        assert all(k["cls"] <= 2 and k["ungnz"] == k["nonzero"] for k in cols[:8])  # bytes; the high bytes of fib(25)'s operands are constant or boolean
    assert rep.unguarded(ADD) == [2, 3, 6, 7]  # the input bytes that are byte-valued on this witness
    e = [e for e in rep.entries if e["chip"] == ADD][0]
    assert [(a["is_send"], a["bus_index"], a["lookup"], a["live_rows"]) for a in e["appearances"]] == [(False, 0, False, 105)]
    assert len(e["rows"]) == 4 and all(v != 0 and v < 256 for _, v in e["rows"])


def test_range_bus_offers_bytes(machines):
    want, rep = both(machines, "fib25")
    for positions in ([p for p in want["positions"] if want["buses"][p["bus"]][:2] == (1, 3)], [dict(p, is_send=int(p["is_send"])) for p in rep.buses[2]["positions"]]):
        recv = [p for p in positions if not p["is_send"] and p["position"] == 0][0]
        send = [p for p in positions if p["is_send"] and p["position"] == 0][0]
        assert recv["max"] <= 255 and send["max"] <= 255 and recv["records"] > 0


# ---- 2. the needle ------------------------------------------------------------------------------------------------------------------------------
def test_needle():
    """The user chip is audited (chips=[0]): the table chip's own two columns are narrow and sent nowhere, as the range chip's are on the
    BasicMachine, and are entries of the whole machine's audit with or without the break."""
    machine = cases.needle_machine()
    clean = va.domain_audit_host(machine, cases.needle_traces(False), [], chips=[0])
    assert np.array_equal(clean.words, ref.words(ref.audit(machine, cases.needle_traces(False), [], chips=[0])))
    assert clean.lookup_buses() == [(True, cases.NEEDLE_BUS)] and clean.total_entries == 0 and clean.entries == [] and clean.columns(0)[0]["guarded_rows"] == 512
    broken = va.domain_audit_host(machine, cases.needle_traces(True), [], chips=[0])
    assert np.array_equal(broken.words, ref.words(ref.audit(machine, cases.needle_traces(True), [], chips=[0])))
    assert broken.total_entries == 1 and broken.unguarded(0) == [0]
    e = broken.entries[0]
    assert (e["chip"], e["column"], e["cls"], e["unguarded_nonzero_rows"], e["rows"]) == (0, 0, "byte", 1, [(511, 1 + 511 % 255)])
    assert broken.columns(0)[0]["guarded_rows"] == 511 and broken.chips[1]["is_table"] and not broken.chips[0]["is_table"]
    for broken in (False, True):
        whole = va.domain_audit_host(machine, cases.needle_traces(broken), [])
        assert np.array_equal(whole.words, ref.words(ref.audit(machine, cases.needle_traces(broken), [])))
        assert whole.unguarded(1) == [0, 1] and whole.unguarded(0) == ([0] if broken else [])


# ---- 3. edge shapes -------------------------------------------------------------------------------------------------------------------------------
def test_edge_shapes():
    machine = cases.edge_machine()
    for name, t in cases.edge_traces():
        rep = va.domain_audit_host(machine, [t], [], max_rows_per_entry=7)
        assert np.array_equal(rep.words, ref.words(ref.audit(machine, [t], [], max_rows_per_entry=7))), name
    by = dict(cases.edge_traces())
    col = lambda name: va.domain_audit_host(machine, [by[name]], []).columns(0)[0]  # noqa: E731
    assert (col("n64_0")["cls"], col("n64_0_1")["cls"], col("n64_255")["cls"], col("n64_31_32")["cls"], col("n64_65535")["cls"]) == ("constant", "boolean", "constant", "byte", "constant")
    assert col("n64_65536")["wide_rows"] == 64 and col("n64_65536")["distinct_narrow"] == 0 and col("n64_%d" % (P - 1))["max"] == P - 1
    assert col("n64_31_32")["distinct_narrow"] == 2 and col("n64_31_32")["dense"] and col("alternating")["cls"] == "half" and not col("alternating")["dense"]
    assert col("n64_31_32")["mixed_rows"] == col("n64_31_32")["sent_rows"] == 43  # the send is live on the rows r % 3 != 2; its second field reads a non-barely


def test_all_narrow_values():
    machine, t = cases.edge_machine(), cases.all_narrow_values()
    rep = va.domain_audit_host(machine, [t], [])
    assert np.array_equal(rep.words, ref.words(ref.audit(machine, [t], [])))
    k = rep.columns(0)[0]
    assert (k["distinct_narrow"], k["dense"], k["cls"], k["min"], k["max"], k["wide_rows"]) == (65536, True, "half", 0, 65535, 0)
    pos = rep.buses[0]["positions"][0]
    assert pos["is_send"] and pos["distinct_narrow"] == 65536 and pos["records"] == 65536


# ---- 4. options and refusals ----------------------------------------------------------------------------------------------------------------------
def test_max_bits(machines):
    mt, prep = witness("fib25")
    r8, r16 = va.domain_audit_host(machines["basic"], mt, prep, max_bits=8), va.domain_audit_host(machines["basic"], mt, prep, max_bits=16)
    assert np.array_equal(r8.words, ref.words(ref.audit(machines["basic"], mt, prep, max_bits=8))) and r8.max_bits == 8
    assert 0 < r8.total_entries < r16.total_entries and all(e["max"] < 256 for e in r8.entries) and any(e["max"] >= 256 for e in r16.entries)
    with pytest.raises(va.VgpuError, match="domain_audit: max_bits is at most 16") as e:
        va.domain_audit_host(machines["basic"], mt, prep, max_bits=17)
    assert e.value.code == -1


def test_limits_keep_counts_exact(machines):
    mt, prep = witness("fib25")
    full = reference(machines, "fib25")
    rep = va.domain_audit_host(machines["basic"], mt, prep, max_entries=0)
    assert rep.truncated and rep.reported == 0 and rep.total_entries == full["total_entries"] and rep.entries == []
    assert np.array_equal(rep.words, ref.words(ref.audit(machines["basic"], mt, prep, max_entries=0)))
    assert [c["entries"] for c in rep.chips] == [c["entries"] for c in full["chips"]]
    for R in (0, 1):
        rep = va.domain_audit_host(machines["basic"], mt, prep, max_rows_per_entry=R)
        assert np.array_equal(rep.words, ref.words(ref.audit(machines["basic"], mt, prep, max_rows_per_entry=R)))
        assert rep.reported == full["total_entries"] and all(len(e["rows"]) == R for e in rep.entries)
    rep = va.domain_audit_host(machines["basic"], mt, prep, max_entries=3)
    assert rep.truncated and rep.reported == 3 and rep.total_entries == full["total_entries"]
    for kw in (dict(max_entries=(1 << 24) + 1), dict(max_rows_per_entry=4097)):
        with pytest.raises(va.VgpuError, match="domain_audit: max_"):
            va.domain_audit_host(machines["basic"], mt, prep, **kw)


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    rep = va.domain_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM])
    assert np.array_equal(rep.words, ref.words(ref.audit(machines["basic"], mt, prep, chips=[ADD, MEM])))
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and {e["chip"] for e in rep.entries} == {MEM, ADD} and rep.columns(CPU) == []
    assert rep.buses == va.domain_audit_host(machines["basic"], mt, prep).buses  # the bus positions are the whole machine's
    with pytest.raises(va.VgpuError, match="domain_audit: chip_mask names a chip the machine does not have"):
        va.domain_audit_host(machines["basic"], mt, prep, chips=[20])


def test_explicit_lookup_buses(machines):
    mt, prep = witness("fib25")
    auto = va.domain_audit_host(machines["basic"], mt, prep)
    same = va.domain_audit_host(machines["basic"], mt, prep, lookup_buses=[(True, 2), 3])
    assert not same.lookup_auto and same.entries == auto.entries and same.buses == auto.buses
    only_range = va.domain_audit_host(machines["basic"], mt, prep, lookup_buses=[3])
    assert np.array_equal(only_range.words, ref.words(ref.audit(machines["basic"], mt, prep, lookup={(True, 3)})))
    assert only_range.lookup_buses() == [(True, 3)] and only_range.total_entries > auto.total_entries  # what only the memory bus guarded
    none = va.domain_audit_host(machines["basic"], mt, prep, lookup_buses=[])
    assert none.lookup_buses() == [] and all(k["guarded_rows"] == 0 for c in none.chips for k in none.columns(c["chip"]))
    assert va.domain_audit_host(machines["basic"], mt, prep, lookup_buses=[(False, 3)]).lookup_buses() == []  # a local bus the machine does not have
    wide = cases.needle_machine(bus=64)
    assert va.domain_audit_host(wide, cases.needle_traces(True), [], chips=[0]).total_entries == 1  # the structural rule takes any index
    with pytest.raises(va.VgpuError, match="domain_audit: bus index 64 of chip user does not fit the 64-bit lookup masks") as e:
        va.domain_audit_host(wide, cases.needle_traces(True), [], lookup_buses=[3])
    assert e.value.code == -1


def test_shapes_are_refused(machines):
    mt, prep = witness("fib25")
    for match, args in (("one main trace per chip", (mt[:-1], prep)), ("needs its preprocessed trace", (mt, prep[:1])), ("trace width mismatch", ([mt[1]] + mt[1:], prep)),
                        ("heights must be powers of two", ([mt[0][:63]] + mt[1:], prep))):
        with pytest.raises(va.VgpuError, match="domain_audit: .*" + match) as e:
            va.domain_audit_host(machines["basic"], *args)
        assert e.value.code == -1


def test_determinism(machines):
    mt, prep = witness("alu50")
    assert np.array_equal(va.domain_audit_host(machines["basic"], mt, prep, **ALL).words, va.domain_audit_host(machines["basic"], mt, prep, **ALL).words)


# ---- 5. the API edges ------------------------------------------------------------------------------------------------------------------------------
def test_signatures():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_entries", 1024, kind), ("max_rows_per_entry", 4, kind), ("chips", None, kind), ("max_bits", 16, kind), ("lookup_buses", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.domain_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.domain_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert ctypes.sizeof(va.DomainAuditOpts) == 48


def test_a_trace_is_a_matrix_and_chip_lists(machines):
    with pytest.raises(va.VgpuError) as e:
        va.domain_audit_host(machines["basic"], [np.zeros(4, dtype=np.uint32)], [])
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: domain_audit: traces are two-dimensional matrices"
    for chips in ([], [32]):
        with pytest.raises(va.VgpuError) as e:
            va.domain_audit_host(machines["basic"], [], [], chips=chips)
        assert e.value.code == -1 and str(e.value) == "vgpu error -1: domain_audit: chips is a non-empty list of chip indices below 32"


def test_null_options_reserved_fields_and_null_handles(machines):
    mt, prep = witness("fib1")
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    n, k = len(mains), len(preps)

    def call(opts):
        h = ctypes.c_void_p()
        rc = L.vgpu_domain_audit_host(machines["basic"]._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                      (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in preps]),
                                      (ctypes.c_void_p * k)(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * k)(*[m.shape[0] for _, m in preps]),
                                      (ctypes.c_uint64 * k)(*[m.shape[1] for _, m in preps]), ctypes.c_uint32(k), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
        return rc, (va._audit_report("domain", va.DomainReport, h).words if rc == 0 else None)

    want = va.domain_audit_host(machines["basic"], mt, prep).words
    rc, words = call(None)  # NULL options: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = call(va.DomainAuditOpts(1024, 4, 0, 0, 1, 0, 0, (ctypes.c_uint32 * 2)(0, 0)))  # max_bits 0: 16
    assert rc == 0 and np.array_equal(words, want)
    rc, _ = call(va.DomainAuditOpts(1024, 4, 0, 16, 1, 0, 0, (ctypes.c_uint32 * 2)(0, 1)))
    assert rc == -1  # reserved != 0 is refused
    rc, _ = call(va.DomainAuditOpts(1024, 4, 0, 16, 2, 0, 0, (ctypes.c_uint32 * 2)(0, 0)))
    assert rc == -1
    M = ctypes.CDLL(va.lib()._name)  # a handle of its own: the restypes set here are not the package's
    f = M.vgpu_domain_audit_host
    f.restype = ctypes.c_int32
    assert f(machines["basic"]._h, None, None, None, ctypes.c_uint32(0), None, None, None, None, ctypes.c_uint32(0), None, None) == -1
    length, words_of, timing, free = (getattr(M, "vgpu_domain_report_%s" % x) for x in ("len", "words", "timing", "free"))
    length.restype, words_of.restype, timing.restype, free.restype = ctypes.c_uint64, ctypes.c_void_p, None, None
    assert length(None) == 0 and words_of(None) is None
    tm = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    timing(None, tm)
    assert list(tm) == [0.0, 0.0, 0.0]
    free(None)


def test_to_json_round_trip(machines):
    rep = va.domain_audit_host(machines["basic"], *witness("fib25"))
    d = json.loads(rep.to_json())
    assert d == json.loads(json.dumps(rep.to_dict())) and set(d) == {"max_bits", "lookup_auto", "truncated", "total_entries", "reported", "device_ms", "host_ms", "evaluations", "chips",
                                                                      "columns", "buses", "entries"}
    assert d["total_entries"] == rep.total_entries and len(d["columns"]) == va.NUM_CHIPS and d["entries"][0]["rows"] == [list(r) for r in rep.entries[0]["rows"]]
    again = va.DomainReport(rep.words, rep.device_ms, rep.host_ms, rep.evaluations)
    assert again.to_dict() == rep.to_dict() and rep.device_ms == 0 and rep.evaluations > 0
    with pytest.raises(ValueError):
        va.DomainReport(rep.words[:-1])


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_domains_on_the_host(tmp_path, machines):
    bl, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out_plain, "--host")
    r = _cli("check", bl, out, "--host", "--domains")
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.domain_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    extra = lines[len(before):]
    assert len(extra) == sum(1 for c in rep.chips if c["entries"]) > 0
    for line, c in zip(extra, [c for c in rep.chips if c["entries"]]):
        assert line.startswith("%s: %d narrow column%s unguarded (column" % (va.CHIP_NAMES[c["chip"]], c["entries"], "" if c["entries"] == 1 else "s")) and line.endswith(")")
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    assert set(j) == set(plain_json) | {"domains"} and "narrow column" not in plain.stdout
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["domains"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--domains", "--chips=add,4", "--max-bits", 8, "--lookup-buses=3")
    j = json.loads(out.read_text())["domains"]
    assert r.returncode == 0 and [c["chip"] for c in j["chips"] if c["audited"]] == [ADD, SUB] and j["max_bits"] == 8 and not j["lookup_auto"]
    assert [(b["bus_index"], b["lookup"]) for b in j["buses"]] == [(0, False), (2, False), (3, True)]
    help_text = _cli("--help").stdout
    assert "--domains" in help_text and "--max-bits" in help_text and "--lookup-buses" in help_text and "never changes the exit status" in help_text


def test_cli_line_of_the_readme(machines):
    """The README's example line for fib(25) is what the CLI prints."""
    from valida_amd import cli

    rep = va.domain_audit_host(machines["basic"], *witness("fib25"), max_entries=1 << 20)
    line = "add: 4 narrow columns unguarded (columns 2-3,6-7: byte-valued on up to 103 rows, on no lookup send)"
    assert line in cli.domain_lines(rep)
    with open(os.path.join(ROOT, "README.md")) as f:
        assert line in f.read()


# ---- 7. the host audit under AddressSanitizer and UBSan, as a stand-alone program ----------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "emu", "domain_audit_host.cpp")
    exe = str(tmp_path / "domain_audit_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("domain_audit_host: ") and "fib25 entries" in r.stdout


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "domain_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libdomainauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "host", "domain_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("domain_audit.hip", "rank_audit.hip", "rank_elim.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_domain_audit.restype = ctypes.c_int64
    return L


def emulated(emu, machine_kind, mt, prep, max_slices=1 << 20, max_entries=1024, max_rows_per_entry=4, chips=None, max_bits=16, bus=cases.NEEDLE_BUS):
    """The report image of the emulated device pass (machine_kind 0: BasicMachine, 1: the needle machine, 2: the edge machine); max_slices large:
    one 256-row tile per slice, so that several workgroups merge through the bitmap in device memory."""
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    n, k = len(mains), len(preps)
    u, cap = ctypes.c_uint32, 1 << 22
    out = np.zeros(cap, dtype=np.uint32)
    mask = 0
    for c in chips or []:
        mask |= 1 << c
    got = emu.emu_domain_audit(u(machine_kind), u(bus), (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                               (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), u(n), (ctypes.c_uint32 * max(1, k))(*[c for c, _ in preps]),
                               (ctypes.c_void_p * max(1, k))(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * max(1, k))(*[m.shape[0] for _, m in preps]),
                               (ctypes.c_uint64 * max(1, k))(*[m.shape[1] for _, m in preps]), u(k), u(max_slices), u(max_entries), u(max_rows_per_entry), u(mask), u(max_bits),
                               out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(cap))
    assert got > 0, got
    return out[:got]


def test_emulated_kernels_on_fib25(emu, machines):
    mt, prep = witness("fib25")
    host = va.domain_audit_host(machines["basic"], mt, prep, max_rows_per_entry=300)
    assert np.array_equal(emulated(emu, 0, mt, prep, max_rows_per_entry=300), host.words)  # mem at 512 rows: two slices, two guard workgroups; lists over both
    assert np.array_equal(emulated(emu, 0, mt, prep, max_slices=1, max_rows_per_entry=300), host.words)  # one slice of several tiles
    host = va.domain_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM], max_bits=8, max_entries=3)
    assert np.array_equal(emulated(emu, 0, mt, prep, chips=[ADD, MEM], max_bits=8, max_entries=3), host.words)


def test_emulated_kernels_on_the_needle_and_the_edges(emu):
    machine = cases.needle_machine()
    for broken in (False, True):
        t = cases.needle_traces(broken)
        assert np.array_equal(emulated(emu, 1, t, []), va.domain_audit_host(machine, t, []).words)
    machine = cases.edge_machine()
    for name, t in cases.edge_traces():
        assert np.array_equal(emulated(emu, 2, [t], [], max_rows_per_entry=7), va.domain_audit_host(machine, [t], [], max_rows_per_entry=7).words), name
