"""The transition audit without a GPU: the host audit (vgpu_transition_audit_host) against the numpy reference of tests/transition_audit_ref.py
word for word, under Machine.basic() and Machine.basic_via_ffi(); what the reference finds on fib(25) and alu(50), pinned; holds(); the
captured step AIR at the lane-word boundaries and beyond the device's widest window; the needle traces; limits and chip mask; the API edges;
`check --host --transitions`; the device kernels' source under tools/hipemu against the host audit; the host audit as a sanitized
stand-alone program.  Trace heights are powers of two (every audit's rule): the gated analytic cases run at 256 rows and more."""
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

import transition_audit_cases as cases
import transition_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, BITWISE, CPU, MEM, MUL, RANGE, SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
PROGRAM = 1
INPUTS = {"fib1": lambda: va.Workload.fib(1), "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50)}
LIMITS = {"fib1": dict(max_rows_per_entry=64, max_terms=3), "fib25": dict(max_entries=1 << 20, max_rows_per_entry=7, max_terms=64), "alu50": dict(max_rows_per_entry=5, max_terms=32)}
_witness, _both = {}, {}


def witness(name):
    if name not in _witness:
        w = INPUTS[name]()
        _witness[name] = (w.main_traces(), w.preprocessed())
    return _witness[name]


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def both(machines, name):
    """The reference's report (made once per witness) and the host audit's under both machine kinds: equal word for word."""
    if name not in _both:
        mt, prep = witness(name)
        want = ref.audit(machines["basic"], mt, prep, **LIMITS[name])
        reps = {k: va.transition_audit_host(m, mt, prep, **LIMITS[name]) for k, m in machines.items()}
        for rep in reps.values():
            ref.assert_report_equals(rep, want)
            assert np.array_equal(rep.words, ref.words(want))
        _both[name] = (want, reps["basic"])
    return _both[name]


def entries_of(rep, chip, gate):
    return {e["column"]: e for e in rep.entries if e["chip"] == chip and e["gate"] == gate}


# ---- 1. the host audit equals the reference; the facts the reference finds ----------------------------------------------------------------------
def test_fib1_every_chip(machines):
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and not rep.truncated and rep.total_entries == rep.reported > 0
    for c in rep.chips:
        if c["height"] == 1:  # no windows: the block is zero
            assert (c["n_gates"], c["gates_listed"], c["rank"], c["dim"], c["transitions"], c["gated"]) == (0, 0, 0, 0, 0, 0)
        else:
            assert c["rank"] + c["dim"] == 2 * c["width"] + 1 == c["rank"] + c["local_only"] + c["next_only"] + c["transitions"] and c["n_gates"] == 1 + 2 * c["n_bool"]
    assert [g["chip"] for g in rep.gates] == sorted(g["chip"] for g in rep.gates) and all(g["audited"] == (g["column"] == 0 or g["windows"] >= 64) for g in rep.gates)


def test_fib25_pinned_findings(machines):
    """What the commented-out memory AIR leads one to expect, and what this witness says.  addr_not_equal and diff are zero on every row of the
    trace (nothing fills them while the AIR is empty), so addr_not_equal is no gate and the three relations under it are not there to find.
    next.counter = counter + 1 holds between operation rows only; the padding rows (is_read + is_write = 0, one counter value) break it, and the
    audit finds it in the form that the padding repairs: next.counter - counter + 400 (is_read + is_write) - 401 (next.is_read + next.is_write)
    = 0, which is next.counter = counter + 1 between two operation rows.  What IS there under a selector: when(next.is_read), next.addr = addr and next.value = value (bytes 1 .. 3; byte 0 is 0
    or 1 on this witness and is itself a gate column), held at each of the gate's 288 windows: the bus record of either row carries the
    address and the value, and mem has no constraint that reads `next`, so for this chip held is exact."""
    want, rep = both(machines, "fib25")
    mem = witness("fib25")[0][MEM]
    assert not mem[:, 9].any() and not mem[:, 11].any()  # diff, addr_not_equal
    c = rep.chips[MEM]
    assert (c["height"], c["width"], c["n_bool"], c["n_gates"], c["gates_audited"], c["rank"], c["dim"], c["local_only"], c["next_only"], c["transitions"], c["gated"]) == (
        512, 14, 6, 13, 11, 16, 13, 6, 6, 1, 21)
    W = 14
    is_read, is_write, counter = 7, 8, 12
    e = entries_of(rep, MEM, None)
    assert sorted(e) == [1 + W + counter] and e[1 + W + counter]["l0"] == 0 and e[1 + W + counter]["kind"] == "both_blocks"
    assert e[1 + W + counter]["terms"] == [(1 + is_read, 400), (1 + is_write, 400), (1 + counter, P - 1), (1 + W + is_read, P - 401), (1 + W + is_write, P - 401), (1 + W + counter, 1)]
    assert (e[1 + W + counter]["free_windows"], e[1 + W + counter]["held_windows"], e[1 + W + counter]["rows"]) == (511, 0, list(range(7)))
    g = entries_of(rep, MEM, (1 + W + is_read, 1))  # when(next.is_read)
    assert sorted(g) == [9, 15, 17, 18, 19, 23]
    for col in (0, 2, 3, 4):  # next.addr = addr, next.value[1..3] = value[1..3]
        assert g[1 + W + col]["terms"] == [(1 + col, P - 1), (1 + W + col, 1)] and g[1 + W + col]["l0"] == 0
        assert (g[1 + W + col]["free_windows"], g[1 + W + col]["held_windows"]) == (0, 288)
    assert [x["windows"] for x in rep.gates if x["chip"] == MEM and x["column"] == 1 + W + is_read] == [288, 223]
    c = rep.chips[CPU]
    assert (c["height"], c["width"], c["n_bool"], c["gates_audited"], c["rank"], c["dim"], c["local_only"], c["next_only"], c["transitions"], c["gated"]) == (256, 51, 30, 45, 49, 54, 23, 17, 14, 626)
    assert rep.chips[RANGE]["transitions"] == 1 and rep.chips[PROGRAM]["dim"] == 0 and rep.total_entries == 677
    for e in rep.entries:
        windows = [x["windows"] for x in rep.gates if x["chip"] == e["chip"] and (x["column"], x["value"]) == (e["gate"] or (0, 0))]
        assert [e["free_windows"] + e["held_windows"]] == windows and e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(7, e["free_windows"])
        assert e["terms"][-1] == (e["column"], 1) or e["support"] > len(e["terms"])


def test_alu50_pinned_findings(machines):
    want, rep = both(machines, "alu50")
    assert rep.truncated and rep.reported == 1024 and rep.total_entries == 11580
    c = rep.chips[MEM]
    assert (c["height"], c["transitions"], c["gated"]) == (2048, 1, 24)
    W, is_read, is_write, counter = 14, 7, 8, 12
    full = va.transition_audit_host(machines["basic"], *witness("alu50"), chips=[MEM], max_terms=32)
    e = entries_of(full, MEM, None)[1 + W + counter]
    assert e["terms"] == [(1 + is_read, 1153), (1 + is_write, 1153), (1 + counter, P - 1), (1 + W + is_read, P - 1154), (1 + W + is_write, P - 1154), (1 + W + counter, 1)]
    g = entries_of(full, MEM, (1 + W + is_read, 1))
    assert sorted(g) == [9, 15, 16, 17, 18, 19, 23] and all((g[1 + W + col]["free_windows"], g[1 + W + col]["held_windows"]) == (0, 750) for col in range(5))
    c = rep.chips[BITWISE]  # 159 window columns: the widest of the BasicMachine
    assert (c["height"], c["width"], c["rank"] + c["dim"]) == (256, 79, 159) and not full.chips[BITWISE]["audited"]


# ---- 2. holds() ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib25", "alu50"])
def test_holds_on_the_audited_traces_and_names_a_broken_entry(machines, name):
    mt, prep = witness(name)
    rep = va.transition_audit_host(machines["basic"], mt, prep, max_entries=1 << 20 if name == "fib25" else 1024, max_terms=256)
    assert rep.holds(mt) == []
    W, counter = 14, 12
    broken = [m.copy() for m in mt]
    broken[MEM][3, counter] = (int(broken[MEM][3, counter]) + 1) % P  # rows 2 | 3 and 3 | 4: the counter's relation and whatever else reads the counter
    bad = rep.holds(broken)
    assert (MEM, None, 1 + W + counter) in bad and all(x[0] == MEM for x in bad)


# ---- 3. the captured step AIR -------------------------------------------------------------------------------------------------------------------
def step_both(width, n, **kw):
    machine, t = cases.step_machine(width), cases.step_trace(n, width)
    rep = va.transition_audit_host(machine, [t], [], max_terms=16, **kw)
    want = ref.audit(machine, [t], [], max_terms=16, jacobians=cases.step_jacobians(width), **kw)
    ref.assert_report_equals(rep, want)
    assert np.array_equal(rep.words, ref.words(want)) and rep.holds([t]) == []
    return rep


@pytest.mark.parametrize("n", [2, 8])
def test_step_air_layout(n):
    """n = 8: seven windows; every gate is audited at min_gate_windows = 2 and none but gate 0 at the default.  n = 2: one window."""
    rep = step_both(5, n, min_gate_windows=2)
    c = rep.chips[0]
    assert (c["height"], c["rank"] + c["dim"], c["n_gates"]) == (n, 11, 5 if n == 8 else 1)
    if n == 8:
        e = entries_of(rep, 0, None)[1 + 5]
        assert (e["l0"], e["terms"], e["free_windows"], e["held_windows"]) == (P - 1, [(1, P - 1), (6, 1)], 0, 7)
        plain = step_both(5, n)
        assert [g["audited"] for g in plain.gates] == [True, False, False, False, False] and plain.chips[0]["gated"] == 0


@pytest.mark.parametrize("width", [31, 32, 64, 91, 92])
def test_step_air_gated(width):
    """2 w + 1 = 63, 65, 129 (the lane-word boundaries of the device pass), 183 (its widest window) and 185 (refused there, answered here).
    next.c0 - c0 - 1 at gate 0, held on every window; c2 - c0 - 4 under (local c1 = 1) only; next.c3 - c3 - c0 under (next c1 = 0) only, free
    on every gated window."""
    n, W = cases.step_height(width), width
    rep = step_both(width, n)
    assert [(g["column"], g["value"], g["audited"]) for g in rep.gates] == [(0, 0, True), (2, 1, True), (2, 0, True), (2 + W, 1, True), (2 + W, 0, True)]
    assert rep.chips[0]["rank"] == 2 * W and rep.chips[0]["transitions"] == 1
    e = entries_of(rep, 0, None)
    assert sorted(e) == [1 + W] and (e[1 + W]["l0"], e[1 + W]["terms"], e[1 + W]["free_windows"], e[1 + W]["held_windows"]) == (P - 1, [(1, P - 1), (1 + W, 1)], 0, n - 1)
    c2 = [(x["gate"], x["l0"], x["terms"], x["kind"], x["held_windows"]) for x in rep.entries if x["column"] == 1 + 2]
    assert c2 == [((2, 1), P - 4, [(1, P - 1), (3, 1)], "one_block", 0)]
    c3 = [(x["gate"], x["l0"], x["terms"], x["kind"], x["held_windows"], x["rows"]) for x in rep.entries if x["column"] == 1 + W + 3]
    free_at = [r for r in range(n - 1) if (r + 1) % 3][:4]
    assert c3 == [((2, 1), 0, [(1, P - 1), (4, P - 1), (1 + W + 3, 1)], "both_blocks", 0, [0, 3, 6, 9]), ((2 + W, 0), 0, [(1, P - 1), (4, P - 1), (1 + W + 3, 1)], "both_blocks", 0, free_at)]


# ---- 4. needle traces ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "first", "last", "straddle"])
def test_needle_traces(kind):
    machine, t = cases.free_machine(cases.NEEDLE_W), cases.needle(kind)
    rep = va.transition_audit_host(machine, [t], [])
    want = ref.audit(machine, [t], [], jacobians=cases.free_jacobians(cases.NEEDLE_W))
    ref.assert_report_equals(rep, want)
    assert np.array_equal(rep.words, ref.words(want))
    found = [(e["l0"], e["terms"], e["free_windows"]) for e in rep.entries if e["gate"] is None and e["column"] == cases.NEEDLE_F]
    assert found == ([(P - 7, cases.NEEDLE_TERMS, cases.NEEDLE_N - 1)] if kind == "none" else [])  # one window is enough to lose the relation
    gates = {(g["column"], g["value"]): g for g in rep.gates}
    # 63 windows: counted, not audited; 64: audited
    assert (gates[5, 1]["windows"], gates[5, 1]["audited"], gates[5, 1]["rank"]) == (63, False, 0) and (gates[7, 1]["windows"], gates[7, 1]["audited"]) == (64, True)
    assert gates[7, 1]["rank"] > 0 and rep.chips[0]["gates_audited"] == rep.chips[0]["gates_listed"] - (3 if kind == "none" else 3)
    # c1: boolean as `local` always; as `next` unless row n - 1 holds a 2
    assert (2, 1) in gates and ((2 + cases.NEEDLE_W, 1) in gates) == (kind != "none")
    lowered = va.transition_audit_host(machine, [t], [], min_gate_windows=63)
    assert {(g["column"], g["value"]): g["audited"] for g in lowered.gates}[5, 1] and lowered.total_entries > rep.total_entries


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------------------
def test_limits_keep_totals_exact(machines):
    mt, prep = witness("fib25")
    full = both(machines, "fib25")[1]
    cut = va.transition_audit_host(machines["basic"], mt, prep, max_entries=9, max_rows_per_entry=2, max_terms=2)
    assert cut.truncated and cut.reported == 9 and cut.total_entries == full.total_entries == 677 and cut.chips == full.chips and cut.gates == full.gates
    for a, b in zip(cut.entries, full.entries):  # the entries that stay are judged as before
        assert (a["column"], a["gate"], a["support"], a["free_windows"], a["held_windows"]) == (b["column"], b["gate"], b["support"], b["free_windows"], b["held_windows"])
        assert a["terms"] == b["terms"][:2] and a["rows"] == b["rows"][:2]
    few = va.transition_audit_host(machines["basic"], mt, prep, max_gates=7, max_entries=1 << 20)
    c = few.chips[CPU]
    assert (c["n_bool"], c["n_gates"], c["gates_listed"]) == (30, 61, 7) and [g for g in few.gates if g["chip"] == CPU] == [g for g in full.gates if g["chip"] == CPU][:7]
    assert few.chips[MEM]["gates_listed"] == 7 and few.total_entries < full.total_entries
    want = ref.audit(machines["basic"], mt, prep, max_gates=7, max_entries=40, min_gate_windows=100, chips=[CPU, MEM])
    got = va.transition_audit_host(machines["basic"], mt, prep, max_gates=7, max_entries=40, min_gate_windows=100, chips=[CPU, MEM])
    ref.assert_report_equals(got, want)
    assert np.array_equal(got.words, ref.words(want)) and got.truncated


def test_chip_mask(machines):
    mt, prep = witness("fib25")
    full = both(machines, "fib25")[1]
    rep = va.transition_audit_host(machines["basic"], mt, prep, chips=[ADD, MEM], **LIMITS["fib25"])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["n_gates"] == 0 and rep.chips[CPU]["width"] == 51
    assert rep.entries == [e for e in full.entries if e["chip"] in (ADD, MEM)] and rep.gates == [g for g in full.gates if g["chip"] in (ADD, MEM)]


def test_max_terms_cut_and_holds_refuses(machines):
    mt, prep = witness("fib25")
    rep = va.transition_audit_host(machines["basic"], mt, prep, max_terms=3, chips=[MEM])
    e = entries_of(rep, MEM, None)[27]
    assert (e["support"], e["terms"]) == (6, [(8, 400), (9, 400), (13, P - 1)])  # the first three, ascending; the support stays exact
    with pytest.raises(va.VgpuError, match="is cut"):
        rep.holds(mt)


# ---- 6. the API edges of tests/test_audit_api_cpu.py, for this audit ------------------------------------------------------------------------------
def test_signatures():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_entries", 1024, kind), ("max_rows_per_entry", 4, kind), ("max_terms", 8, kind), ("min_gate_windows", 64, kind), ("max_gates", 256, kind), ("chips", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.transition_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.transition_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert signature_of(va.TransitionReport.holds) == [("self", empty, kind), ("main_matrices", empty, kind)]


def test_a_trace_is_a_matrix(machines):
    for args in (([np.zeros(4, dtype=np.uint32)], []), ([], [(0, np.zeros(4, dtype=np.uint32))])):
        with pytest.raises(va.VgpuError) as e:
            va.transition_audit_host(machines["basic"], *args)
        assert e.value.code == -1 and str(e.value) == "vgpu error -1: transition_audit: traces are two-dimensional matrices"


@pytest.mark.parametrize("chips", [[], [32]])
def test_chip_lists(machines, chips):
    with pytest.raises(va.VgpuError) as e:
        va.transition_audit_host(machines["basic"], [], [], chips=chips)
    assert e.value.code == -1 and str(e.value) == "vgpu error -1: transition_audit: chips is a non-empty list of chip indices below 32"


def test_option_refusals(machines):
    mt, prep = witness("fib1")
    for match, kw in (("must be at least 1", dict(min_gate_windows=0)), ("must be at least 1", dict(max_gates=0)), ("max_gates is at most 4096", dict(max_gates=4097)),
                      ("max_terms is at most 4096", dict(max_terms=4097)), ("one main trace per chip", dict(mt=mt[:-1])), ("powers of two", dict(mt=[mt[0][:24]] + mt[1:]))):
        with pytest.raises(va.VgpuError, match="transition_audit: .*" + match) as e:
            va.transition_audit_host(machines["basic"], kw.pop("mt", mt), prep, **kw)
        assert e.value.code == -1


def test_null_out_and_null_report_handle(machines):
    L = ctypes.CDLL(va.lib()._name)  # a handle of its own: the restypes set here are not the package's
    f = L.vgpu_transition_audit_host
    f.restype = ctypes.c_int32
    L.vgpu_last_error.restype = ctypes.c_char_p
    assert f(machines["basic"]._h, None, None, None, ctypes.c_uint32(0), None, None, None, None, ctypes.c_uint32(0), None, None) == -1
    assert L.vgpu_last_error()
    length, words, timing, free = (getattr(L, "vgpu_transition_report_%s" % x) for x in ("len", "words", "timing", "free"))
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
        rc = L.vgpu_transition_audit_host(machines["basic"]._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                          (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in preps]),
                                          (ctypes.c_void_p * k)(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * k)(*[m.shape[0] for _, m in preps]),
                                          (ctypes.c_uint64 * k)(*[m.shape[1] for _, m in preps]), ctypes.c_uint32(k), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
        return rc, (va._audit_report("transition", va.TransitionReport, h).words if rc == 0 else None)

    want = va.transition_audit_host(machines["basic"], mt, prep).words
    rc, words = call(None)  # NULL options: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = call(va.TransitionAuditOpts(0, 0, 0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 0, 0)))  # zero fields: the defaults
    assert rc == 0 and np.array_equal(words, want) and (int(words[9]), int(words[10])) == (64, 256)
    rc, _ = call(va.TransitionAuditOpts(0, 0, 0, 0, 0, 0, (ctypes.c_uint32 * 3)(0, 1, 0)))
    assert rc == -1  # reserved != 0 is refused


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_transitions_on_the_host(tmp_path, machines):
    from valida_amd.cli import transition_lines

    bl, out, out_plain = tmp_path / "byte_loads.bin", tmp_path / "report.json", tmp_path / "plain.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out_plain, "--host")
    r = _cli("check", bl, out, "--host", "--transitions", "--min-gate-windows", 8)
    assert r.returncode == plain.returncode == 0, r.stderr
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.transition_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_terms=256, min_gate_windows=8)
    expect = transition_lines(rep)
    assert expect and lines[len(before):] == expect
    head = [x for x in expect if x.startswith("cpu: ")][0]
    c, mine = rep.chips[CPU], [e for e in rep.entries if e["chip"] == CPU]
    assert head.startswith("cpu: %d transition relations (%d held on every window); %d gated relations" % (
        c["transitions"], len([e for e in mine if e["gate"] is None and not e["free_windows"]]), c["gated"])) and "gates in all" in head and "never held" in head
    j, plain_json = json.loads(out.read_text()), json.loads(out_plain.read_text())
    assert set(j) == set(plain_json) | {"transitions"} and "transition" not in plain.stdout
    assert {k: v for k, v in j.items() if k not in ("transitions", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["transitions"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    r = _cli("check", bl, out, "--host", "--transitions", "--chips=add,4", "--max-gates", 3)
    j = json.loads(out.read_text())["transitions"]
    assert r.returncode == 0 and [c["chip"] for c in j["chips"] if c["audited"]] == [ADD, SUB] and j["max_gates"] == 3 and all(c["gates_listed"] <= 3 for c in j["chips"])
    help_text = _cli("--help").stdout
    assert "--transitions" in help_text and "--min-gate-windows" in help_text and "--max-gates" in help_text


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "transition_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libtransitionauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "transition_audit.hpp"), os.path.join(csrc, "host", "rank_audit.hpp"),
            os.path.join(csrc, "host", "mutation_audit.hpp"), os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("transition_audit.hip", "rank_elim.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_transition_audit.restype = ctypes.c_int64
    L.emu_ta_basis_shape.restype = ctypes.c_int32
    return L


def emulated(emu, machine_kind, mt, prep, interpret, rows_per_wave=0, windows_per_slice=0, windows_per_count=0, entries_per_chunk=0, max_entries=1024, max_rows_per_entry=4, max_terms=8,
             min_gate_windows=64, max_gates=256, chips=None):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(1 << 22, np.uint32)
    u32, u64, vp_ = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    got = emu.emu_transition_audit(
        u32(machine_kind), (vp_ * n)(*[m.ctypes.data for m in keep[:n]]), (u64 * n)(*[m.shape[0] for m in keep[:n]]), (u64 * n)(*[m.shape[1] for m in keep[:n]]), u32(n),
        (u32 * max(1, k))(*[c for c, _ in prep]), (vp_ * max(1, k))(*[m.ctypes.data for m in keep[n:]]), (u64 * max(1, k))(*[m.shape[0] for m in keep[n:]]),
        (u64 * max(1, k))(*[m.shape[1] for m in keep[n:]]), u32(k), u32(interpret), u32(rows_per_wave), u32(windows_per_slice), u32(windows_per_count), u32(entries_per_chunk),
        u32(max_entries), u32(max_rows_per_entry), u32(max_terms), u32(min_gate_windows), u32(max_gates), u32(sum(1 << c for c in chips) if chips else 0), out.ctypes.data_as(vp_),
        u64(out.size))
    assert got > 0
    return out[:got]


def test_kernel_source_under_emulation(machines, emu):
    """Every kernel of transition_audit.hip (with rank_elim.hpp) with the wave primitives in their emulation forms, on fib(1) without mul (1024
    rows; the emulated ballots are slow): the compiled chip templates at ta_shape's own launch shapes, then the interpreted register programs
    with 3 windows per elimination slice (mem: 21 partial bases per gate, two levels of the tree; gates over the grid's y), 3 rows per
    enforcement workgroup (the halo, the wrap, and windows whose two rows lie in different workgroups), 5 windows per workgroup of the count
    and list passes, the entries' vectors staged 2 at a time (a word of bits spans chunks), every gate of at least 4 windows audited.  The
    assembled report is the host audit's, word for word."""
    mt, prep = witness("fib1")
    chips = [c for c in range(14) if c != MUL]
    host = va.transition_audit_host(machines["basic"], mt, prep, chips=chips)
    assert host.reported > 0 and host.chips[CPU]["transitions"] > 0
    assert np.array_equal(emulated(emu, 0, mt, prep, 0, chips=chips), host.words)
    host = va.transition_audit_host(machines["basic"], mt, prep, chips=chips, min_gate_windows=4, max_rows_per_entry=20)
    assert host.reported > 500 and any(len(e["rows"]) == 20 and e["rows"][-1] - e["rows"][0] > 6 for e in host.entries) and any(e["held_windows"] and e["free_windows"] for e in host.entries)
    got = emulated(emu, 0, mt, prep, 1, rows_per_wave=3, windows_per_slice=3, windows_per_count=5, entries_per_chunk=2, chips=chips, min_gate_windows=4, max_rows_per_entry=20)
    assert np.array_equal(got, host.words)


@pytest.mark.parametrize("width", [31, 32])
def test_step_airs_under_emulation(emu, width):
    """2 w + 1 = 63 and 65 window columns: one and two words per lane; 128 rows, 40 windows per slice (four partial bases per gate)."""
    machine, t = cases.step_machine(width), cases.step_trace(128, width)
    host = va.transition_audit_host(machine, [t], [], min_gate_windows=30, max_rows_per_entry=8)
    assert host.chips[0]["gates_audited"] == 5 and host.reported > 0
    assert np.array_equal(emulated(emu, 4, [t], [], 1, rows_per_wave=3, windows_per_slice=40, windows_per_count=50, min_gate_windows=30, max_rows_per_entry=8), host.words)


@pytest.mark.parametrize("kind", ["none", "first", "straddle"])
def test_needle_traces_under_emulation(emu, kind):
    """The needle traces' first 512 rows, 32 windows per slice as on the device (16 partial bases per gate; 'straddle': window 95 reads the
    first row of the following slice), limits that cut the list."""
    t = np.ascontiguousarray(cases.needle(kind)[:512])
    machine = cases.free_machine(cases.NEEDLE_W)
    host = va.transition_audit_host(machine, [t], [], max_entries=5, max_terms=2)
    assert host.truncated and ([e["column"] for e in host.entries if e["gate"] is None and e["column"] == cases.NEEDLE_F] == [cases.NEEDLE_F]) == (kind == "none")
    assert np.array_equal(emulated(emu, 2, [t], [], 1, windows_per_slice=32, rows_per_wave=4, max_entries=5, max_terms=2), host.words)


def test_the_widest_window(emu):
    out = (ctypes.c_uint64 * 3)()
    assert emu.emu_ta_basis_shape(ctypes.c_uint32(91), ctypes.c_uint64(1 << 20), ctypes.c_uint32(256), out) == 0 and out[2] <= 160 * 1024  # 183 window columns
    assert out[0] % 32 == 0 and out[1] == ((1 << 20) - 1 + out[0] - 1) // out[0]
    assert emu.emu_ta_basis_shape(ctypes.c_uint32(92), ctypes.c_uint64(1 << 20), ctypes.c_uint32(256), out) == 1  # 185: refused
    assert emu.emu_ta_basis_shape(ctypes.c_uint32(79), ctypes.c_uint64(1 << 20), ctypes.c_uint32(256), out) == 0  # bitwise: 159


# ---- 9. C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_transition_audit", "vgpu_transition_audit_host", "vgpu_transition_report_len", "vgpu_transition_report_words", "vgpu_transition_report_timing",
             "vgpu_transition_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Transition audit" in header and "VTR1" in header and "vgpu_transition_audit_opts_t" in header and ctypes.sizeof(va.TransitionAuditOpts) == 40


# ---- 10. the host audit under the sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path, machines):
    """tests/emu/transition_audit_host.cpp: fib(25) on the host VM and the host transition audit, built with AddressSanitizer and UBSan and run
    as a subprocess (nothing sanitized is loaded into this interpreter).  Its figures are the library's for the same limits."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "transition_audit_host")
    subprocess.run([gxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "emu", "transition_audit_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe, "25"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    mt, prep = witness("fib25")
    rep = va.transition_audit_host(machines["basic"], mt, prep, max_entries=1 << 20, max_rows_per_entry=64, max_terms=16)
    assert ("fib(25): %d words, %d entries, %d gates, %d transition relations, %d gated relations, %d never held" % (
        len(rep.words), rep.total_entries, len(rep.gates), sum(c["transitions"] for c in rep.chips), sum(c["gated"] for c in rep.chips),
        len([e for e in rep.entries if e["held_windows"] == 0]))) in r.stdout, r.stdout
