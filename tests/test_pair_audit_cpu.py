"""The pair audit without a GPU: the host implementation of the contract (vgpu_pair_audit_host) against the brute-force restatement of
tests/pair_audit_ref.py (the oracle's own chip transcription, every pair at both rows, no coupling shortcut) word for word, for both machine
kinds; analytic AIRs captured through vgpu_air_* whose compensations are known in closed form; the theorem behind the pruning (uncoupled pairs
are never compensated) on every reference run; options; the device kernels' very source under tools/hipemu; `check --pairs` on the command line.
The reference of each input is computed once per module and cut to the limits a test asks for (counts do not depend on them).  The slack pairs
pinned here are the reference's, not the code under test's."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
SMALL_CHIPS = [c for c in range(14) if c not in (CPU, BITWISE)]  # the chips fib(25) and alu(50) are run on (the issue's choice)
ALL_ROWS = 4096  # the option's largest row limit: no trace of a reference input is higher (mem of alu(50): 2048 rows)
# name: (workload, chips audited)
INPUTS = {"fib1": (lambda: va.Workload.fib(1), None), "fib25": (lambda: va.Workload.fib(25), SMALL_CHIPS), "alu50": (lambda: va.Workload.alu(50), SMALL_CHIPS)}
# fib(25), chips other than cpu and bitwise: the slack pairs the reference finds
_BYTES = [(0, 4), (0, 11), (1, 5), (1, 12), (2, 6), (2, 13), (3, 7), (3, 14), (4, 11), (5, 12), (6, 13), (7, 14)]
FIB25_SLACK = {
    PROGRAM: [], MEM: [(7, 8)], ADD: _BYTES, SUB: _BYTES, MUL: [(14, 15), (14, 16), (15, 16)], DIV: [(12, 13)], SHIFT: [(7, 12)],
    LT: [(1, 5), (2, 6), (3, 7), (21, 24), (21, 26)], COM: [(0, 4), (1, 5), (2, 6), (3, 7)], OUTPUT: [], RANGE: [], STATIC_DATA: []}
_witness, _reference = {}, {}


def witness(name):
    if name not in _witness:
        w = INPUTS[name][0]()
        _witness[name] = (w.main_traces(), w.preprocessed())
    return _witness[name]


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def reference(machines, name, deltas=(1, P - 1), **limits):
    key = (name, tuple(deltas))
    if key not in _reference:
        mt, prep = witness(name)
        _reference[key] = ref.audit(machines["basic"], mt, prep, deltas=deltas, max_entries=1 << 24, max_rows_per_entry=ALL_ROWS, chips=INPUTS[name][1])
        assert _reference[key]["uncoupled_compensated"] == 0  # the theorem behind the pruning, on every reference run
    return ref.recut(_reference[key], **limits) if limits else ref.recut(_reference[key], 1024, 4)


def both(machines, name, deltas=(1, P - 1), **limits):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, deltas, **limits)
    mt, prep = witness(name)
    reps = {k: va.pair_audit_host(m, mt, prep, deltas=deltas, chips=INPUTS[name][1], **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
def test_fib1_every_chip(machines):
    mt, _ = witness("fib1")
    assert mt[CPU].shape[0] <= 32
    want, rep = both(machines, "fib1")
    assert all(c["audited"] for c in rep.chips) and rep.deltas == [1, P - 1]
    assert rep.chips[BITWISE]["coupled"] == 79 * 78 // 2 and rep.chips[CPU]["slack"] > 0  # height 1: every pair is coupled
    for chip in range(14):
        assert rep.chips[chip]["coupled"] == len(want["coupling"][chip])


def test_fib25_pinned_slack_pairs(machines):
    want, rep = both(machines, "fib25", max_entries=1 << 20)
    assert not rep.truncated
    for chip, pairs in FIB25_SLACK.items():
        assert sorted(set((e["c1"], e["c2"]) for e in want["entries"] if e["chip"] == chip)) == pairs, va.CHIP_NAMES[chip]
        assert rep.slack_pairs(chip) == pairs and rep.chips[chip]["slack"] == len(pairs)
    assert not rep.chips[CPU]["audited"] and rep.chips[CPU]["coupled"] == 0 and not any(rep.chips[CPU]["free"]) and rep.chips[CPU]["height"] == 256
    # every compensated row is free, and is in no other report: at least one of its singles is detected
    for e in rep.entries:
        assert 0 < e["compensated"] <= e["free"] <= rep.chips[e["chip"]]["height"]


def test_alu50(machines):
    want, rep = both(machines, "alu50", max_entries=1 << 20)
    assert {c: rep.chips[c]["height"] for c in (MEM, ADD, SUB, LT)} == {MEM: 2048, ADD: 256, SUB: 64, LT: 64}
    assert rep.chips[ADD]["slack"] > 0 and rep.chips[LT]["coupled"] < 45 * 44 // 2  # (lt at height 64 has uncoupled pairs)


# ---- 2. analytic AIRs through the capture interface ------------------------------------------------------------------------------------------
class VcolTerm(ctypes.Structure):  # vgpu_vcol_term_t
    _fields_ = [("is_preprocessed", ctypes.c_uint32), ("column", ctypes.c_uint32), ("weight", ctypes.c_uint32)]


class Vcol(ctypes.Structure):  # vgpu_vcol_t
    _fields_ = [("terms", ctypes.POINTER(VcolTerm)), ("n_terms", ctypes.c_uint32), ("constant", ctypes.c_uint32)]


class Interaction(ctypes.Structure):  # vgpu_interaction_t
    _fields_ = [("fields", ctypes.POINTER(Vcol)), ("n_fields", ctypes.c_uint32), ("count", Vcol), ("is_global", ctypes.c_uint32), ("bus_index", ctypes.c_uint32),
                ("is_send", ctypes.c_uint32)]


SUM3, BUS, SEP = range(3)


def analytic_machine():
    """Three captured AIRs: SUM3 (a, b, c) with the one constraint a + b - c = 0; BUS (a, b, m) without constraints and one interaction with
    the field a + b and the count m; SEP (a, b) with a (a - 1) = 0 and b (b - 1) = 0 — two columns in separate constraints."""
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0

    def new(name, width):
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
        return air

    def push(air):
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)

    air = new(b"sum3", 3)
    a, b, c = (L.vgpu_air_variable(air, u(0), u(k), u(0)) for k in range(3))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_add(air, u(a), u(b))), u(c))))
    push(air)
    air = new(b"bus", 3)
    terms = (VcolTerm * 2)(VcolTerm(0, 0, 1), VcolTerm(0, 1, 1))
    count = (VcolTerm * 1)(VcolTerm(0, 2, 1))
    fields = (Vcol * 1)(Vcol(terms, 2, 0))
    it = Interaction(fields, 1, Vcol(count, 1, 0), 0, 0, 1)
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
    push(air)
    air = new(b"sep", 2)
    one = L.vgpu_air_constant(air, u(1))
    for k in range(2):
        x = L.vgpu_air_variable(air, u(0), u(k), u(0))
        L.vgpu_air_assert_zero(air, u(L.vgpu_air_mul(air, u(x), u(L.vgpu_air_sub(air, u(x), u(one))))))
    push(air)
    return va.Machine(m)


def analytic_traces(n):
    r = np.arange(n, dtype=np.uint32)
    return [np.stack([r + 1, 2 * r + 3, 3 * r + 4], axis=1).astype(np.uint32), np.stack([r, np.full(n, 5), (r + 1) % 2], axis=1).astype(np.uint32),
            np.stack([r % 2, (r // 2) % 2], axis=1).astype(np.uint32)]


def check_analytic(rep, n):
    """The closed forms at deltas (1, p - 1): q = 0 (+1, +1), 1 (+1, -1), 2 (-1, +1), 3 (-1, -1)."""
    live = [r for r in range(n) if (r + 1) % 2]
    every = list(range(n))[:4]
    by = {(e["chip"], e["c1"], e["c2"], e["q"]): e for e in rep.entries}
    want = {(SUM3, 0, 1, 1): (n, n, every), (SUM3, 0, 1, 2): (n, n, every), (SUM3, 0, 2, 0): (n, n, every), (SUM3, 0, 2, 3): (n, n, every), (SUM3, 1, 2, 0): (n, n, every),
            (SUM3, 1, 2, 3): (n, n, every), (BUS, 0, 1, 1): (n, len(live), live[:4]), (BUS, 0, 1, 2): (n, len(live), live[:4])}
    assert {k: (e["free"], e["compensated"], e["rows"]) for k, e in by.items()} == want  # exactly these and nothing else
    s, b, p = rep.chips
    assert (s["coupled"], s["slack"], s["free"], s["compensated"]) == (3, 3, [2 * n, n, n, 2 * n], [2 * n, n, n, 2 * n])
    assert (b["coupled"], b["slack"], b["free"], b["compensated"]) == (3, 1, [n - len(live), n, n, n - len(live)], [0, len(live), len(live), 0])
    # sep: a + 1 is free where a = 0, a - 1 where a = 1 (likewise b); the pair is free exactly where both singles are
    a, bb = [r % 2 for r in range(n)], [(r // 2) % 2 for r in range(n)]
    free = [sum(1 for r in range(n) if a[r] == (0 if i == 0 else 1) and bb[r] == (0 if j == 0 else 1)) for i in range(2) for j in range(2)]
    assert (p["coupled"], p["slack"], p["free"], p["compensated"]) == (1 if n == 1 else 0, 0, free, [0, 0, 0, 0])
    assert rep.total_entries == rep.reported == 8 and not rep.truncated


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(n):
    rep = va.pair_audit_host(analytic_machine(), analytic_traces(n), [])
    check_analytic(rep, n)
    single = va.mutation_audit_host(analytic_machine(), analytic_traces(n), [])
    assert single.unbound_columns(SUM3) == [] and single.chips[SUM3]["free"] == [0, 0]  # what the mutation audit says of the same AIR: all bound


# ---- 3. options -------------------------------------------------------------------------------------------------------------------------------
def test_options(machines):
    full_want, full = both(machines, "fib1", max_entries=1 << 20)
    want, rep = both(machines, "fib1", max_entries=3)
    assert rep.truncated and rep.reported == 3 and rep.total_entries == full.total_entries > 3 and rep.chips == full.chips
    assert [(e["chip"], e["c1"], e["c2"], e["q"]) for e in rep.entries] == [(e["chip"], e["c1"], e["c2"], e["q"]) for e in full.entries[:3]]
    want, one = both(machines, "fib1", max_entries=1 << 20, max_rows_per_entry=1)
    want, many = both(machines, "fib1", max_entries=1 << 20, max_rows_per_entry=1000)
    assert one.chips == many.chips == full.chips and any(e["compensated"] > 4 for e in many.entries)
    for a, b in zip(one.entries, many.entries):
        assert len(a["rows"]) == 1 and a["rows"][0] == b["rows"][0] and b["rows"] == sorted(set(b["rows"])) and len(b["rows"]) == min(b["compensated"], 1000)
    # chip_mask zeroes the others and leaves the selected chips' words as they were
    mt, prep = witness("fib1")
    m = machines["basic"]
    part = va.pair_audit_host(m, mt, prep, max_entries=1 << 20, chips=[ADD, LT])
    for c, f in zip(part.chips, full.chips):
        if c["chip"] in (ADD, LT):
            assert c == f
        else:
            assert c == dict(f, audited=False, coupled=0, slack=0, free=[0] * 4, compensated=[0] * 4)
    assert part.entries == [e for e in full.entries if e["chip"] in (ADD, LT)]
    for deltas in ((1,), (2, 1, P - 1, 12345)):
        rep = va.pair_audit_host(m, mt, prep, deltas=deltas, max_entries=1 << 20, chips=[ADD, SUB, COM])
        D = len(deltas)
        assert rep.deltas == list(deltas) and all(len(c["free"]) == D * D for c in rep.chips)
        i = list(deltas).index(1)  # the pair (+1, +1) of any set is the default set's q = 0
        assert [c["compensated"][i * D + i] for c in rep.chips if c["audited"]] == [full.chips[c]["compensated"][0] for c in (ADD, SUB, COM)]


def test_argument_validation(machines):
    m = machines["basic"]
    mt, prep = witness("fib1")

    def refused(match, main=mt, pre=prep, **kw):
        with pytest.raises(va.VgpuError, match=match) as e:
            va.pair_audit_host(m, main, pre, **kw)
        assert e.value.code == -1  # VGPU_ERR_INVALID_ARG

    refused("pair_audit: need one main trace per chip", main=mt[:-1])
    refused("width mismatch for chip add", main=mt[:ADD] + [mt[ADD][:, :-1]] + mt[ADD + 1:])
    refused("powers of two", main=mt[:MUL] + [mt[MUL][:-1]] + mt[MUL + 1:])
    refused("needs its preprocessed trace", pre=prep[:1])
    refused("max_entries", max_entries=0)
    refused("1 to 4 deltas", deltas=())
    refused("a delta must be a canonical value in 1..p-1", deltas=(P,))
    refused("the deltas must be distinct", deltas=(5, 7, 5))
    refused("chips", chips=[])
    refused("chip_mask names a chip", chips=[14])
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[x.ctypes.data for x in mt])
    hs, ws = (ctypes.c_uint64 * 14)(*[x.shape[0] for x in mt]), (ctypes.c_uint64 * 14)(*[x.shape[1] for x in mt])
    pa = (ctypes.c_void_p * 2)(*[x.ctypes.data for _, x in prep])
    ph, pw = (ctypes.c_uint64 * 2)(*[x.shape[0] for _, x in prep]), (ctypes.c_uint64 * 2)(*[x.shape[1] for _, x in prep])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in prep])
    L = va.lib()

    def opts(max_entries=0, rows=0, n=0, deltas=(0, 0, 0, 0), mask=0, reserved=0):
        return ctypes.byref(va.PairAuditOpts(max_entries, rows, n, (ctypes.c_uint32 * 4)(*deltas), mask, reserved))

    assert ctypes.sizeof(va.PairAuditOpts) == 40
    assert L.vgpu_pair_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(reserved=1), ctypes.byref(h)) == -1 and b"reserved" in L.vgpu_last_error()
    assert L.vgpu_pair_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, opts(n=5), ctypes.byref(h)) == -1 and b"at most 4 deltas" in L.vgpu_last_error()
    assert L.vgpu_pair_audit_host(m._h, None, hs, ws, 14, chips, pa, ph, pw, 2, None, ctypes.byref(h)) == -1 and b"null" in L.vgpu_last_error()
    L.vgpu_pair_report_len.restype = ctypes.c_uint64
    L.vgpu_pair_report_words.restype = ctypes.POINTER(ctypes.c_uint32)
    L.vgpu_pair_report_len.argtypes = L.vgpu_pair_report_words.argtypes = L.vgpu_pair_report_free.argtypes = [ctypes.c_void_p]
    want = va.pair_audit_host(m, mt, prep).words
    for o in (opts(), None):  # a zeroed struct (or NULL) means the defaults
        assert L.vgpu_pair_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, o, ctypes.byref(h)) == 0
        n = L.vgpu_pair_report_len(h)
        assert np.array_equal(np.ctypeslib.as_array(L.vgpu_pair_report_words(h), shape=(n,)), want)
        L.vgpu_pair_report_free(h)


def test_report_image_and_json(machines):
    mt, prep = witness("fib1")
    rep = va.pair_audit_host(machines["basic"], mt, prep)
    w = [int(x) for x in rep.words]
    assert w[0] == 0x31525056 and bytes(rep.words[:1].tobytes()) == b"VPR1" and w[1] == len(w) and w[2:4] == [2, 0] and w[6:12] == [rep.reported, 14, 1, P - 1, 0, 0]
    assert rep.device_ms == 0.0 and rep.host_ms > 0 and rep.evaluations > 0
    again = va.PairReport(rep.words)
    assert again.entries == rep.entries and again.chips == rep.chips and again.deltas == rep.deltas
    j = json.loads(rep.to_json())
    assert j["deltas"] == [1, P - 1] and j["total_entries"] == rep.total_entries and j["entries"][0] == rep.entries[0] and j["chips"] == rep.chips
    assert np.array_equal(va.pair_audit_host(machines["basic"], mt, prep).words, rep.words)  # the same words run after run


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "pair_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libpairauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "pair_audit.hpp"), os.path.join(csrc, "host", "mutation_audit.hpp"),
            os.path.join(csrc, "host", "constraint_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("pair_audit.hip", "mutation_eval.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_pair_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, block_threads=0, deltas=(1, P - 1), max_entries=1024, max_rows_per_entry=4, pairs_per_slice=0, bus_walk=0, chips=None):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k, D = len(mt), len(prep), len(deltas)
    out = np.zeros(12 + 14 * (8 + 4 * D * D) + min(max_entries, 4096) * (10 + min(max_rows_per_entry, 4096)), np.uint32)
    got = emu.emu_pair_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(block_threads), ctypes.c_uint32(pairs_per_slice), ctypes.c_uint32(bus_walk), (ctypes.c_uint32 * D)(*deltas), ctypes.c_uint32(D), ctypes.c_uint32(max_entries),
        ctypes.c_uint32(max_rows_per_entry), ctypes.c_uint32(sum(1 << c for c in chips) if chips else 0), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    return out[:got]


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
def test_kernel_source_under_emulation(machines, emu, interpret):
    """Counting pass, scan and listing pass of pair_audit.hip, the compiled chip templates, the interpreted programs and the bus-only chips: the
    assembled report is the reference's, word for word.  fib(1) runs every chip (the height-1 chips sliced); in fib(25) mul (1024 rows), mem
    (512) and add (128) span several workgroups, with 64-row workgroups all the more, so the r - 1 halo, the wrap between row 0 and row n - 1
    and the rank scan all cross workgroup boundaries (mul's compensated rows number 1024 per entry: lists of 300 run over five workgroups)."""
    mt, prep = witness("fib1")
    for kw in (dict(), dict(pairs_per_slice=7, max_rows_per_entry=100, max_entries=40), dict(bus_walk=1, pairs_per_slice=1 << 20)):
        limits = dict(max_entries=kw.get("max_entries", 1024), max_rows_per_entry=kw.get("max_rows_per_entry", 4))
        assert np.array_equal(emulated(emu, mt, prep, interpret, **kw), ref.words(reference(machines, "fib1", **limits)))
    mt, prep = witness("fib25")
    assert mt[MUL].shape[0] == 1024 and mt[MEM].shape[0] == 512
    for kw in (dict(block_threads=64, max_rows_per_entry=300), dict(pairs_per_slice=1 << 20, max_rows_per_entry=3)):
        got = emulated(emu, mt, prep, interpret, chips=SMALL_CHIPS, **kw)
        assert np.array_equal(got, ref.words(reference(machines, "fib25", max_entries=1024, max_rows_per_entry=kw["max_rows_per_entry"])))
    if not interpret:  # four deltas (16 delta pairs per pair, 64 pairs per slice): against the host audit
        deltas = (2, 1, P - 1, 12345)
        host = va.pair_audit_host(machines["basic"], mt, prep, deltas=deltas, chips=[ADD, LT, COM])
        assert np.array_equal(emulated(emu, mt, prep, 0, deltas=deltas, chips=[ADD, LT, COM]), host.words)


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def exe(prog, advice=b""):
    return va.Workload.from_executable(vp.machine_code(prog), advice=advice)


def test_cli_check_pairs_on_the_host(tmp_path, machines):
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out, "--host")
    plain_json = json.loads(out.read_text())
    r = _cli("check", bl, out, "--host", "--pairs")
    assert r.returncode == plain.returncode == 0, r.stderr  # a slack pair is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = exe(vp.byte_loads_program())
    rep = va.pair_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_entries=1 << 20)
    chips = [c for c in rep.chips if c["slack"]]
    assert chips and len(lines) == len(before) + len(chips)
    for line, c in zip(lines[len(before):], chips):
        assert line.startswith("%s: %d slack pair%s of %d coupled: (%d,%d)" % ((va.CHIP_NAMES[c["chip"]], c["slack"], "" if c["slack"] == 1 else "s", c["coupled"]) + rep.slack_pairs(c["chip"])[0]))
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"pairs"} and {k: v for k, v in j.items() if k not in ("pairs", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["pairs"].items() if k not in timing} == {k: v for k, v in rep.to_dict().items() if k not in timing}
    r = _cli("check", bl, out, "--host", "--pairs", "--deltas=2", "--chips=add,4")
    p = json.loads(out.read_text())["pairs"]
    assert r.returncode == 0 and p["deltas"] == [2] and [c["chip"] for c in p["chips"] if c["audited"]] == [ADD, SUB]
    r = _cli("check", bl, out, "--host", "--pairs", "--chips=nochip")
    assert r.returncode != 0 and "neither a chip name" in r.stderr + r.stdout
