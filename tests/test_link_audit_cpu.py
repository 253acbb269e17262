"""The link audit without a GPU: the host implementation of the contract (vgpu_link_audit_host) against the restatement of
tests/link_audit_ref.py (the field audit reference's masks, the bus audit reference's tuples, one AND per tuple) word for word, for both machine
kinds; what the reference finds on fib(25) and mixed_ops:3; a captured machine whose answers are known in closed form; refusals; the device
kernels' very source under tools/hipemu; `check --links` on the command line; the C ABI's new symbols.  The reference of each input is computed
once per module and cut to the limits a test asks for (counts do not depend on them).  The figures pinned here are the reference's, not the
code under test's."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bus_audit_ref as bref
import link_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_pair_audit_cpu import Interaction, Vcol, VcolTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CPU, PROGRAM, MEM, ADD, SUB, MUL, DIV, SHIFT, LT, COM, BITWISE, OUTPUT, RANGE, STATIC_DATA = range(14)
GENERAL, MEMORY, RANGE_BUS = (1, 0), (1, 2), (1, 3)
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
        _reference[name] = ref.audit(machines["basic"], mt, prep)
    return ref.cut(_reference[name], **limits)


def both(machines, name, **limits):
    """The reference's report and the host audit's under both machine kinds: equal word for word."""
    want = reference(machines, name, **limits)
    mt, prep = witness(name)
    reps = {k: va.link_audit_host(m, mt, prep, **limits) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, want)
        assert np.array_equal(rep.words, ref.words(want))
    return want, reps["basic"]


def bus_of(rep, key):
    return next(b for b in rep.buses if tuple(b["bus"]) == key)


def open_of(want, chip):
    """{(interaction, field): (floating, open)} of the reference's dict."""
    return {(r["interaction"], j): (n, r["open"][j]) for r in want["chips"][chip]["records"] for j, n in enumerate(r["floating"]) if n}


def check_invariants(machines, name, rep):
    """What holds on every workload: floating is the field audit's count, open <= floating, the tuples are the bus audit reference's distinct
    padded tuples, a fully listed tuple's mask is the AND of its records' masks."""
    mt, prep = witness(name)
    fields = va.field_audit_host(machines["basic"], mt, prep, max_entries=1 << 20)
    for c, fc in zip(rep.chips, fields.chips):
        assert len(c["records"]) == len(fc["records"])
        for r, fr_ in zip(c["records"], fc["records"]):
            assert r["floating"] == fr_["floating"] and r["constant"] == fr_["constant"] and r["live_rows"] == fr_["live_rows"]
            assert all(o <= f for o, f in zip(r["open"], r["floating"]))
    prep_of = dict(prep)
    distinct = {}
    for chip in range(14):
        for it in machines["basic"].interactions(chip):
            bus = (int(it["global"]), int(it["bus"]))
            live = np.nonzero(bref.vcol(it["count"], mt[chip], prep_of.get(chip)))[0]
            width = bus_of(rep, bus)["width"]
            f = [tuple(int(bref.vcol(x, mt[chip], prep_of.get(chip))[r]) for x in it["fields"]) for r in live]
            distinct.setdefault(bus, set()).update(t + (0,) * (width - len(t)) for t in f)
    for b in rep.buses:
        assert b["tuples"] == len(distinct.get(tuple(b["bus"]), ())) and b["open_tuples"] <= b["tuples"]
        assert all(n <= b["open_tuples"] for n in b["open_in"]) and all(r >= n for n, r in zip(b["open_in"], b["open_records"]))
    for t in rep.tuples:
        assert t["mask"] != 0
        if len(t["records"]) == t["n_send"] + t["n_recv"]:
            m = 0xffffffff
            for r in t["records"]:
                m &= r[4]
            assert m == t["mask"]


# ---- 1. the host audit equals the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fib1", "fib25", "alu50", "mixed_ops"])
def test_host_equals_reference(machines, name):
    want, rep = both(machines, name, max_tuples=1 << 20, max_records_per_tuple=4096)
    assert not rep.truncated and rep.reported == rep.open_tuples == sum(b["open_tuples"] for b in rep.buses)
    check_invariants(machines, name, rep)
    want, rep = both(machines, name, max_tuples=3, max_records_per_tuple=2)
    assert rep.truncated == (rep.open_tuples > 3) and rep.reported == min(3, rep.open_tuples) and all(len(t["records"]) <= 2 for t in rep.tuples)
    both(machines, name)  # the defaults


def test_fib25_what_the_reference_finds(machines):
    """cpu's general send floats and is answered everywhere (add's receive pins every field); mem's receive is open (mem has no constraints)."""
    want, rep = both(machines, "fib25", max_tuples=1 << 20)
    g, m, r = bus_of(rep, GENERAL), bus_of(rep, MEMORY), bus_of(rep, RANGE_BUS)
    assert (g["width"], g["tuples"], g["open_tuples"]) == (14, 74, 0) and g["open_in"] == [0] * 14
    assert (m["width"], m["tuples"], m["open_tuples"]) == (8, 349, 349) and m["open_in"] == [0, 0, 349, 0, 345, 345, 345, 345]
    assert (r["tuples"], r["open_tuples"]) == (49, 49)
    for got in (open_of(want, CPU), rep.open(CPU)):
        assert all(got[(3, j)] == (105, 0) for j in range(13))
    for got in (open_of(want, MEM), rep.open(MEM)):
        assert got[(0, 2)] == (401, 401) and all(got[(0, j)] == (401, 0) for j in (0, 1, 3)) and all(got[(0, j)] == (401, 397) for j in (4, 5, 6, 7))
    assert rep.open(ADD) == {(k, 0): (105, 105) for k in range(4)}
    assert want["largest_group"] == 267  # more than one 256-record block of the device's join


def test_mixed_ops_what_the_reference_finds(machines):
    want, rep = both(machines, "mixed_ops", max_tuples=1 << 20)
    g = bus_of(rep, GENERAL)
    assert (g["tuples"], g["open_tuples"]) == (81, 66)
    for got in (open_of(want, DIV), rep.open(DIV)):
        assert got == {(0, j): (12, 12) for j in range(13)}
    assert open_of(want, CPU)[(3, 0)] == (58, 31) and open_of(want, CPU)[(3, 4)] == (58, 43)


# ---- 2. a captured machine with closed forms --------------------------------------------------------------------------------------------------
S0, L0, S1, T1, S2, H2, S3, L3, T3, N4, L4, S5, Q5, X6 = range(14)


def analytic_machine():
    """Fourteen captured AIRs of columns (a, b, on) (N4: (a, on)) on global bus 0, X6 on global bus 1; every count is `on`.
    S* send (a, b) and have no constraint; L* receive (a, b) and have none; T* receive with on (b - 2a) = 0; H2 receives with on (a - 7) = 0;
    N4 sends the one-field tuple (a); Q5 receives with b - a a = 0."""
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def var(air, col):
        return L.vgpu_air_variable(air, u(0), u(col), u(0))

    def vcol(terms, constant=0):
        t = (VcolTerm * max(1, len(terms)))(*[VcolTerm(0, c, wt) for c, wt in terms])
        return Vcol(t, len(terms), constant)

    def chip(name, width, send, bus=0, constraint=None):
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
        if constraint is not None:
            L.vgpu_air_assert_zero(air, u(constraint(air)))
        fields = [vcol([(c, 1)]) for c in range(width - 1)]
        f = (Vcol * len(fields))(*fields)
        it = Interaction(f, len(fields), vcol([(width - 1, 1)]), 1, bus, 1 if send else 0)
        assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)

    def t_rule(air):  # on (b - 2a)
        two_a = L.vgpu_air_mul(air, u(L.vgpu_air_constant(air, u(2))), u(var(air, 0)))
        return L.vgpu_air_mul(air, u(var(air, 2)), u(L.vgpu_air_sub(air, u(var(air, 1)), u(two_a))))

    def h_rule(air):  # on (a - 7)
        return L.vgpu_air_mul(air, u(var(air, 2)), u(L.vgpu_air_sub(air, u(var(air, 0)), u(L.vgpu_air_constant(air, u(7))))))

    def q_rule(air):  # b - a a
        return L.vgpu_air_sub(air, u(var(air, 1)), u(L.vgpu_air_mul(air, u(var(air, 0)), u(var(air, 0)))))

    chip(b"s0", 3, True)
    chip(b"l0", 3, False)
    chip(b"s1", 3, True)
    chip(b"t1", 3, False, constraint=t_rule)
    chip(b"s2", 3, True)
    chip(b"h2", 3, False, constraint=h_rule)
    chip(b"s3", 3, True)
    chip(b"l3", 3, False)
    chip(b"t3", 3, False, constraint=t_rule)
    chip(b"n4", 2, True)
    chip(b"l4", 3, False)
    chip(b"s5", 3, True)
    chip(b"q5", 3, False, constraint=q_rule)
    chip(b"x6", 3, True, bus=1)
    return va.Machine(m)


def analytic_traces(n):
    """Family A (100 + r, 200 + r): S0 (row 1 sends nothing) and L0.  B (300 + r, 600 + 2r): S1 and T1 (row 1 receives nothing), and X6 on bus
    1.  C (7, 400 + r): S2 and H2.  D (500 + r, 1000 + 2r): S3, L3 and T3.  E (600 + r [, 0]): N4 and L4.  F (a, a a), a = r mod 3: S5 and Q5."""
    r = np.arange(n, dtype=np.uint32)
    one, zero = np.ones(n, np.uint32), np.zeros(n, np.uint32)
    skip1 = np.where(r == 1, 0, 1).astype(np.uint32)
    A = lambda on: np.stack([100 + r, 200 + r, on], axis=1).astype(np.uint32)
    B = lambda on: np.stack([300 + r, 600 + 2 * r, on], axis=1).astype(np.uint32)
    C = np.stack([7 * one, 400 + r, one], axis=1).astype(np.uint32)
    D = np.stack([500 + r, 1000 + 2 * r, one], axis=1).astype(np.uint32)
    F = np.stack([r % 3, (r % 3) ** 2, one], axis=1).astype(np.uint32)
    return [A(skip1), A(one), B(one), B(skip1), C, C, D, D, D, np.stack([600 + r, one], axis=1).astype(np.uint32), np.stack([600 + r, zero, one], axis=1).astype(np.uint32), F, F, B(one)]


def check_analytic(rep, n):
    """The closed forms at height n."""
    gap = 1 if n >= 2 else 0   # row 1 exists: S0 sends nothing there, T1 receives nothing there
    zeros = (n + 2) // 3       # rows with a = 0 in family F
    b0, b1 = rep.buses
    assert (tuple(b0["bus"]), b0["width"], tuple(b1["bus"]), b1["width"]) == ((1, 0), 2, (1, 1), 2)
    assert b0["live"] == 13 * n - 2 * gap and b0["tuples"] == 5 * n + min(n, 3)
    # open: A everywhere (0b11), B where T1 is silent (0b11), C (0b10: H2 pins a), E (0b01: the padding pins position 1), F's tuple (0, 0) (0b01)
    assert b0["open_tuples"] == n + gap + n + n + 1
    assert b0["open_in"] == [n + gap + n + 1, n + gap + n]
    assert b0["open_records"] == [(2 * n - gap) + gap + 2 * n + 2 * zeros, (2 * n - gap) + gap + 2 * n]
    assert (b1["live"], b1["tuples"], b1["open_tuples"], b1["open_in"], b1["open_records"]) == (n, n, n, [n, n], [n, n])  # the same tuples on bus 1 do not join
    both_ = lambda fl, op: {(0, 0): (fl, op), (0, 1): (fl, op)}
    assert rep.open(S0) == both_(n - gap, n - gap) and rep.open(L0) == both_(n, n)
    assert rep.open(S1) == both_(n, gap) and rep.open(T1) == {}                     # anchored: T1 pins both positions
    assert rep.open(S2) == {(0, 0): (n, 0), (0, 1): (n, n)} and rep.open(H2) == {(0, 1): (n, n)}
    assert rep.open(S3) == both_(n, 0) and rep.open(L3) == both_(n, 0) and rep.open(T3) == {}  # anchored although L3 floats
    assert rep.open(N4) == {(0, 0): (n, n)} and rep.open(L4) == {(0, 0): (n, n), (0, 1): (n, 0)}
    assert rep.open(S5) == {(0, 0): (n, zeros), (0, 1): (n, 0)} and rep.open(Q5) == {(0, 0): (zeros, zeros)}
    assert rep.open(X6) == both_(n, n)
    assert rep.open_tuples == b0["open_tuples"] + n == rep.reported and not rep.truncated
    by = {(tuple(t["bus"]), tuple(t["fields"])): t for t in rep.tuples}
    assert by[((1, 0), (100, 200))]["mask"] == 0b11 and by[((1, 0), (7, 400))]["mask"] == 0b10 and by[((1, 0), (600, 0))]["mask"] == 0b01
    assert by[((1, 0), (0, 0))]["mask"] == 0b01 and (by[((1, 0), (0, 0))]["n_send"], by[((1, 0), (0, 0))]["n_recv"]) == (zeros, zeros)
    assert ((1, 0), (300, 600)) not in by and ((1, 0), (500, 1000)) not in by and by[((1, 1), (300, 600))]["mask"] == 0b11
    if n >= 2:
        assert by[((1, 0), (101, 201))]["records"] == [(L0, 1, 0, 0, 0b11)] and by[((1, 0), (301, 602))]["records"] == [(S1, 1, 0, 1, 0b11)]
        assert ((1, 0), (1, 1)) not in by
    firsts = [t["records"][0][:3] for t in rep.tuples]
    assert firsts == sorted(firsts)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_machine(n):
    rep = va.link_audit_host(analytic_machine(), analytic_traces(n), [], max_tuples=1 << 10, max_records_per_tuple=16)
    check_analytic(rep, n)


# ---- 3. refusals and options ------------------------------------------------------------------------------------------------------------------
def wide_machine(fields):
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    air = ctypes.c_void_p()
    assert L.vgpu_air_new(b"wide", u(fields), u(0), ctypes.byref(air)) == 0
    terms = [(VcolTerm * 1)(VcolTerm(0, c, 1)) for c in range(fields)]
    f = (Vcol * fields)(*[Vcol(t, 1, 0) for t in terms])
    it = Interaction(f, fields, Vcol((VcolTerm * 1)(), 0, 1), 1, 0, 1)
    assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
    assert L.vgpu_machine_push_air(m, air) == 0
    L.vgpu_air_free(air)
    return va.Machine(m)


def _host_raw(machine, mt, opts):
    """vgpu_link_audit_host with a raw options pointer (None: NULL); (status, words)."""
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt]
    n = len(mains)
    h = ctypes.c_void_p()
    rc = L.vgpu_link_audit_host(machine._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * 1)(), (ctypes.c_void_p * 1)(), (ctypes.c_uint64 * 1)(),
                                (ctypes.c_uint64 * 1)(), ctypes.c_uint32(0), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
    return rc, (va._link_report(h).words if rc == 0 else None)


def test_a_bus_of_33_fields_is_refused():
    rep = va.link_audit_host(wide_machine(32), [np.arange(64, dtype=np.uint32).reshape(2, 32)], [])
    assert rep.buses[0]["width"] == 32 and rep.open_tuples == 2 and [t["mask"] for t in rep.tuples] == [0xffffffff] * 2
    with pytest.raises(va.VgpuError, match=r"link_audit: bus \(1, 0\) is 33 fields wide.*at most 32 fields \(33 - 32 = 1 too many\)") as e:
        va.link_audit_host(wide_machine(33), [np.arange(66, dtype=np.uint32).reshape(2, 33)], [])
    assert e.value.code == -1


def test_bad_shapes_and_options():
    machine, mt = analytic_machine(), analytic_traces(8)
    want = va.link_audit_host(machine, mt, []).words
    rc, words = _host_raw(machine, mt, None)  # NULL opts: the defaults
    assert rc == 0 and np.array_equal(words, want)
    rc, words = _host_raw(machine, mt, va.LinkAuditOpts(0, 0, 0, 0))  # zero fields select the defaults 64, 4, 64
    assert rc == 0 and np.array_equal(words, want) and np.array_equal(va.link_audit_host(machine, mt, [], 64, 4, 64).words, want)
    for bad in (va.LinkAuditOpts(0, 0, 0, 1), va.LinkAuditOpts(0, 0, 65, 0), va.LinkAuditOpts((1 << 24) + 1, 0, 0, 0), va.LinkAuditOpts(0, 4097, 0, 0)):
        rc, _ = _host_raw(machine, mt, bad)
        assert rc == -1 and b"link_audit" in va.lib().vgpu_last_error()
    with pytest.raises(va.VgpuError, match="link_audit: max_tuples and max_records_per_tuple must be at least 1"):
        va.link_audit_host(machine, mt, [], max_tuples=0)
    with pytest.raises(va.VgpuError, match="link_audit: hash_bits must be 1..64"):
        va.link_audit_host(machine, mt, [], hash_bits=65)
    with pytest.raises(va.VgpuError, match="link_audit: .*one main trace per chip"):
        va.link_audit_host(machine, mt[:-1], [])
    with pytest.raises(va.VgpuError, match="link_audit: trace heights must be powers of two"):
        va.link_audit_host(machine, [m[:3] for m in mt], [])
    with pytest.raises(va.VgpuError, match="link_audit: trace width mismatch"):
        va.link_audit_host(machine, [m[:, :2] for m in mt], [])
    with pytest.raises(va.VgpuError, match="two-dimensional"):
        va.link_audit_host(machine, [m.ravel() for m in mt], [])
    with pytest.raises(ValueError, match="not a link report image"):
        va.LinkReport(va.bus_audit_host(machine, mt, []).words)
    assert np.array_equal(va.link_audit_host(machine, mt, []).words, want)  # the same words run after run


def test_hash_bits_do_not_change_the_host_report(machines):
    mt, prep = witness("fib25")
    want = va.link_audit_host(machines["basic"], mt, prep).words
    for bits in (8, 16):
        assert np.array_equal(va.link_audit_host(machines["basic"], mt, prep, hash_bits=bits).words, want)


# ---- 4. the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "link_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "liblinkauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp")] + [os.path.join(csrc, "host", f) for f in ("link_audit.hpp", "field_audit.hpp", "bus_audit.hpp", "rank_audit.hpp", "mutation_audit.hpp",
                                                                                                   "constraint_audit.hpp", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("link_audit.hip", "bus_audit.hip", "field_elim.hpp", "bus_records.hpp", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_link_audit.restype = ctypes.c_int64
    return L


def emulated(emu, mt, prep, interpret, hash_bits, rows_per_workgroup=0, max_tuples=64, max_records_per_tuple=4):
    """[(exact path ran, words)] per entry of hash_bits."""
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    out = np.zeros(1 << 20, np.uint32)
    got = emu.emu_link_audit(
        (ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
        ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
        (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k), ctypes.c_uint32(interpret),
        ctypes.c_uint32(rows_per_workgroup), ctypes.c_uint32(max_tuples), ctypes.c_uint32(max_records_per_tuple), (ctypes.c_uint32 * len(hash_bits))(*hash_bits),
        ctypes.c_uint32(len(hash_bits)), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert got > 0
    res, at = [], 0
    for _ in hash_bits:
        size = int(out[at + 2])
        res.append((bool(out[at]), out[at + 1:at + 1 + size].copy()))
        at += 1 + size
    assert at == got
    return res


@pytest.mark.parametrize("interpret", [0, 1], ids=["native", "interpreted"])
@pytest.mark.parametrize("name", ["fib25", "mixed_ops"])
def test_kernel_source_under_emulation(machines, emu, name, interpret):
    """link_audit.hip's kernels with the elimination's wave primitives in their emulation forms, driven as Prover::link_audit drives them: the
    mask pass for the compiled chip templates, the interpreted dual register programs and the bus-only chips with 3 rows per workgroup (the
    r - 1 halo, the wrap between row 0 and row n - 1 and the reuse of a bus-only chip's masks cross workgroup boundaries), the bus audit's
    records / groups / reduce, join and tally over several 256-record blocks (fib(25): 1481 live records, a tuple of 267), select and report;
    with 64 key bits and with 8, where keys collide and the exact path groups by the full tuples.  The assembled report is the host audit's,
    word for word.  NOT covered here: the hardware's own ballot, wave barrier and atomics between workgroups, the radix sort's
    scatter, the opt-in to more than 64 KB of LDS, and the launch shapes of tall traces; tests/test_link_audit_gpu.py covers those."""
    mt, prep = witness(name)
    host = va.link_audit_host(machines["basic"], mt, prep, max_tuples=40, max_records_per_tuple=5)
    assert host.truncated and sum(b["live"] for b in host.buses) > 512
    (exact64, w64), (exact8, w8) = emulated(emu, mt, prep, interpret, [64, 8], rows_per_workgroup=3, max_tuples=40, max_records_per_tuple=5)
    assert not exact64 and exact8
    assert np.array_equal(w64, host.words) and np.array_equal(w8, host.words)


# ---- 5. command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_links_on_the_host(tmp_path, machines):
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    plain = _cli("check", bl, out, "--host")
    plain_json = json.loads(out.read_text())
    assert "links" not in plain_json
    r = _cli("check", bl, out, "--host", "--links", "--max-tuples", 5, "--max-records", 2)
    assert r.returncode == plain.returncode == 0, r.stderr  # an open position is not a fault of the witness
    lines, before = r.stdout.strip().split("\n"), plain.stdout.strip().split("\n")
    assert lines[:len(before)] == before
    w = va.Workload.from_executable(vp.machine_code(vp.byte_loads_program()))
    rep = va.link_audit_host(machines["basic"], w.main_traces(), w.preprocessed(), max_tuples=5, max_records_per_tuple=2)
    n_bus = sum(1 for b in rep.buses if b["open_tuples"])
    n_rec = sum(1 for c in rep.chips for r_ in c["records"] if any(r_["open"]))
    assert n_bus and n_rec and len(lines) == len(before) + n_bus + n_rec
    m = bus_of(rep, MEMORY)
    assert "memory bus: %d of %d tuples open; open positions 2, 4-7" % (m["open_tuples"], m["tuples"]) in lines
    rec = rep.chips[MEM]["records"][0]
    assert "mem: interaction 0 (receives on the memory bus): fields 2, 4-7 open on %d of %d floating rows" % (max(rec["open"]), max(rec["floating"])) in lines
    j = json.loads(out.read_text())
    assert set(j) == set(plain_json) | {"links"} and {k: v for k, v in j.items() if k not in ("links", "host_ms")} == {k: v for k, v in plain_json.items() if k != "host_ms"}
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in j["links"].items() if k not in timing} == json.loads(json.dumps({k: v for k, v in rep.to_dict().items() if k not in timing}))
    assert j["links"]["truncated"] and j["links"]["reported"] == 5
    help_text = _cli("check", "--help").stdout
    assert "--links" in help_text and "judged alone" in help_text and "multiplicities" in help_text and "does not depend on this flag" in help_text


# ---- 6. C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_symbols():
    names = ["vgpu_link_audit", "vgpu_link_audit_host", "vgpu_link_report_len", "vgpu_link_report_words", "vgpu_link_report_timing", "vgpu_link_report_free"]
    lib = os.path.join(ROOT, "valida_amd", "libvgpu.so")
    exported = set(line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "vgpu.h")) as f:
        header = f.read()
    for n in names:
        assert n in exported and re.search(r"\b%s\(" % n, header), n
    assert "Link audit" in header and "VLA1" in header and "judged alone" in header and "multiplicities" in header
