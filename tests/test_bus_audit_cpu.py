"""The bus audit without a GPU: the host implementation of the contract (vgpu_bus_audit_host) against the independent numpy restatement of
tests/bus_audit_ref.py on every input of the issue's table, for both machine kinds; truncation; the zero-padding rule; argument validation; the
device kernels' very source under tools/hipemu; the `check` action of the command line.  The literals pinned here were produced by a prototype
of the reference, not by the code under test."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bus_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
GENERAL, MEMORY, RANGE = (1, 0), (1, 2), (1, 3)
CPU, MEM, ADD, OUTPUT, RANGE_CHIP = 0, 2, 3, 11, 12


def exe(prog, advice=b""):
    return va.Workload.from_executable(vp.machine_code(prog), advice=advice)


def witness(w, faults=()):
    mt, prep = w.main_traces(), w.preprocessed()
    for chip, row, col in faults:
        mt[chip][row, col] = (int(mt[chip][row, col]) + 1) % P
    return mt, prep


BALANCED = {
    "fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "static_data": lambda: va.Workload.named("static_data"),
    "signed_inequality": lambda: va.Workload.named("signed_inequality"), "byte_loads": lambda: exe(vp.byte_loads_program()),
    "advice": lambda: exe(vp.advice_program(5), b"\x01\x80\xff"), "byte_loop50": lambda: exe(vp.byte_loop_program(50), bytes(range(30))),
    "fib9359": lambda: va.Workload.fib(9359), "fib37446": lambda: va.Workload.fib(37446),
}
C2_FAULTS = ((RANGE_CHIP, 7, 0), (MEM, 12345, 4))


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def both(machines, mt, prep, **kw):
    """The reference's answer (it is the same for both machine kinds: checked on mixed_ops) and the host audit's under both."""
    r = ref.audit(machines["basic"], mt, prep)
    reps = {k: va.bus_audit_host(m, mt, prep, **kw) for k, m in machines.items()}
    for rep in reps.values():
        ref.assert_report_equals(rep, r, kw.get("max_tuples", 64), kw.get("max_records_per_tuple", 4))
    assert np.array_equal(reps["basic"].words, reps["ffi"].words)
    return r, reps["basic"]


@pytest.mark.parametrize("name", list(BALANCED))
def test_balanced_witnesses(machines, name):
    w = BALANCED[name]()
    if name == "fib9359":
        assert w.cpu_height == 1 << 16
    if name == "fib37446":
        assert w.cpu_height == 1 << 18
    r, rep = both(machines, *witness(w))
    assert r["total_unbalanced"] == 0 and rep.balanced and rep.total_unbalanced == 0 and not rep.truncated and rep.tuples == []
    assert [b["bus"] for b in rep.buses] == [GENERAL, MEMORY, RANGE] and [b["width"] for b in rep.buses] == [14, 8, 1]


def test_zero_padding_rule(machines, fib25):
    """The cpu chip sends 14 fields on the general bus (the last is clk_or_zero), the add chip receives 13: equal only after zero-padding."""
    its = {c: machines["basic"].interactions(c) for c in (CPU, ADD)}
    assert max(len(i["fields"]) for i in its[CPU] if i["send"] and (i["global"], i["bus"]) == (True, 0)) == 14
    assert [len(i["fields"]) for i in its[ADD] if not i["send"] and (i["global"], i["bus"]) == (True, 0)] == [13]
    mt, prep = witness(fib25)
    assert va.bus_audit_host(machines["basic"], mt, prep).balanced
    # and the padding is not a blanket excuse: a non-zero last field on the cpu side (clk_or_zero, column 50) of an add row unbalances it
    row = int(np.nonzero(mt[CPU][:, 3] == 100)[0][0])
    mt[CPU][row, 50] = 5
    rep = va.bus_audit_host(machines["basic"], mt, prep)
    assert rep.total_unbalanced == 2 and [t["bus"] for t in rep.tuples] == [GENERAL, GENERAL]
    assert rep.tuples[0]["fields"][13] == 5 and rep.tuples[0]["net_signed"] == 1 and rep.tuples[1]["fields"][13] == 0 and rep.tuples[1]["net_signed"] == -1


def test_fault_in_the_range_trace(machines, fib25):
    r, rep = both(machines, *witness(fib25, [(RANGE_CHIP, 7, 0)]), max_tuples=64, max_records_per_tuple=1000)
    assert rep.total_unbalanced == 1
    (t,) = rep.tuples
    assert t["bus"] == RANGE and t["fields"] == [7] and t["net_signed"] == -1 and t["net"] == P - 1
    assert all(rec[0] == ADD and rec[3] == 1 for rec in t["records"][:-1]) and t["records"][-1][:4] == (RANGE_CHIP, 7, 0, 0)
    assert t["n_recv"] == 1 and t["n_send"] == len(t["records"]) - 1 and t["recv_sum"] == (t["send_sum"] + 1) % P


def test_fault_in_the_add_trace(machines, fib25):
    r, rep = both(machines, *witness(fib25, [(ADD, 5, 11)]))
    assert rep.total_unbalanced == 4 and sorted(t["bus"] for t in rep.tuples) == [GENERAL, GENERAL, RANGE, RANGE]


def test_store_byte(machines):
    w = exe(vp.store_byte_program())
    mt, prep = witness(w)
    r, rep = both(machines, mt, prep)
    assert rep.total_unbalanced == 5 and not rep.balanced
    assert [t["bus"] for t in rep.tuples] == [MEMORY] * 5 and [t["net_signed"] for t in rep.tuples] == [-1] * 5
    assert [t["records"] for t in rep.tuples] == [[(MEM, row, 0, 0, 1)] for row in range(15, 20)]
    assert [t["fields"][0] for t in rep.tuples] == [1] * 5 and [t["fields"][1] for t in rep.tuples] == [4, 6, 8, 10, 13]  # is_read, clk
    assert [int(mt[CPU][clk, 3]) for clk in (4, 6, 8, 10, 13)] == [vp.STOREU8] * 5


def test_echo(machines):
    r, rep = both(machines, *witness(exe(vp.echo_program(3), b"abc")))
    assert rep.total_unbalanced == 6 and [t["bus"] for t in rep.tuples] == [GENERAL] * 6
    for k, t in enumerate(rep.tuples[:3]):
        assert t["fields"] == [300, 0, 0, 0, 97 + k] + [0] * 9 and t["net_signed"] == 1 and t["records"][0][:2] == (CPU, 1 + 2 * k) and t["records"][0][3] == 1
    for k, t in enumerate(rep.tuples[3:]):
        assert t["fields"] == [0, 0, 0, 0, 97 + k] + [0] * 8 + [1 + 2 * k] and t["net_signed"] == -1 and t["records"][0][:2] == (OUTPUT, k) and t["records"][0][3] == 0


@pytest.mark.parametrize("name,total,general,range_,largest", [("mixed_ops:40", 640, 406, 234, 127), ("mixed_ops:700", 6917, 6661, 256, 1697)])
def test_mixed_ops(machines, name, total, general, range_, largest):
    r, rep = both(machines, *witness(va.Workload.named(name)), max_tuples=10000)
    assert rep.total_unbalanced == total == rep.reported and not rep.truncated
    per = {b["bus"]: b["unbalanced"] for b in rep.buses}
    assert per == {GENERAL: general, MEMORY: 0, RANGE: range_}
    assert max(len(t["records"]) for t in r["tuples"]) == largest == max(t["n_send"] + t["n_recv"] for t in rep.tuples)


@pytest.fixture(scope="module")
def mixed700(machines):
    mt, prep = witness(va.Workload.named("mixed_ops:700"))
    return mt, prep, ref.audit(machines["basic"], mt, prep)


@pytest.mark.parametrize("max_tuples", [1, 64, 10000])
@pytest.mark.parametrize("max_records", [1, 4])
def test_truncation(machines, mixed700, max_tuples, max_records):
    mt, prep, r = mixed700
    rep = va.bus_audit_host(machines["basic"], mt, prep, max_tuples=max_tuples, max_records_per_tuple=max_records)
    ref.assert_report_equals(rep, r, max_tuples, max_records)
    assert rep.total_unbalanced == 6917 and rep.reported == min(max_tuples, 6917) and rep.truncated == (max_tuples < 6917)
    assert all(len(t["records"]) <= max_records for t in rep.tuples)
    full = va.bus_audit_host(machines["basic"], mt, prep, max_tuples=10000, max_records_per_tuple=4)
    assert [dict(t, records=t["records"][:max_records]) for t in full.tuples[:max_tuples]] == rep.tuples


def test_full_size_c2(machines):
    """C2 (2^20 cpu rows, 2^22 memory rows): balanced, 8 089 214 live records of 13 632 781 pairs; with two faults, three tuples in this order."""
    w = va.Workload.fib(149794)
    assert w.cpu_height == 1 << 20
    mt, prep = witness(w)
    assert mt[MEM].shape[0] == 1 << 22
    rep = va.bus_audit_host(machines["basic"], mt, prep)
    assert rep.balanced and sum(b["live"] for b in rep.buses) == 8089214
    assert {b["bus"]: b["live"] for b in rep.buses} == {GENERAL: 1198362, MEMORY: 4493872, RANGE: 2396980}
    for chip, row, col in C2_FAULTS:
        mt[chip][row, col] += 1
    r, rep = both(machines, mt, prep)
    assert r["pairs"] == 13632781 and r["live"] == 8089214
    assert rep.total_unbalanced == 3
    a, b, c = rep.tuples
    assert (a["bus"], a["fields"], a["net_signed"], a["records"]) == (MEMORY, [1, 43217, 4048, 0, 215, 242, 210, 40], 1, [(CPU, 43217, 0, 1, 1)])
    assert (b["bus"], b["fields"], b["net_signed"], b["records"]) == (MEMORY, [1, 43217, 4048, 0, 215, 242, 210, 41], -1, [(MEM, 12345, 0, 0, 1)])
    assert (c["bus"], c["fields"], c["net_signed"]) == (RANGE, [7], -1) and [rec[:2] for rec in c["records"]] == [(ADD, 29), (ADD, 110), (ADD, 112), (ADD, 115)]


# ---- argument validation -----------------------------------------------------------------------------------------------------------------
def test_argument_validation(machines, fib25):
    m = machines["basic"]
    mt, prep = witness(fib25)

    def refused(match, main=mt, pre=prep, **kw):
        with pytest.raises(va.VgpuError, match=match) as e:
            va.bus_audit_host(m, main, pre, **kw)
        assert e.value.code == -1  # VGPU_ERR_INVALID_ARG

    refused("one main trace per chip", main=mt[:-1])
    refused("width mismatch for chip add", main=mt[:ADD] + [mt[ADD][:, :-1]] + mt[ADD + 1:])
    refused("powers of two", main=mt[:ADD] + [mt[ADD][:-1]] + mt[ADD + 1:])
    refused("chip add has no preprocessed columns", pre=prep + [(ADD, mt[ADD])])
    refused("needs its preprocessed trace", pre=prep[:1])
    refused("repeated preprocessed chip", pre=prep + prep[:1])
    refused("preprocessed trace shape mismatch", pre=[prep[0], (prep[1][0], prep[1][1][:128])])
    refused("hash_bits", hash_bits=0)
    refused("hash_bits", hash_bits=65)
    refused("max_tuples", max_tuples=0)
    # the C entry point itself: hash_bits beyond 64 and null arguments are refused with a code and a message, a zeroed struct means the defaults
    opts = va.BusAuditOpts(0, 0, 65)
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[x.ctypes.data for x in mt])
    hs, ws = (ctypes.c_uint64 * 14)(*[x.shape[0] for x in mt]), (ctypes.c_uint64 * 14)(*[x.shape[1] for x in mt])
    pa = (ctypes.c_void_p * 2)(*[x.ctypes.data for _, x in prep])
    ph, pw = (ctypes.c_uint64 * 2)(*[x.shape[0] for _, x in prep]), (ctypes.c_uint64 * 2)(*[x.shape[1] for _, x in prep])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in prep])
    L = va.lib()
    assert L.vgpu_bus_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, ctypes.byref(opts), ctypes.byref(h)) == -1 and b"hash_bits" in L.vgpu_last_error()
    assert L.vgpu_bus_audit_host(m._h, None, hs, ws, 14, chips, pa, ph, pw, 2, None, ctypes.byref(h)) == -1 and b"null" in L.vgpu_last_error()
    assert L.vgpu_bus_audit_host(m._h, arr, hs, ws, 14, chips, pa, ph, pw, 2, ctypes.byref(va.BusAuditOpts(0, 0, 0)), ctypes.byref(h)) == 0
    L.vgpu_bus_report_len.restype = ctypes.c_uint64
    L.vgpu_bus_report_len.argtypes = L.vgpu_bus_report_free.argtypes = [ctypes.c_void_p]
    assert L.vgpu_bus_report_len(h) == 8 + 3 * 12
    L.vgpu_bus_report_free(h)


def test_report_image_and_json(machines):
    mt, prep = witness(exe(vp.store_byte_program()))
    rep = va.bus_audit_host(machines["basic"], mt, prep)
    w = [int(x) for x in rep.words]
    assert w[0] == 0x31524256 and w[1] == len(w) and w[2:8] == [0, 0, 5, 0, 5, 3]
    again = va.BusReport(rep.words)
    assert again.tuples == rep.tuples and again.buses == rep.buses
    j = json.loads(rep.to_json())
    assert j["total_unbalanced"] == 5 and not j["balanced"] and [t["fields"][1] for t in j["tuples"]] == [4, 6, 8, 10, 13] and j["device_ms"] == 0.0
    assert np.array_equal(va.bus_audit_host(machines["basic"], mt, prep).words, rep.words)  # the same words run after run


# ---- the device kernels' source under emulation ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "bus_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libbusauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "host", "bus_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
        os.path.join(csrc, "kernels", f) for f in ("bus_audit.hip", "interactions.hpp", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_bus_records.restype = L.emu_bus_audit.restype = ctypes.c_int64
    return L


def emu_args(mt, prep):
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in mt] + [np.ascontiguousarray(m, dtype=np.uint32) for _, m in prep]
    n, k = len(mt), len(prep)
    args = [(ctypes.c_void_p * n)(*[m.ctypes.data for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in keep[:n]]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in keep[:n]]),
            ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in prep]), (ctypes.c_void_p * k)(*[m.ctypes.data for m in keep[n:]]),
            (ctypes.c_uint64 * k)(*[m.shape[0] for m in keep[n:]]), (ctypes.c_uint64 * k)(*[m.shape[1] for m in keep[n:]]), ctypes.c_uint32(k)]
    return args, keep


EMU_INPUTS = {"store_byte": lambda: exe(vp.store_byte_program()), "mixed_ops:40": lambda: va.Workload.named("mixed_ops:40")}


@pytest.mark.parametrize("name", list(EMU_INPUTS))
def test_record_kernel_source_under_emulation(emu, machines, name):
    """k_ba_records (and the tuple recomputation the report and the exact path use) give the multiset of (bus, padded tuple, signed count, record id)
    that the reference lists, and equal keys whenever (bus, padded tuple) are equal — the ALU chips' 13-field receives against cpu's 14-field sends included."""
    m = machines["basic"]
    mt, prep = witness(EMU_INPUTS[name]())
    args, keep = emu_args(mt, prep)
    pairs = sum(mt[c].shape[0] * len(m.interactions(c)) for c in range(14))
    keys, counts, wmax = np.zeros(pairs, np.uint64), np.zeros(pairs, np.uint32), ctypes.c_uint32()
    tuples = np.zeros((pairs, 6 + 14), np.uint32)
    n = emu.emu_bus_records(*args, ctypes.c_uint32(64), ctypes.c_uint64(pairs), keys.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p),
                            tuples.ctypes.data_as(ctypes.c_void_p), ctypes.byref(wmax))
    assert n == pairs and wmax.value == 14
    # the reference's records, straight from the interaction image
    want = {}
    prep_of = dict(prep)
    slot = 0
    first = []
    for c in range(14):
        first.append(slot)
        slot += mt[c].shape[0] * len(m.interactions(c))
    for c in range(14):
        its = m.interactions(c)
        for k, it in enumerate(its):
            cnt = ref.vcol(it["count"], mt[c], prep_of.get(c))
            f = [ref.vcol(x, mt[c], prep_of.get(c)) for x in it["fields"]]
            for row in np.nonzero(cnt)[0]:
                fields = [int(x[row]) for x in f] + [0] * (14 - len(f))
                want[first[c] + int(row) * len(its) + k] = (c, int(row), k, int(it["send"]), int(it["global"]), int(it["bus"]), fields, int(cnt[row]))
    live = np.nonzero(counts)[0]
    assert sorted(want) == live.tolist() and np.all(keys[counts == 0] == np.uint64(0xFFFFFFFFFFFFFFFF))
    key_of = {}
    saw_13_against_14 = False
    for s in live:
        c, row, k, snd, glob, bus, fields, cnt = want[int(s)]
        assert tuples[s].tolist() == [c, row, k, snd, glob, bus] + fields and int(counts[s]) == cnt
        ident = (glob, bus, tuple(fields))
        if ident in key_of:
            assert key_of[ident][0] == int(keys[s])
            saw_13_against_14 |= (glob, bus) == GENERAL and {key_of[ident][1], len(m.interactions(c)[k]["fields"])} == {13, 14}
        else:
            key_of[ident] = (int(keys[s]), len(m.interactions(c)[k]["fields"]))
    assert len(set(v[0] for v in key_of.values())) == len(key_of)  # 64 key bits: no collision among a few thousand tuples
    assert saw_13_against_14  # both programs add: the add chip's 13-field receive met the cpu chip's 14-field send under one key


@pytest.mark.parametrize("name", list(EMU_INPUTS))
@pytest.mark.parametrize("hash_bits", [64, 8])
def test_group_reduction_and_report_under_emulation(emu, machines, name, hash_bits):
    """Heads, the group scan, the LDS-then-atomics reduction, the collision check and the exact path, selection and the report rows — the device
    source with the radix sort's scatter replaced by a host sort (tests/emu/bus_audit_emu.cpp says why) — against the reference."""
    m = machines["basic"]
    mt, prep = witness(EMU_INPUTS[name]())
    r = ref.audit(m, mt, prep)
    args, keep = emu_args(mt, prep)
    R, T = 4, 10000
    out = np.zeros(7 + 3 + T * (8 + 14 + 2 * R), np.uint32)
    n = emu.emu_bus_audit(*args, ctypes.c_uint32(hash_bits), ctypes.c_uint32(T), ctypes.c_uint32(R), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.size))
    assert n > 0
    live, groups, collided, n_unb, n_rep, stride, exact = (int(x) for x in out[:7])
    assert live == r["live"] and n_unb == r["total_unbalanced"] == n_rep and stride == 8 + 14 + 2 * R
    assert exact == (hash_bits == 8) and (collided > 0) == (hash_bits == 8)
    assert out[7:10].tolist() == [b["unbalanced"] for b in r["buses"]]
    buses = [b["bus"] for b in r["buses"]]
    first = np.cumsum([0] + [mt[c].shape[0] * len(m.interactions(c)) for c in range(14)])
    for t, want in enumerate(r["tuples"]):
        e = out[10 + t * stride:10 + (t + 1) * stride].tolist()
        assert buses[e[0]] == want["bus"] and e[8:8 + len(want["fields"])] == want["fields"] and not any(e[8 + len(want["fields"]):22])
        assert (e[2] | (e[3] << 32)) % P == want["send_sum"] and (e[4] | (e[5] << 32)) % P == want["recv_sum"] and e[6:8] == [want["n_send"], want["n_recv"]]
        assert e[1] == min(R, len(want["records"]))
        for k, (c, row, inter, snd, cnt) in enumerate(want["records"][:R]):
            assert e[22 + 2 * k:24 + 2 * k] == [int(first[c]) + row * len(m.interactions(c)) + inter, cnt]


# ---- command line --------------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_on_the_host(tmp_path, machines):
    sb, bl, out = tmp_path / "store_byte.bin", tmp_path / "byte_loads.bin", tmp_path / "report.json"
    sb.write_bytes(vp.machine_code(vp.store_byte_program()))
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    r = _cli("check", sb, out, "--host")
    assert r.returncode == 1, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 6 and lines[-1].startswith("unbalanced: 5 tuples")
    for line, clk in zip(lines, (4, 6, 8, 10, 13)):
        assert line.startswith("memory bus [1, %d, " % clk) and line.endswith("cycle %d: pc %d STOREU8" % (clk, clk)) and "mem row" in line and "net -1" in line
    want = ref.audit(machines["basic"], *witness(exe(vp.store_byte_program())))
    j = json.loads(out.read_text())
    assert j["total_unbalanced"] == 5 and not j["balanced"] and not j["truncated"]
    assert [dict(t, bus=tuple(t["bus"]), records=[tuple(x) for x in t["records"]]) for t in j["tuples"]] == want["tuples"]
    assert [dict(b, bus=tuple(b["bus"])) for b in j["buses"]] == want["buses"]
    r = _cli("check", bl, out, "--host")
    assert r.returncode == 0 and r.stdout.startswith("balanced: ") and json.loads(out.read_text())["balanced"]
    r = _cli("check", tmp_path / "missing.bin", out, "--host")
    assert r.returncode == 1 and r.stderr.startswith("check: ")


def test_cli_check_without_a_gpu_fails_with_a_message(tmp_path):
    import conftest

    if conftest.has_gpu():
        pytest.skip("this box has a GPU (tests/test_bus_audit_gpu.py checks through the CLI on the device)")
    bl, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    bl.write_bytes(vp.machine_code(vp.byte_loads_program()))
    r = _cli("check", bl, out)
    assert r.returncode == 1 and r.stderr.startswith("check: ") and not out.exists()
