"""The arithmetic audit without a GPU: the host twin (vgpu_arithmetic_audit_host) against the numpy and plain-integer reference of
tests/arithmetic_audit_ref.py word for word on the VM witnesses under both machine kinds; the per-opcode and soft counts pinned by the reference
and by a recount from the operation logs; the planted quotient; one test per kind and reason; the edge corpus on the captured `alu` machine;
limits, null options and refusals; the command line; the host twin under AddressSanitizer and UBSan as a stand-alone program; the device
kernels' very source under tools/hipemu."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import arithmetic_audit_cases as cases
import arithmetic_audit_ref as ref
import valida_amd as va
import valida_programs as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
# name -> (live, judged, other, the non-zero opcode counts, soft, mulhs_sign_matters) of the receives: written down once the reference's report and
# the recount from the operation logs agreed
PINNED = {"fib25": (105, 105, 0, {"ADD32": 105}, 0, 0),
          "fib582": (2333, 2333, 0, {"ADD32": 2333}, 0, 0),
          "alu100": (800, 800, 0, {"ADD32": 300, "SUB32": 100, "LT32": 100, "AND32": 100, "OR32": 100, "XOR32": 100}, 0, 0),
          "signed_inequality": (16, 16, 0, {"LT32": 7, "LTE32": 1, "SLT32": 7, "SLE32": 1}, 0, 0),
          "left_imm_ops": (10, 10, 0, {"LT32": 5, "LTE32": 5}, 0, 0)}


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def held(machine, main, prep, **kw):
    """The host report, held to the reference word for word."""
    host = va.arithmetic_audit_host(machine, main, prep, **kw)
    sides = va.ARITHMETIC_SIDES[kw.get("sides", "receives")]
    bus = kw.get("bus")
    want = ref.words(ref.audit(machine, main, prep, max_findings=kw.get("max_findings", 64), bus=(True, 0) if bus is None else bus, sides=sides))
    assert np.array_equal(host.words, want), (host.counters, host.hard[:2], host.soft[:2])
    assert host.device_ms == 0 and host.evaluations == host.counters["live"]
    return host


def on_alu(trace, kind="alu", **kw):
    traces = [trace] * (2 if kind == "alu_pair" else 1)
    return held(cases.machine(kind), traces, [], **kw)


def oplog_recount(w):
    """From Workload.oplog() in plain integers: the operations by opcode over the eight ALU logs (one row of a receiving chip each), the SHR-logged
    shifts that hold the arithmetic shift of a negative operand, the SDIV entries by 2^k that hold the arithmetic shift of a negative operand
    with a non-zero remainder, and the MULHS entries whose signed high word differs from the unsigned one."""
    d = w.oplog()
    logs = [vp.np_u32(d.alu[k], d.n_alu[k], 4) for k in range(4)] + [vp.np_u32(d.alu2[k], d.n_alu2[k], 4) for k in range(4)]
    by_opcode, shr, quotient, mulhs = {}, 0, 0, 0
    for log in logs:
        for opcode, a, b, c in np.asarray(log).reshape(-1, 4).tolist():
            name = va.ARITHMETIC_OPCODES[opcode - 100]
            by_opcode[name] = by_opcode.get(name, 0) + 1
            if name == "SHR32" and b >> 31 and c and a != b >> c:
                assert a == ref.sra(b, c)
                shr += 1
            if name == "SDIV32" and c & (c - 1) == 0 and b >> 31 and b % c:
                assert a == ref.sra(b, c.bit_length() - 1)
                quotient += 1
            if name == "MULHS32" and (b >> 31 or c >> 31) and ((ref.signed(b) * ref.signed(c)) >> 32) & 0xFFFFFFFF != a:
                mulhs += 1
    return by_opcode, shr, quotient, mulhs


# ---- 1. the VM witnesses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.VM))
def test_host_equals_the_reference_on_the_vm_witnesses(machines, name):
    """Under the compiled and the captured machine, receives, sends and both; no hard finding: the VM is the arithmetic's definition."""
    main, prep = cases.witness(name)
    for sides in ("receives", "sends", "both"):
        reports = [held(m, main, prep, sides=sides) for m in machines.values()]
        assert np.array_equal(reports[0].words, reports[1].words)
        assert reports[0].total_hard == 0 and reports[0].truncated == (False, False)
    both, recv, send = reports[0], held(machines["basic"], main, prep), held(machines["basic"], main, prep, sides="sends")
    assert both.counters["live"] == recv.counters["live"] + send.counters["live"]
    assert [(e["chip"], e["interaction"]) for e in both.entries] == sorted((e["chip"], e["interaction"]) for e in recv.entries + send.entries)


@pytest.mark.parametrize("name", list(cases.VM))
def test_pinned_counts_by_two_routes(machines, name):
    main, prep = cases.witness(name)
    a = ref.audit(machines["basic"], main, prep)
    c = a["counters"]
    by_ref = (c["live"], c["judged"], c["other"], {va.ARITHMETIC_OPCODES[k]: n for k, n in enumerate(a["opcodes"]) if n}, c["soft"], c["mulhs_sign_matters"])
    by_opcode, shr, quotient, mulhs = oplog_recount(cases.workload(name))
    assert by_ref == PINNED[name]
    assert (sum(by_opcode.values()), by_opcode, shr + quotient, mulhs) == (PINNED[name][0], PINNED[name][3], PINNED[name][4], PINNED[name][5])
    host = va.arithmetic_audit_host(machines["basic"], main, prep)
    assert {k: v for k, v in host.opcodes.items() if v} == PINNED[name][3] and host.total_soft == PINNED[name][4]


def test_mixed_ops_and_the_traces_that_hold_no_operands(machines):
    """mixed_ops:8 runs mul, mulhu, mulhs, div, sdiv, shl, shr, sra, ne, eq, add, sub, xor and lt.  Facts about the reference that the audit shows
    there: its div and com traces hold only the opcode flag (alu_u32/src/div/mod.rs:84-103, "TODO: Fill in other columns"; com/mod.rs:87-103), so
    each of the 32 records the div chip receives reads (opcode, 0, 0, 0) and is UNDEFINED, division by zero, and each of the 8 EQ32 records of com
    reads 0 == 0 = 0, a WRONG_RESULT (the 8 NE32 records read 0 != 0 = 0 and pass); the 8 SRA rows of the shift chip carry opcode SHR32 and the
    arithmetic result (ARITHMETIC_SHR, soft); the 8 MULHS records hold the unsigned high word where the signed one differs.  With the div and com
    rows completed from the operation logs, as finished chips would hold them, no hard finding is left and the 8 SRA delegations are
    SHIFT_QUOTIENT."""
    main, prep = cases.witness("mixed_ops8")
    rep = held(machines["basic"], main, prep)
    c = rep.counters
    by_opcode, shr, quotient, mulhs = oplog_recount(cases.workload("mixed_ops8"))
    assert (shr, quotient, mulhs) == (8, 8, 8)
    assert {k: v for k, v in rep.opcodes.items() if v} == by_opcode and len(by_opcode) == 13  # SRA32 itself is only ever sent: the log holds it as SHR32
    assert (c["hard"], c["undefined"], c["division_by_zero"], c["wrong_result"], c["soft"], c["arithmetic_shr"], c["mulhs_sign_matters"], c["other"]) == (40, 32, 32, 8, 8, 8, 8, 9)
    assert {(f["chip"], f["kind"], f["opcode"]) for f in rep.hard} == {(cases.DIV, "undefined", 103), (cases.DIV, "undefined", 110), (cases.COM, "wrong_result", 116)}
    assert {f["chip"] for f in rep.soft} == {cases.SHIFT}
    d = cases.workload("mixed_ops8").oplog()
    main = [m.copy() for m in main]
    for row, (opcode, a, b, c_) in enumerate(vp.np_u32(d.alu2[1], d.n_alu2[1], 4).tolist()):
        main[cases.DIV][row, 0:12] = cases.word_bytes(b) + cases.word_bytes(c_) + cases.word_bytes(a)
    for row, (opcode, a, b, c_) in enumerate(vp.np_u32(d.alu2[3], d.n_alu2[3], 4).tolist()):  # com: the inputs in columns 0..7, the boolean in column 11
        main[cases.COM][row, 0:8], main[cases.COM][row, 11] = cases.word_bytes(b) + cases.word_bytes(c_), a
    done = held(machines["basic"], main, prep)
    assert (done.total_hard, done.counters["shift_quotient"], done.counters["arithmetic_shr"]) == (0, 8, 8)
    sends = held(machines["basic"], main, prep, sides="sends")
    assert sends.opcodes["SRA32"] == 8 and sends.total_soft == 0  # the cpu sends SRA32 with the arithmetic result: what the opcode computes
    # the shift chip delegates SRA as DIV32 (shift/mod.rs: is_shr + is_sra select Div32), whose unsigned quotient the arithmetic result is not
    assert sends.counters["wrong_result"] == 8 and {(f["chip"], f["opcode"]) for f in sends.hard} == {(cases.SHIFT, 103)}


# ---- 2. the planted quotient ----------------------------------------------------------------------------------------------------------------
def test_the_planted_quotient(machines):
    """imm32 100; imm32 7; div32; stop.  The reference's div trace holds no operands (the record reads 0 / 0: UNDEFINED on the witness as
    generated), so the honest row (100, 7, 14) is written first, as a finished div chip would hold it: no finding.  Then 14 becomes 15 in the div
    row, the cpu's write channel and the memory table's write row: the bus audit, the constraint audit, the memory audit and the program audit
    report word for word what they report on the untampered witness, and the arithmetic audit reports exactly one WRONG_RESULT at the div chip
    (and, with the sends, the same verdict on the cpu's record)."""
    m = machines["basic"]
    raw_main, prep = cases.witness("div_100_7")
    raw = held(m, raw_main, prep)
    assert (raw.total_hard, raw.counters["division_by_zero"]) == (1, 1) and raw.hard[0]["chip"] == cases.DIV and raw.hard[0]["x"] == [0, 0, 0, 0]
    main, prep, cpu_row = cases.completed_div()
    assert held(m, main, prep, sides="both").total_hard == 0
    planted, prep, cpu_row = cases.planted_quotient()
    for name in ("bus", "constraint", "memory", "program"):
        audit = getattr(va, name + "_audit_host")
        assert np.array_equal(audit(m, planted, prep).words, audit(m, main, prep).words), name
    rep = held(m, planted, prep)
    assert rep.total_hard == 1 and rep.counters["wrong_result"] == 1 and rep.total_soft == 0
    f = rep.hard[0]
    assert (f["kind"], f["chip"], f["interaction"], f["row"], f["opcode"], f["mask"], f["expected"], f["count"], f["is_send"]) == ("wrong_result", cases.DIV, 0, 0, 103, 0b1000, 14, 1, False)
    assert (f["x"], f["y"], f["z"]) == ([0, 0, 0, 100], [0, 0, 0, 7], [0, 0, 0, 15])
    assert [e["hard"] for e in rep.entries] == [int(e["chip"] == cases.DIV) for e in rep.entries]
    both = held(m, planted, prep, sides="both")
    assert both.total_hard == 2 and [(g["chip"], g["row"], g["is_send"]) for g in both.hard] == [(cases.CPU, cpu_row, True), (cases.DIV, 0, False)]
    assert all((g["kind"], g["mask"], g["expected"], g["z"]) == ("wrong_result", 0b1000, 14, [0, 0, 0, 15]) for g in both.hard)


# ---- 3. one test per kind and reason ------------------------------------------------------------------------------------------------------------
def test_mulhs_with_a_negative_operand(machines):
    """-2 * 3: the unsigned high word 2 is what the reference computes and is accepted; the ISA's signed high word 0xFFFFFFFF is WRONG_RESULT."""
    main, prep = cases.witness("mulhs")
    rep = held(machines["basic"], main, prep)
    assert rep.total_hard == 0 and rep.counters["mulhs_sign_matters"] == 1 and rep.opcodes["MULHS32"] == 1
    mul = 5
    row = [r for r in range(main[mul].shape[0]) if main[mul][r, 0:4].tolist() == [255, 255, 255, 254]]
    assert len(row) == 1
    t = [m.copy() for m in main]
    it = machines["basic"].interactions(mul)[0]
    zcols = [f[1][0][1] for f in it["fields"][9:13]]
    assert t[mul][row[0], zcols].tolist() == [0, 0, 0, 2]
    t[mul][row[0], zcols] = 255
    rep = held(machines["basic"], t, prep)
    assert rep.counters["wrong_result"] == 1 and rep.counters["mulhs_sign_matters"] == 1
    assert (rep.hard[0]["expected"], rep.hard[0]["mask"], rep.hard[0]["chip"]) == (2, 0b1111, mul)


def test_sra_of_a_negative_odd_value(machines):
    """-11 >> 1 = -6.  The shift chip's row carries opcode SHR32 and -6 (ARITHMETIC_SHR); the div log holds (SDIV32, -6, -11, 2), which in the div
    chip's row (written as a finished div chip would hold it; the reference's generator leaves it empty) is SHIFT_QUOTIENT: -11 / 2 truncates to
    -5.  No hard finding."""
    main, prep = cases.witness("sra")
    d = cases.workload("sra").oplog()
    ops = vp.np_u32(d.alu2[1], d.n_alu2[1], 4).tolist()
    assert ops == [[110, 0xFFFFFFFA, 0xFFFFFFF5, 2]]
    main = [m.copy() for m in main]
    main[cases.DIV][0, 0:12] = cases.word_bytes(0xFFFFFFF5) + cases.word_bytes(2) + cases.word_bytes(0xFFFFFFFA)
    rep = held(machines["basic"], main, prep)
    assert rep.total_hard == 0 and (rep.counters["shift_quotient"], rep.counters["arithmetic_shr"]) == (1, 1)
    assert [(f["kind"], f["chip"], f["opcode"], f["expected"]) for f in rep.soft] == [("shift_quotient", cases.DIV, 110, 0xFFFFFFFB), ("arithmetic_shr", cases.SHIFT, 106, 0x7FFFFFFA)]


def test_both_sides_judge_the_cpus_send_as_the_chips_receive(machines):
    main, prep = cases.witness("alu100")
    t = [m.copy() for m in main]
    add, row = 3, 5
    it = machines["basic"].interactions(add)[4]
    zcol = it["fields"][12][1][0][1]
    t[add][row, zcol] = (int(t[add][row, zcol]) + 1) % 256
    x, y = ([int(t[add][row, it["fields"][k][1][0][1]]) for k in range(a, a + 4)] for a in (1, 5))
    cpu_row = [r for r in range(t[0].shape[0]) if t[0][r, 3] == 100 and t[0][r, 9] == 1 and t[0][r, 32:36].tolist() == x and t[0][r, 39:43].tolist() == y][0]
    t[0][cpu_row, 49] = t[add][row, zcol]
    rep = held(machines["basic"], t, prep, sides="both")
    assert rep.total_hard == 2
    a, b = rep.hard
    assert (a["chip"], a["row"], a["is_send"], b["chip"], b["row"], b["is_send"]) == (0, cpu_row, True, add, row, False)
    assert all(a[k] == b[k] for k in ("kind", "mask", "opcode", "x", "y", "z", "expected")) and a["kind"] == "wrong_result" and a["mask"] == 0b1000
    assert held(machines["basic"], t, prep).total_hard == 1 and held(machines["basic"], t, prep, sides="sends").total_hard == 1


def test_each_kind_and_reason_on_one_record():
    def one(opcode, x, y, z, count=1):
        return on_alu(cases.padded([cases.record(opcode, x, y, z, count)]))

    for opcode, x, y, z, kind, mask, want in ((103, 9, 0, 0, "undefined", 1, 0), (110, 9, 0, 0, "undefined", 1, 0), (110, 0x80000000, 0xFFFFFFFF, 0x80000000, "undefined", 2, 0),
                                              (105, 1, 32, 0, "undefined", 3, 0), (106, 1, 255, 0, "undefined", 3, 0), (113, 1, 256, 0, "undefined", 3, 0),
                                              (100, 0xFFFFFFFF, 1, 1, "wrong_result", 0b1000, 0), (102, 0x10000, 0x10000, 1, "wrong_result", 0b1000, 0),
                                              (114, 0xFFFFFFFF, 0xFFFFFFFF, 1, "wrong_result", 0b1111, 0xFFFFFFFE), (117, 0x80000000, 0, 0, "wrong_result", 0b1000, 1),
                                              (110, 0xFFFFFFF5, 0x80000000, 0xFFFFFFFF, "shift_quotient", 0b1111, 0), (110, 0xFFFFFFF5, 1, 0xFFFFFFF5, None, 0, 0),
                                              (106, 0x80000000, 31, 0xFFFFFFFF, "arithmetic_shr", 0b1111, 1), (106, 0x80000000, 0, 0x80000000, None, 0, 0),
                                              (113, 0x80000000, 31, 0xFFFFFFFF, None, 0, 0), (113, 0x80000000, 31, 1, "wrong_result", 0b1111, 0xFFFFFFFF)):
        rep = one(opcode, x, y, z)
        found = rep.hard + rep.soft
        assert len(found) == (kind is not None), (opcode, x, y, z)
        if kind:
            assert (found[0]["kind"], found[0]["mask"], found[0]["expected"]) == (kind, mask, want), (opcode, x, y, z, found[0])
            assert rep.counters[kind] == 1 and (rep.total_hard, rep.total_soft) == ((1, 0) if kind in va.ARITHMETIC_HARD_KINDS else (0, 1))
    t = cases.padded([cases.record(100, 1, 2, 3)])
    t[0, 12], t[0, 1] = 256, P - 1
    rep = on_alu(t)
    assert (rep.hard[0]["kind"], rep.hard[0]["mask"], rep.hard[0]["expected"]) == ("malformed", 1 | 1 << 11, 0)
    assert one(300, 1, 2, 9).counters["other"] == 1 and one(99, 1, 2, 9).counters["judged"] == 0 and one(119, 1, 2, 9).total_hard == 0
    assert one(100, 1, 2, 9, count=0).counters["live"] == 0 and one(100, 1, 2, 9, count=P - 1).hard[0]["count"] == P - 1


# ---- 4. the edge corpus ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", cases.HEIGHTS)
def test_edge_corpus_at_height(h):
    rep = on_alu(cases.edge_trace(h), max_findings=1 << 20)
    assert rep.counters["live"] <= h and rep.counters["slots"] >= h


def test_the_whole_corpus_and_the_other_machines():
    t = cases.full_corpus_trace()
    rep = on_alu(t, max_findings=1 << 20)
    c = rep.counters
    assert all(rep.opcodes[name] > 0 for name in va.ARITHMETIC_OPCODES) and all(c[k] > 0 for k in va.ARITHMETIC_KINDS + va.ARITHMETIC_REASONS) and c["other"] == 4
    assert c["mulhs_sign_matters"] > 0 and len(rep.hard) == c["hard"] and len(rep.soft) == c["soft"]
    pair = on_alu(t, "alu_pair", sides="both", max_findings=1 << 20)
    assert pair.counters["hard"] == 2 * c["hard"] and [e["is_send"] for e in pair.entries] == [False, True] and [f["chip"] for f in pair.hard] == [0] * c["hard"] + [1] * c["hard"]
    assert on_alu(t, "alu_pair", sides="sends").entries[0]["chip"] == 1
    assert np.array_equal(on_alu(t, "clk", max_findings=1 << 20).words[10:80], rep.words[10:80])  # a fourteenth field is ignored


# ---- 5. limits, null options, refusals -----------------------------------------------------------------------------------------------------------
def test_limits():
    t = cases.many_findings()
    for k in (0, 1, 299, 300, 301, 1 << 20):
        rep = on_alu(t, max_findings=k)
        assert (rep.total_hard, rep.total_soft) == (300, 300) and len(rep.hard) == min(k, 300) and len(rep.soft) == min(k, 300)
        assert rep.truncated == (k < 300, k < 300) and rep.max_findings == k
    with pytest.raises(va.VgpuError, match="arithmetic_audit: max_findings is at most 2\\^20"):
        va.arithmetic_audit_host(cases.machine("alu"), [t], [], max_findings=(1 << 20) + 1)


def _host_raw(machine, traces, opts):
    """vgpu_arithmetic_audit_host with the options pointer as given (None: null)."""
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in traces]
    ptrs = (ctypes.c_void_p * len(mains))(*[m.ctypes.data for m in mains])
    hs = (ctypes.c_uint64 * len(mains))(*[m.shape[0] for m in mains])
    ws = (ctypes.c_uint64 * len(mains))(*[m.shape[1] for m in mains])
    h = ctypes.c_void_p()
    code = L.vgpu_arithmetic_audit_host(machine._h, ptrs, hs, ws, ctypes.c_uint32(len(mains)), None, None, None, None, ctypes.c_uint32(0), None if opts is None else ctypes.byref(opts),
                                        ctypes.byref(h))
    if code:
        return code, L.vgpu_last_error().decode(), None
    L.vgpu_arithmetic_report_len.restype = ctypes.c_uint64
    L.vgpu_arithmetic_report_words.restype = ctypes.POINTER(ctypes.c_uint32)
    n = L.vgpu_arithmetic_report_len(h)
    words = np.ctypeslib.as_array(L.vgpu_arithmetic_report_words(h), shape=(n,)).copy()
    timing = (ctypes.c_double * 3)()
    L.vgpu_arithmetic_report_timing(h, timing)
    L.vgpu_arithmetic_report_free(h)
    return 0, "", (words, list(timing))


def test_null_options_and_a_struct_taken_as_given():
    t = cases.many_findings()
    code, _, (words, timing) = _host_raw(cases.machine("alu"), [t], None)
    rep = va.ArithmeticReport(words)
    assert code == 0 and np.array_equal(words, on_alu(t).words) and (rep.max_findings, rep.bus, rep.sides) == (64, (True, 0), 1)
    assert timing[0] == 0 and timing[1] > 0 and timing[2] == rep.counters["live"] == 600
    code, _, (words, _) = _host_raw(cases.machine("alu"), [t], va.ArithmeticAuditOpts(0, 1, 0, 1, 0))
    rep = va.ArithmeticReport(words)
    assert len(rep.hard) == 0 and rep.total_hard == 300 and rep.truncated == (True, True)
    code, msg, _ = _host_raw(cases.machine("alu"), [t], va.ArithmeticAuditOpts(0, 1, 0, 0, 0))
    assert code == -1 and "sides is 1 (receives), 2 (sends) or 3 (both), got 0" in msg


def test_refusals_with_their_messages(machines):
    t = cases.edge_trace(64)
    alu = cases.machine("alu")
    for match, machine, kw in (("interaction 0 of chip short has 12 fields on global bus 0; an ALU record has at least 13", cases.machine("short"), {}),
                               ("no chip receives on global bus 0: there is no ALU record to audit", cases.machine("tx_only"), {}),
                               ("no chip sends on global bus 0", alu, dict(sides="sends")), ("no chip receives on global bus 7", alu, dict(bus=7)),
                               ("no chip sends or receives on local bus 0", alu, dict(bus=(False, 0), sides="both")), ("sides is 1 \\(receives\\), 2 \\(sends\\) or 3 \\(both\\), got 4", alu, dict(sides=4)),
                               ("max_findings is at most 2\\^20", alu, dict(max_findings=(1 << 20) + 1))):
        with pytest.raises(va.VgpuError, match="arithmetic_audit: " + match) as e:
            va.arithmetic_audit_host(machine, [t], [], **kw)
        assert e.value.code == -1
    code, msg, _ = _host_raw(alu, [t], va.ArithmeticAuditOpts(64, 1, 0, 1, 1))
    assert code == -1 and "arithmetic_audit: reserved must be zero" in msg
    with pytest.raises(va.VgpuError, match="arithmetic_audit: sides is receives, sends or both"):
        va.arithmetic_audit_host(alu, [t], [], sides="all")
    main, prep = cases.witness("fib25")
    # the memory bus's records have 8 fields; the shape refusals are the bus audit's, under this audit's name
    with pytest.raises(va.VgpuError, match="arithmetic_audit: interaction 0 of chip mem has 8 fields on global bus 2"):
        va.arithmetic_audit_host(machines["basic"], main, prep, bus=2)
    with pytest.raises(va.VgpuError, match="arithmetic_audit: need one main trace per chip"):
        va.arithmetic_audit_host(machines["basic"], main[:-1], prep)
    with pytest.raises(va.VgpuError, match="arithmetic_audit: trace heights must be powers of two"):
        va.arithmetic_audit_host(alu, [t[:63]], [])
    assert on_alu(t).counters["live"] == 64  # the library is usable afterwards


def test_signatures_and_json():
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("max_findings", 64, kind), ("bus", None, kind), ("sides", "receives", kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.arithmetic_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.arithmetic_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert ctypes.sizeof(va.ArithmeticAuditOpts) == 20
    rep = on_alu(cases.full_corpus_trace())
    again = va.ArithmeticReport.from_dict(json.loads(rep.to_json()))
    assert again.to_dict() == rep.to_dict() and np.array_equal(again.words, rep.words) and again.hard == rep.hard and rep.truncated == (True, False)
    with pytest.raises(ValueError):
        va.ArithmeticReport(rep.words[:-1])
    w = cases.workload("fib25")
    assert np.array_equal(w.arithmetic_audit_host().words, va.arithmetic_audit_host(va.Machine.basic(), *cases.witness("fib25")).words)


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_lines_and_exit_status(machines):
    """`check` audits the witness the VM generates: the planted lines and the exit status are those of the functions it calls."""
    from valida_amd import cli

    m = machines["basic"]
    clean = va.arithmetic_audit_host(m, *cases.witness("fib25"))
    assert cli.arithmetic_lines(clean) == ["alu: 105 live records in 1159 slots of 9 entries, 105 judged (ADD32 105), 0 other, 0 MULHS32 records where the sign matters, 0 soft, no finding"]
    assert cli.check_status(True, None, None, None, clean) == 0
    # every existing call of check_status behaves as before
    assert cli.check_status(True, None, None) == 0 and cli.check_status(False, None, None) == 1 and cli.check_status(False, None, None, None, clean) == 1
    main, prep, _ = cases.planted_quotient()
    rep = va.arithmetic_audit_host(m, main, prep)
    lines = cli.arithmetic_lines(rep)
    assert lines[0] == "div: 1 wrong result (row 0, DIV32: 100 / 7 = 15, expected 14)" and len(lines) == 2 and lines[1].endswith("1 finding") and cli.check_status(True, None, None, None, rep) == 1
    main, prep = cases.witness("sra")
    rep = va.arithmetic_audit_host(m, main, prep, sides="both")
    lines = cli.arithmetic_lines(rep)
    assert lines[0] == "div: 1 undefined operation (row 0, SDIV32: 0 /s 0 = 0, division by zero)"
    assert lines[1] == "shift: 1 wrong result (row 0, sent, DIV32: 4294967285 / 2 = 4294967290, expected 2147483642)"
    assert lines[2] == "shift: 1 SHR32 record holds the arithmetic shift (row 0, SHR32: 4294967285 >> 1 = 4294967290, expected 2147483642)" and len(lines) == 4
    soft_only = va.arithmetic_audit_host(cases.machine("alu"), [cases.padded([cases.record(110, 0xFFFFFFF5, 2, 0xFFFFFFFA)])], [])
    lines = cli.arithmetic_lines(soft_only, basic=False)
    assert lines[0] == "chip 0: 1 signed quotient by a power of two holds the arithmetic shift (row 0, SDIV32: 4294967285 /s 2 = 4294967290, expected 4294967291)"
    assert cli.check_status(True, None, None, None, soft_only) == 0
    t = cases.padded([cases.record(100, 1, 2, 3)])
    t[0, 2] = 256
    assert cli.arithmetic_lines(va.arithmetic_audit_host(cases.machine("alu"), [t], []), basic=False)[0] == "chip 0: 1 malformed record (row 0, ADD32: fields 2 are not bytes)"


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_arithmetic_on_the_host(tmp_path):
    """A program of additions is clean; a division is not: the reference's div trace holds no operands, so the witness's div record reads 0 / 0."""
    loop, adv, out = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(10)))
    adv.write_bytes(bytes(range(10)))
    r = _cli("check", loop, out, adv, "--host", "--arithmetic", "--sides", "both", "--max-findings", 3)
    assert r.returncode == 0, r.stderr[-3000:]
    last = r.stdout.strip().split("\n")[-1]
    assert last.startswith("alu: ") and last.endswith("no finding")
    rep = va.ArithmeticReport.from_dict(json.loads(out.read_text())["arithmetic"])
    assert rep.total_hard == 0 and rep.sides == 3 and rep.max_findings == 3 and rep.counters["live"] > 0
    div = tmp_path / "div.bin"
    div.write_bytes(vp.machine_code(cases.div_program()))
    r = _cli("check", div, out, "--host", "--arithmetic")
    assert r.returncode == 1 and "div: 1 undefined operation (row 0, DIV32: 0 / 0 = 0, division by zero)" in r.stdout.split("\n")


# ---- 7. the host audit under AddressSanitizer and UBSan, as a stand-alone program ------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "emu", "arithmetic_audit_host.cpp")
    exe = str(tmp_path / "arithmetic_audit_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("arithmetic_audit_host: fib(25): 210 live of 1416 slots, 210 judged, 0 hard, 0 soft") and "refusals: 6 of 6" in r.stdout


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "arithmetic_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libarithmeticauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "host", "arithmetic_audit.hpp"),
            os.path.join(csrc, "host", "bus_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
                os.path.join(csrc, "kernels", f) for f in ("arithmetic_audit.hip", "arithmetic_rule.hpp", "memory_audit.hip", "bus_records.hpp", "interactions.hpp", "launch.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_arithmetic_audit.restype = ctypes.c_int64
    return L


def emulated(emu, kind, main, prep, opts):
    """The report image of the emulated device pass."""
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in main]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    u64 = ctypes.c_uint64

    def arrays(ms):
        n = max(1, len(ms))
        return (ctypes.c_void_p * n)(*[m.ctypes.data for m in ms]), (u64 * n)(*[m.shape[0] for m in ms]), (u64 * n)(*[m.shape[1] for m in ms])

    mp, mh, mw = arrays(mains)
    pp, ph, pw = arrays([m for _, m in preps])
    chips = (ctypes.c_uint32 * max(1, len(preps)))(*[c for c, _ in preps])
    cap = 1 << 22
    out = np.zeros(cap, dtype=np.uint32)
    got = emu.emu_arithmetic_audit(ctypes.c_uint32(kind), mp, mh, mw, ctypes.c_uint32(len(mains)), chips, pp, ph, pw, ctypes.c_uint32(len(preps)), ctypes.byref(opts),
                                   out.ctypes.data_as(ctypes.c_void_p), u64(cap))
    assert got > 0, got
    return out[:got]


def test_emulated_kernels_on_the_vm_witnesses(emu, machines):
    for name in ("fib25", "alu100", "mixed_ops8"):
        main, prep = cases.witness(name)
        for sides in ("receives", "both"):
            want = va.arithmetic_audit_host(machines["basic"], main, prep, sides=sides)
            assert np.array_equal(emulated(emu, 0, main, prep, va._arithmetic_opts(64, None, sides)), want.words), (name, sides)
    main, prep, _ = cases.planted_quotient()
    assert np.array_equal(emulated(emu, 0, main, prep, va._arithmetic_opts(64, None, "both")), va.arithmetic_audit_host(machines["basic"], main, prep, sides="both").words)


def test_emulated_kernels_on_the_edge_corpus(emu):
    alu, pair = cases.machine("alu"), cases.machine("alu_pair")
    for h in cases.HEIGHTS:
        t = cases.edge_trace(h)
        assert np.array_equal(emulated(emu, 1, [t], [], va._arithmetic_opts(1 << 20, None, "receives")), va.arithmetic_audit_host(alu, [t], [], max_findings=1 << 20).words), h
    t = cases.full_corpus_trace()
    for k in (0, 1, 7, 64, 1 << 20):
        assert np.array_equal(emulated(emu, 1, [t], [], va._arithmetic_opts(k, None, "receives")), va.arithmetic_audit_host(alu, [t], [], max_findings=k).words), k
        assert np.array_equal(emulated(emu, 2, [t, t], [], va._arithmetic_opts(k, None, "both")), va.arithmetic_audit_host(pair, [t, t], [], max_findings=k, sides="both").words), k
    m = cases.many_findings()
    for k in (299, 300, 301):
        assert np.array_equal(emulated(emu, 1, [m], [], va._arithmetic_opts(k, None, "receives")), va.arithmetic_audit_host(alu, [m], [], max_findings=k).words), k
    s = cases.synthetic(2048)
    want = va.arithmetic_audit_host(alu, [s], [], max_findings=5)
    assert want.total_hard == 16 and np.array_equal(emulated(emu, 1, [s], [], va._arithmetic_opts(5, None, "receives")), want.words)
