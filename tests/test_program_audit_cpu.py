"""The program audit without a GPU: the host audit (vgpu_program_audit_host) against the numpy reference (tests/program_audit_ref.py) word for
word on the VM witnesses under both machine kinds, with the pinned numbers; the skipped words of a branching program; fib(25) tampered seven
ways; the balance property on the captured `rom` machine (the bus audit reports no unbalanced tuple exactly when the program audit reports
no finding); the edge traces; the limits; null options and every refusal; the command line's lines and exit status; the host audit under
AddressSanitizer and UBSan as a stand-alone program; the device kernels' very source under tools/hipemu."""
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

import program_audit_cases as cases
import program_audit_ref as ref
import valida_amd as va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P


@pytest.fixture(scope="module")
def machines():
    return {"basic": va.Machine.basic(), "ffi": va.Machine.basic_via_ffi()}


def on_rom(n_fields, main, prep, rom_len=0, **kw):
    """The host's report of a `rom` witness, held to the reference's."""
    opts = cases.rom_opts(n_fields)
    want = ref.audit(main, prep, rom_len=rom_len, **opts, **kw)
    rep = va.program_audit_host(cases.rom_machine(n_fields), main, prep, rom_len=rom_len, **opts, **kw)
    assert np.array_equal(rep.words, ref.words(want)), (rep.counters, want["counters"])
    return rep


def found(rep):
    return [(f["kind"], f["row"]) for f in rep.hard]


# ---- 1. the VM's witnesses ---------------------------------------------------------------------------------------------------------------------
PINNED = {"fib25": (256, 32, 23, 7, 65, 138, 64, 53), "fib582": (4096, 32, 23, 13, 583, 2923, 5, 1167), "alu100": (1024, 16, 14, 13, 120, 805, 119, 99),
          "signed_inequality": (32, 32, 20, 19, 13, 19, 12, 0)}


@pytest.mark.parametrize("name", list(cases.VM))
def test_host_equals_reference_on_the_vm_witnesses(machines, name):
    main, prep, rom_len = cases.witness(name)
    want = ref.words(ref.audit(main, prep, rom_len=rom_len))
    for m in machines.values():
        rep = va.program_audit_host(m, main, prep, rom_len=rom_len)
        assert np.array_equal(rep.words, want)
    c = rep.counters
    assert rep.total_hard == 0 and rep.hard == [] and rep.truncated == (False, False, False) and (rep.fetch_chip, rep.table_chip, rep.n_fields) == (0, 1, 6)
    assert c["unfetched_words"] == 0 and rep.unfetched == [] and c["fetched_words"] == c["rom_len"] == rom_len and rep.evaluations == c["fetches"] + c["table_rows"] and rep.device_ms == 0
    assert c["sequential"] + c["stay"] + c["jumps"] == c["fetches"] - 1
    if name in PINNED:
        assert (c["fetches"], c["table_rows"], c["rom_len"], c["hottest_pc"], c["hottest_count"], c["sequential"], c["stay"], c["jumps"]) == PINNED[name]
    if name != "signed_inequality":
        assert rep.total_wrapped == 0 and rep.wrapped == []
    assert np.array_equal(cases.workload(name).program_audit_host().words, rep.words)  # Workload passes its rom_len


def test_signed_inequality_wraps_its_negative_immediates(machines):
    """The reference's set_imm_value writes the u32 value mod p where the ROM holds from_i32: 8 of 32 rows, never a fault."""
    from valida_amd import cli

    main, prep, rom_len = cases.witness("signed_inequality")
    rep = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
    assert rep.total_hard == 0 and rep.total_wrapped == 8 and len(rep.wrapped) == 8 and rep.wrapped[0]["row"] == 5 and rep.wrapped[0]["pc"] == 5
    mask = 0
    for f in rep.wrapped:
        mask |= f["mask"]
        assert f["kind"] == "wrapped_operand" and all((f["found"][j] - f["expected"][j]) % P == cases.TWO32 for j in f["fields"]) and f["fields"]
    assert mask == 0xC  # operands b and c
    assert cli.check_status(True, None, None, rep) == 0


def test_skipped_words():
    (main, prep), rom_len = cases.skipping()
    rep = on_rom(2, main, prep, rom_len)
    assert rep.counters["unfetched_words"] == 2 and rep.counters["unfetched_ranges"] == 1 and rep.unfetched == [(2, 4)] and rep.total_hard == 0
    assert (rep.counters["sequential"], rep.counters["stay"], rep.counters["jumps"], rep.counters["hottest_pc"], rep.counters["hottest_count"]) == (1, 5, 1, 4, 6)


# ---- 2. fib(25) tampered: exactly the stated findings --------------------------------------------------------------------------------------------
def vm_report(machines, kind):
    main, prep, rom_len = cases.vm_tampered(kind)
    want = ref.words(ref.audit(main, prep, rom_len=rom_len))
    for m in machines.values():
        rep = va.program_audit_host(m, main, prep, rom_len=rom_len)
        assert np.array_equal(rep.words, want)
    return rep, main, prep


def test_a_changed_operand_is_one_wrong_instruction(machines):
    rep, main, prep = vm_report(machines, "operand")
    assert found(rep) == [("wrong_instruction", 100)] and rep.total_hard == 1 and rep.total_wrapped == 0
    f = rep.hard[0]
    pc = int(main[0][100, 1])
    assert f["mask"] == 2 and f["fields"] == [1] and f["pc"] == pc and f["expected"][:6] == [int(x) for x in prep[0][1][pc, 1:7]] and f["found"][1] == (f["expected"][1] + 7) % P


def test_an_operand_moved_by_2_to_the_32_is_one_wrapped_operand(machines):
    rep, _, _ = vm_report(machines, "wrapped")
    assert rep.total_hard == 0 and rep.hard == [] and [(f["row"], f["mask"]) for f in rep.wrapped] == [(100, 2)] and rep.total_wrapped == 1


def test_a_pc_moved_to_another_word(machines):
    rep, main, _ = vm_report(machines, "pc_other_word")
    old, new = int(cases.witness("fib25")[0][0][100, 1]), int(main[0][100, 1])
    assert found(rep) == [("wrong_instruction", 100)] + [("multiplicity", i) for i in sorted((old, new))] and rep.total_hard == 3 and rep.total_wrapped == 0
    by_row = {f["row"]: f for f in rep.hard[1:]}
    assert by_row[old]["found"][0] == by_row[old]["expected"][0] + 1 and by_row[new]["found"][0] == by_row[new]["expected"][0] - 1 and by_row[new]["expected"][1] == by_row[new]["expected"][0]


def test_a_pc_on_a_padding_row_of_the_table(machines):
    rep, main, _ = vm_report(machines, "pc_padding")
    old = int(cases.witness("fib25")[0][0][100, 1])
    assert found(rep) == [("pc_out_of_rom", 100)] + [("multiplicity", i) for i in (old, 31)] and rep.total_hard == 3 and rep.hard[0]["pc"] == 31 and rep.hard[2]["expected"][:2] == [1, 1]


def test_a_pc_of_p_minus_1(machines):
    rep, main, _ = vm_report(machines, "pc_p_minus_1")
    old = int(cases.witness("fib25")[0][0][100, 1])
    assert found(rep) == [("pc_out_of_rom", 100), ("multiplicity", old)] and rep.hard[0]["pc"] == P - 1 and rep.total_hard == 2
    assert rep.counters["jumps"] >= 2


def test_a_multiplicity_and_a_key(machines):
    rep, _, _ = vm_report(machines, "multiplicity")
    assert found(rep) == [("multiplicity", 3)] and rep.total_hard == 1 and rep.hard[0]["found"][0] == rep.hard[0]["expected"][0] + 1
    rep, _, _ = vm_report(machines, "key")
    assert found(rep) == [("table_key", 5)] and rep.total_hard == 1 and (rep.hard[0]["found"][0], rep.hard[0]["expected"][0]) == (6, 5)


# ---- 3. the balance property ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("clean",) + cases.TAMPERINGS)
def test_the_bus_balances_exactly_when_there_is_no_finding(kind):
    """The `rom` machine's bus is the reference's program bus, uncommented: with rom_len = the table's height the two audits agree."""
    main, prep = cases.clean(cases.loop_pcs(256, 32), 32) if kind == "clean" else cases.rom_tampered(kind)
    rep = on_rom(2, main, prep)
    bus = va.bus_audit_host(cases.rom_machine(2), main, prep)
    assert bus.balanced == (rep.total_hard == 0 and rep.total_wrapped == 0) == (kind == "clean")
    assert bus.buses[0]["bus"] == (1, cases.BUS) and bus.buses[0]["sends"] == 256


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------------
def test_edge_traces():
    seen = {}
    for name, nf, (main, prep), rom_len in cases.edge_cases():
        seen[name] = on_rom(nf, main, prep, rom_len)
    for H in cases.FETCH_HEIGHTS:
        rep = seen["fetch_height_%d" % H]
        assert rep.counters["fetches"] == H and rep.total_hard == 0 and rep.counters["sequential"] + rep.counters["jumps"] == H - 1
    for T in cases.TABLE_HEIGHTS:
        assert seen["table_height_%d" % T].counters["table_rows"] == T and seen["table_height_%d" % T].total_hard == 0
    c = seen["one_pc"].counters
    assert (c["hottest_pc"], c["hottest_count"], c["stay"], c["fetched_words"], c["unfetched_ranges"]) == (7, 4096, 4095, 1, 2) and seen["one_pc"].unfetched == [(0, 7), (8, 32)]
    assert (seen["63_and_1"].counters["hottest_count"], seen["63_and_1"].counters["fetched_words"]) == (253, 2) and seen["63_and_1"].total_hard == 0
    assert seen["two_bins"].counters["hottest_pc"] == 3 and seen["two_bins"].counters["hottest_count"] == 1024 and seen["two_bins"].counters["jumps"] == 2047
    c = seen["slice_edges"].counters
    assert c["fetched_words"] == 4 and c["unfetched_ranges"] == 2 and seen["slice_edges"].unfetched == [(1, 32767), (32769, 65535)] and c["hottest_pc"] == 0 and c["hottest_count"] == 2049
    assert found(seen["planted"]) == [("wrong_instruction", r) for r in cases.PLANT_ROWS]
    assert found(seen["eight_fields"]) == [("wrong_instruction", 300)] and seen["eight_fields"].hard[0]["mask"] == 0x80 and [(f["row"], f["mask"]) for f in seen["eight_fields"].wrapped] == [(301, 1)]
    assert seen["one_field"].n_fields == 1 and seen["one_field"].total_hard == 0


def test_a_bin_count_above_2_to_the_16():
    main, prep = cases.big_bin()
    rep = on_rom(2, main, prep)
    assert rep.counters["hottest_count"] == 1 << 17 and rep.counters["hottest_pc"] == 1 and rep.unfetched == [(0, 1)] and rep.total_hard == 0


def test_synthetic_trace():
    """The pattern the GPU tests run at four heights: runs, strides, a hot word, planted findings of three kinds."""
    main, prep = cases.synthetic(8192)
    c = on_rom(2, main, prep, max_findings=300).counters
    assert c["wrong_instruction"] > 0 and c["wrapped_operand"] > 0 and c["pc_out_of_rom"] == 1 and c["multiplicity"] == 1 and c["stay"] > 0 and c["jumps"] > 0


def test_limits():
    main, prep = cases.many()
    full = on_rom(2, main, prep, max_findings=1 << 20, max_ranges=1 << 20)
    c = full.counters
    assert (c["table_key"], c["wrong_instruction"], c["wrapped_operand"], c["multiplicity"], c["unfetched_ranges"]) == (300, 300, 300, 300, 512) and c["hard"] == len(full.hard) == 900
    assert len(full.wrapped) == 300 and len(full.unfetched) == 512 and full.unfetched[:2] == [(1, 2), (3, 4)] and full.truncated == (False, False, False)
    assert [f["kind"] for f in full.hard] == ["table_key"] * 300 + ["wrong_instruction"] * 300 + ["multiplicity"] * 300
    for k in (0, 1, 300, 301, 601):
        rep = on_rom(2, main, prep, max_findings=k, max_ranges=k)
        assert rep.hard == full.hard[:k] and rep.wrapped == full.wrapped[:k] and rep.unfetched == full.unfetched[:k] and rep.counters == full.counters
        assert rep.truncated == (True, k < 300, k < 512)


# ---- 5. options, refusals -----------------------------------------------------------------------------------------------------------------------------
def _host_call(machine, main, prep, opts):
    L = va.lib()
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in main]
    preps = [(c, np.ascontiguousarray(m, dtype=np.uint32)) for c, m in prep]
    n, k = len(mains), len(preps)
    h = ctypes.c_void_p()
    rc = L.vgpu_program_audit_host(machine._h, (ctypes.c_void_p * n)(*[m.ctypes.data for m in mains]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in mains]),
                                   (ctypes.c_uint64 * n)(*[m.shape[1] for m in mains]), ctypes.c_uint32(n), (ctypes.c_uint32 * k)(*[c for c, _ in preps]),
                                   (ctypes.c_void_p * k)(*[m.ctypes.data for _, m in preps]), (ctypes.c_uint64 * k)(*[m.shape[0] for _, m in preps]),
                                   (ctypes.c_uint64 * k)(*[m.shape[1] for _, m in preps]), ctypes.c_uint32(k), ctypes.byref(opts) if opts is not None else None, ctypes.byref(h))
    return rc, (va._audit_report("program", va.ProgramReport, h) if rc == 0 else None)


def test_null_options_are_the_basic_machines(machines):
    main, prep, rom_len = cases.vm_tampered("operand")
    rc, rep = _host_call(machines["basic"], main, prep, None)
    want = va.program_audit_host(machines["basic"], main, prep)  # rom_len 0: the table's height
    assert rc == 0 and np.array_equal(rep.words, want.words) and rep.counters["rom_len"] == 32 and (rep.max_findings, rep.max_ranges) == (64, 64) and found(rep) == [("wrong_instruction", 100)]
    assert rep.counters["unfetched_words"] == 32 - rom_len and rep.unfetched == [(rom_len, 32)]  # the padding rows count as words then
    opts = va._program_opts(rom_len, 0, 0, None, None)  # a struct is taken as given: 0 lists nothing
    rc, rep = _host_call(machines["basic"], main, prep, opts)
    assert rc == 0 and rep.hard == [] and rep.total_hard == 1
    M = ctypes.CDLL(va.lib()._name)
    length, words_of, timing, free = (getattr(M, "vgpu_program_report_%s" % x) for x in ("len", "words", "timing", "free"))
    length.restype, words_of.restype, timing.restype, free.restype = ctypes.c_uint64, ctypes.c_void_p, None, None
    assert length(None) == 0 and words_of(None) is None
    tm = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    timing(None, tm)
    assert list(tm) == [0.0, 0.0, 0.0]
    free(None)


REFUSALS = [(dict(fetch=(0, 3, [1, 2])), "pc_col 3 is outside chip fetcher's trace"), (dict(fetch=(0, 0, [1, 3])), "field column 3 .* is outside chip fetcher's trace"),
            (dict(table=(1, 0, [1, 3], 0)), "table column 3 .* is outside chip table's preprocessed trace"), (dict(table=(1, 3, [1, 2], 0)), "key_col 3 is outside"),
            (dict(table=(1, 0, [1, 2], 1)), "mult_col 1 is outside chip table's trace"), (dict(table=(0, 0, [1, 2], 0)), "table chip fetcher has no preprocessed trace"),
            (dict(fetch=(2, 0, [1, 2])), "fetch_chip 2 is not a chip"), (dict(table=(7, 0, [1, 2], 0)), "table_chip 7 is not a chip"), (dict(rom_len=33), "rom_len 33 is above the table's height 32"),
            (dict(max_findings=(1 << 20) + 1), "at most 2\\^20"), (dict(max_ranges=(1 << 20) + 1), "at most 2\\^20")]


def test_refusals():
    main, prep = cases.clean(cases.loop_pcs(64, 32), 32)
    machine = cases.rom_machine(2)
    for kw, match in REFUSALS:
        with pytest.raises(va.VgpuError, match="program_audit: .*" + match) as e:
            va.program_audit_host(machine, main, prep, **dict(cases.rom_opts(2), **kw))
        assert e.value.code == -1
    for n_fields in (0, 9):
        opts = va._program_opts(0, 64, 64, (0, 0, [1, 2]), (1, 0, [1, 2], 0))
        opts.n_fields = n_fields
        assert _host_call(machine, main, prep, opts)[0] == -1 and "n_fields is 1 to 8" in va.lib().vgpu_last_error().decode()
    opts = va._program_opts(0, 64, 64, (0, 0, [1, 2]), (1, 0, [1, 2], 0))
    opts.reserved = 1
    assert _host_call(machine, main, prep, opts)[0] == -1 and "reserved must be zero" in va.lib().vgpu_last_error().decode()
    short = [(1, prep[0][1][:16])]  # the table's two traces differ in height
    with pytest.raises(va.VgpuError, match="program_audit: the table chip's main trace has 32 rows and its preprocessed trace 16"):
        va.program_audit_host(machine, main, short, **cases.rom_opts(2))
    with pytest.raises(va.VgpuError, match="program_audit: .*one main trace per chip"):
        va.program_audit_host(machine, main[:1], prep, **cases.rom_opts(2))
    with pytest.raises(va.VgpuError, match="program_audit: n_fields is 1 to 8"):
        va.program_audit_host(machine, main, prep, fetch=(0, 0, []), table=(1, 0, [], 0))
    assert on_rom(2, main, prep).total_hard == 0  # the library is usable afterwards


def test_signatures_and_json(machines):
    kind, empty = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.empty
    options = [("rom_len", 0, kind), ("max_findings", 64, kind), ("max_ranges", 64, kind), ("fetch", None, kind), ("table", None, kind)]

    def signature_of(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    assert signature_of(va.program_audit_host) == [(n, empty, kind) for n in ("machine", "main_matrices", "preprocessed")] + options
    assert signature_of(va.Prover.program_audit) == [(n, empty, kind) for n in ("self", "main", "preprocessed")] + options
    assert ctypes.sizeof(va.ProgramAuditOpts) == 104
    main, prep, rom_len = cases.vm_tampered("pc_padding")
    rep = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
    d = json.loads(rep.to_json())
    again = va.ProgramReport.from_dict(d)
    assert again.to_dict() == rep.to_dict() and np.array_equal(again.words, rep.words) and again.hard == rep.hard
    with pytest.raises(ValueError):
        va.ProgramReport(rep.words[:-1])


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_lines_and_exit_status(machines):
    """`check` audits the witness the VM generates, which is truthful: the tampered lines and the exit status are those of the functions it calls."""
    from valida_amd import cli

    main, prep, rom_len = cases.witness("fib25")
    clean = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
    lines = cli.program_lines(clean)
    assert len(lines) == 1 and lines[0].startswith("cpu: 256 fetches of a 23-word ROM (32 table rows): all words fetched, hottest pc 7 (65 fetches), 138 sequential, 64 stay, 53 jumps")
    assert lines[0].endswith("no finding") and cli.check_status(True, None, None, clean) == 0
    # every existing call of check_status behaves as before
    assert cli.check_status(True, None, None) == 0 and cli.check_status(False, None, None) == 1 and cli.check_status(False, None, None, clean) == 1
    main, prep, rom_len = cases.witness("signed_inequality")
    wrapped = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
    lines = cli.program_lines(wrapped)
    assert lines[0] == "cpu: 8 fetches differ from the ROM only by 2^32 in an immediate (first row 5, pc 5, fields c)" and len(lines) == 2 and cli.check_status(True, None, None, wrapped) == 0
    main, prep, rom_len = cases.vm_tampered("operand")
    rep = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
    f = rep.hard[0]
    lines = cli.program_lines(rep)
    assert lines[0] == "cpu: 1 wrong instruction (row 100, pc %d: operand a %d, ROM %d)" % (f["pc"], f["found"][1], f["expected"][1]) and len(lines) == 2 and lines[1].endswith("1 finding")
    assert cli.check_status(True, None, None, rep) == 1
    main, prep, rom_len = cases.vm_tampered("pc_padding")
    lines = cli.program_lines(va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len))
    assert lines[0] == "cpu: 1 pc outside the ROM (row 100, pc 31, ROM length 23)" and lines[1].startswith("program: 2 wrong multiplicities (word %d: multiplicity " % int(cases.witness("fib25")[0][0][100, 1]))
    main, prep, rom_len = cases.vm_tampered("key")
    assert cli.program_lines(va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len))[0] == "program: 1 wrong table key (row 5: key 6)"
    (main, prep), rom_len = cases.skipping()
    skip = va.program_audit_host(cases.rom_machine(2), main, prep, rom_len=rom_len, **cases.rom_opts(2))
    assert "2 of 5 words never fetched ([2, 4))" in cli.program_lines(skip)[-1]


def test_cli_check_program_on_the_host(tmp_path, machines):
    import sys

    import valida_programs as vp

    prog, out = tmp_path / "byte_loads.bin", tmp_path / "report.json"
    prog.write_bytes(vp.machine_code(vp.byte_loads_program()))
    r = subprocess.run([sys.executable, "-m", "valida_amd.cli", "check", str(prog), str(out), "--host", "--program"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    last = r.stdout.strip().split("\n")[-1]
    assert last.startswith("cpu: ") and "all words fetched" in last and last.endswith("no finding")
    j = json.loads(out.read_text())
    rep = va.ProgramReport.from_dict(j["program"])
    assert rep.total_hard == 0 and rep.counters["rom_len"] == va.Workload.from_executable(prog.read_bytes()).program_len


# ---- 7. the host audit under AddressSanitizer and UBSan, as a stand-alone program ------------------------------------------------------------------
def test_host_audit_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "emu", "program_audit_host.cpp")
    exe = str(tmp_path / "program_audit_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("program_audit_host: fib(25): 256 fetches, 23 of 23 words fetched, 0 hard, 0 wrapped") and "operand: 1 hard" in r.stdout and "refusals: 7 of 7" in r.stdout


# ---- 8. the device kernels' source under emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "program_audit_emu.cpp")
    out = os.path.join(ROOT, "build", "libprogramauditemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "host", "program_audit.hpp"),
            os.path.join(csrc, "host", "bus_audit.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [os.path.join(csrc, "kernels", f) for f in ("program_audit.hip", "memory_audit.hip", "launch.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_program_audit.restype = ctypes.c_int64
    return L


def emulated(emu, fetch, tmain, tprep, opts):
    """The report image of the emulated device pass over the three traces the audit reads."""
    f, t, p = (np.ascontiguousarray(m, dtype=np.uint32) for m in (fetch, tmain, tprep))
    cap = 1 << 20
    out = np.zeros(cap, dtype=np.uint32)
    u64 = ctypes.c_uint64
    got = emu.emu_program_audit(ctypes.c_void_p(f.ctypes.data), u64(f.shape[0]), u64(f.shape[1]), ctypes.c_void_p(t.ctypes.data), u64(t.shape[0]), u64(t.shape[1]),
                                ctypes.c_void_p(p.ctypes.data), u64(p.shape[0]), u64(p.shape[1]), ctypes.byref(opts), out.ctypes.data_as(ctypes.c_void_p), u64(cap))
    assert got > 0, got
    return out[:got]


def test_emulated_kernels_on_the_vm_witnesses_and_the_tampered_traces(emu, machines):
    inputs = [cases.witness(n) for n in ("fib25", "signed_inequality", "alu100")] + [cases.vm_tampered(k) for k in cases.TAMPERINGS]
    for main, prep, rom_len in inputs:
        want = va.program_audit_host(machines["basic"], main, prep, rom_len=rom_len)
        assert np.array_equal(emulated(emu, main[0], main[1], prep[0][1], va._program_opts(rom_len, 64, 64, None, None)), want.words)


def test_emulated_kernels_on_the_edge_traces(emu):
    for name, nf, (main, prep), rom_len in cases.edge_cases():
        o = cases.rom_opts(nf)
        want = va.program_audit_host(cases.rom_machine(nf), main, prep, rom_len=rom_len, **o)
        assert np.array_equal(emulated(emu, main[0], main[1], prep[0][1], va._program_opts(rom_len, 64, 64, o["fetch"], o["table"])), want.words), name
    main, prep = cases.many()
    o = cases.rom_opts(2)
    for k in (0, 1, 300, 601):
        want = va.program_audit_host(cases.rom_machine(2), main, prep, max_findings=k, max_ranges=k, **o)
        assert np.array_equal(emulated(emu, main[0], main[1], prep[0][1], va._program_opts(0, k, k, o["fetch"], o["table"])), want.words), k
