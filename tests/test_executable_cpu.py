"""Valida executables on the host: the loader (raw machine code and ELF, elf/src/lib.rs:19-120), the four instructions the VM gained
(READ_ADVICE, LOADU8, LOADS8, STOREU8: cpu/src/lib.rs:398-436, :493-601, :646-697), their operation logs and cpu rows, the kernel source of
k_tracegen_cpu under tools/hipemu, the verdicts of the oracle's and the product's verifiers, and `python -m valida_amd.cli`."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH = 0x1000  # stack height of the built-in workloads
IS_LOAD_U8, IS_LOAD_S8, IS_STORE_U8, IS_ADVICE = 14, 15, 17, 23
CH = lambda c, k: 29 + 7 * c + k  # memory channel c: used, is_read, addr, value[4]


def load(data, **kw):
    return va.Workload.from_executable(data, **kw)


def text_words(n):
    return vp.machine_code([(vp.IMM32, [-4 * (i + 1), 0, 0, 0, i]) for i in range(n - 1)] + [(vp.STOP, [])])


# ---- loader ------------------------------------------------------------------------------------------------------------------------------
def sample_elf(is64):
    code = text_words(3)
    sections = [(".text", vp.SHT_PROGBITS, 6, 48, code),                             # ALLOC|EXECINSTR at a nonzero address: initial pc 2
                (".data", vp.SHT_PROGBITS, 3, 0x100, bytes([1, 2, 3, 4, 5, 6])),      # ALLOC|WRITE, padded to 8 bytes
                (".rodata", vp.SHT_PROGBITS, 2, 0x200, bytes([9, 8, 7, 6])),          # ALLOC
                (".rodata.str", vp.SHT_PROGBITS, 0x32, 0x104, b"AB"),                 # ALLOC|MERGE|STRINGS: overwrites the .data cell 0x104
                (".comment", vp.SHT_PROGBITS, 0x30, 0x300, b"xyzw"),                  # not ALLOC: ignored
                (".bss", vp.SHT_NOBITS, 3, 0x400, 64)]                                # NOBITS: ignored
    return elf_bytes(sections, is64), code


def elf_bytes(sections, is64=True, **kw):
    return vp.elf(sections, is64=is64, **kw)


@pytest.mark.parametrize("is64", [False, True])
def test_elf_rom_initial_pc_and_static_cells(is64):
    img, code = sample_elf(is64)
    w = load(img, max_cycles=0)
    rom = w.preprocessed()[0][1]
    assert w.program_len == 2 + 3  # a zero image up to sh_addr + sh_size: two zero instructions, then the text
    assert rom[:2, 1:].max() == 0 and rom[2:5, 1].tolist() == [vp.IMM32, vp.IMM32, vp.STOP]
    assert w.cycles == 0 and w.cpu_height == 0
    cells = {0x100: 0x01020304, 0x104: 0x41420000, 0x200: 0x09080706}  # Word([b0, b1, b2, b3]); the later section wins at 0x104
    for a, v in cells.items():
        assert w.cell(a) == v
    for a in (0x108, 0x300, 0x400):
        with pytest.raises(va.VgpuError):
            w.cell(a)
    d = w.oplog()
    assert int(d.n_cpu) == 0 and vp.np_u32(d.static_cells, d.n_static, 2).tolist() == sorted([a, v] for a, v in cells.items())
    with pytest.raises(va.VgpuError, match="without running"):
        w.main_trace(0)
    r = load(img, stack_height=SH)  # runs from pc 2
    assert r.cycles == 3 and r.cell(SH - 4) == 0 and r.cell(SH - 8) == 1
    assert r.main_trace(0)[0, 1] == 2  # pc column


@pytest.mark.parametrize("is64", [False, True])
def test_llvm_readelf_parses_the_test_images(is64):
    readelf = shutil.which("llvm-readelf") or next((p for p in ("/opt/rocm/llvm/bin/llvm-readelf",) if os.path.exists(p)), None)
    if readelf is None:
        pytest.skip("no llvm-readelf on this machine")
    img, _ = sample_elf(is64)
    path = os.path.join(ROOT, "build", "test_elf%d.o" % (64 if is64 else 32))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").write(img)
    out = subprocess.run([readelf, "-S", "-W", path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for name in (".text", ".data", ".rodata", ".rodata.str", ".comment", ".bss", ".shstrtab"):
        assert name in out.stdout
    assert "warning" not in out.stderr.lower()


def test_raw_machine_code_and_a_trailing_partial_record():
    code = text_words(4)
    for tail in (b"", b"\x07", bytes(23)):
        w = load(code + tail, stack_height=SH)
        assert w.program_len == 4 and w.cycles == 4 and w.cell(SH - 12) == 2
    assert load(b"", max_cycles=0).program_len == 0
    assert load(b"\x7fEL", max_cycles=0).program_len == 0  # shorter than the magic: raw machine code


def test_loader_refusals():
    code = text_words(2)
    good = [(".text", vp.SHT_PROGBITS, 6, 0, code)]
    img = elf_bytes(good)
    cases = {
        "truncated ELF header": img[:40],
        "truncated ELF identification": img[:10],
        "ELF class 3": elf_bytes(good, elf_class=3),
        "big-endian": elf_bytes(good, big_endian=True),
        "extended section numbering": elf_bytes(good, e_shnum=0),
        "no text section": elf_bytes([(".data", vp.SHT_PROGBITS, 3, 0, b"1234")]),
        "section header table": img[:-10],
        "32-bit address space": elf_bytes([good[0], (".data", vp.SHT_PROGBITS, 3, 0xFFFFFFFC, b"12345678")]),
        "limit of 4194304 instructions": elf_bytes([(".text", vp.SHT_PROGBITS, 6, 24 << 22, code)]),
    }
    for name, img2 in cases.items():
        with pytest.raises(va.VgpuError, match=name):
            load(img2, max_cycles=0)
    # section data outside the file: the .text size field of the ELF64 image pointed past the end
    e = bytearray(img)
    shoff = struct.unpack_from("<Q", e, 0x28)[0]
    struct.pack_into("<Q", e, shoff + 64 + 32, len(e))
    with pytest.raises(va.VgpuError, match="outside the file"):
        load(bytes(e), max_cycles=0)
    # a static-data count above the limit (sections may overlap: the count is of the cells the file declares)
    many = elf_bytes([good[0]] + [(".data", vp.SHT_PROGBITS, 3, 0, bytes(1 << 20)) for _ in range(17)])
    with pytest.raises(va.VgpuError, match="limit of 4194304 cells"):
        load(many, max_cycles=0)
    # raw machine code above the instruction limit
    with pytest.raises(va.VgpuError, match="limit of 4194304 instructions"):
        load(bytes(24 * ((1 << 22) + 1)), max_cycles=0)


_FUZZ = r"""
import random, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import valida_amd as va
from test_executable_cpu import sample_elf
img, _ = sample_elf(%(is64)s)
rng = random.Random(%(seed)d)
ok = refused = 0
cases = [img[:k] for k in range(len(img) + 1)]
for _ in range(%(n)d):
    b = bytearray(img)
    for _ in range(rng.randint(1, 4)):
        i = rng.randrange(len(b))
        b[i] = rng.choice([0, 0xFF, 0x7F, 0x80, rng.randrange(256)])
    cases.append(bytes(b))
for c in cases:
    try:
        va.Workload.from_executable(c, max_cycles=0)
        ok += 1
    except va.VgpuError:
        refused += 1
print(ok, refused)
"""


@pytest.mark.parametrize("is64", [False, True])
def test_truncations_and_mutations_load_or_are_refused(is64):
    src = _FUZZ % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), is64=is64, seed=7 + is64, n=2500)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ok, refused = map(int, r.stdout.split())
    assert ok + refused > 2500 and ok > 0 and refused > 0


# ---- VM semantics ------------------------------------------------------------------------------------------------------------------------
def channels(row):
    return [(int(row[CH(c, 0)]), int(row[CH(c, 2)]), [int(x) for x in row[CH(c, 3):CH(c, 3) + 4]]) for c in range(3)]


def test_loadu8_loads8_at_each_byte_offset():
    w = load(vp.machine_code(vp.byte_loads_program()), stack_height=SH)
    assert [w.cell(SH - 16 - 8 * k) for k in range(4)] == [0xF4, 0x33, 0x82, 0x11]
    assert [w.cell(SH - 20 - 8 * k) for k in range(4)] == [0xFFFFFFF4, 0x33, 0xFFFFFF82, 0x11]
    cpu = w.main_trace(0)
    row = cpu[2 + 3 * 2 + 1]  # LOADU8 of offset 2: pointer read, word read, write
    assert row[3] == vp.LOADU8 and row[IS_LOAD_U8] == 1 and row[9:26].sum() == 1
    assert channels(row) == [(1, SH - 12, [0, 0, 0x0F, 0xFE]), (1, SH - 4, [0x11, 0x82, 0x33, 0xF4]), (1, SH - 16 - 16, [0, 0, 0, 0x82])]
    row = cpu[2 + 3 * 2 + 2]
    assert row[3] == vp.LOADS8 and row[IS_LOAD_S8] == 1 and channels(row)[2] == (1, SH - 20 - 16, [0xFF, 0xFF, 0xFF, 0x82])


def test_storeu8_into_each_byte_and_into_a_never_written_word():
    w = load(vp.machine_code(vp.store_byte_program()), stack_height=SH)
    # Word::update_byte reverses the cell before it replaces a byte (core.rs:46-57): 11223344 -> 443322AA -> AA22AA44 -> 44AA22AA -> AA22AA44
    assert w.cell(SH - 4) == 0xAA22AA44
    assert w.cell(SH - 24) == 0x0000AA00  # read_or_init: a never-written word reads as 0
    cpu = w.main_trace(0)
    first = cpu[4]  # the first STOREU8: reads [fp-16] (the pointer), [fp-12] (the byte's word), [fp-4] (read_or_init), writes fp-4
    assert first[3] == vp.STOREU8 and first[IS_STORE_U8] == 1 and first[9:26].sum() == 1
    assert channels(first) == [(1, SH - 16, [0, 0, 0x0F, 0xFC]), (1, SH - 4, [0x11, 0x22, 0x33, 0x44]), (1, SH - 4, [0x44, 0x33, 0x22, 0xAA])]
    last = cpu[13]
    assert channels(last)[1] == (1, SH - 24, [0, 0, 0, 0]) and channels(last)[2] == (1, SH - 24, [0, 0, 0xAA, 0])
    d = w.oplog()
    mem = vp.np_u32(d.mem, d.n_mem, 4)
    assert mem[mem[:, 0] == 13].tolist() == [[13, SH - 28, SH - 23, 0], [13, SH - 12, 0xAA, 0], [13, SH - 24, 0, 0], [13, SH - 24, 0xAA00, 1]]


def test_advice_shorter_than_the_reads():
    w = load(vp.machine_code(vp.advice_program(5)), advice=b"\x01\x80\xff", stack_height=SH)
    assert [w.cell(SH - 4 - 4 * i) for i in range(5)] == [1, 0x80, 0xFF, 0xFFFFFFFF, 0xFFFFFFFF]
    cpu = w.main_trace(0)
    assert cpu[:5, IS_ADVICE].tolist() == [1] * 5 and cpu[5:, IS_ADVICE].max() == 0
    assert channels(cpu[3]) == [(0, 0, [0] * 4), (0, 0, [0] * 4), (1, SH - 16, [255] * 4)]
    e = load(vp.machine_code(vp.echo_program(4)), advice=b"hi!")
    assert e.output() == b"hi!\xff"


def test_vm_errors_carry_pc_and_opcode():
    with pytest.raises(va.VgpuError, match=r"unrecognized opcode 14, pc = 1"):
        load(vp.machine_code([vp.imm32(-4, 1), (14, [0, 0, 0])]))
    with pytest.raises(va.VgpuError, match=r"pc = 1 is beyond the ROM of 1 instructions"):
        load(vp.machine_code([vp.imm32(-4, 1)]))
    with pytest.raises(va.VgpuError, match=r"cycle limit of 100 cycles.*pc = 1, opcode = 6"):
        load(vp.machine_code([vp.imm32(-4, 0), (vp.BNE, [24, -4, 1, 0, 1])]), max_cycles=100)  # a branch to itself
    with pytest.raises(va.VgpuError, match=r"read before write: .*pc = 0, opcode = 11"):
        load(vp.machine_code([(vp.LOADU8, [-4, 0, -8]), (vp.STOP, [])]))
    assert load(vp.machine_code(vp.byte_loop_program(3)), max_cycles=4 + 8 * 3 + 1).cycles == 29
    with pytest.raises(va.VgpuError, match="cycle limit of 28"):
        load(vp.machine_code(vp.byte_loop_program(3)), max_cycles=28)


# ---- the same workload as the built-ins ------------------------------------------------------------------------------------------------
def _same(a, b):
    assert (a.cycles, a.cpu_ops, a.mem_ops, a.add_ops, a.program_len, a.cpu_height) == (b.cycles, b.cpu_ops, b.mem_ops, b.add_ops, b.program_len, b.cpu_height)
    for x, y in zip(a.main_traces(), b.main_traces()):
        assert x.shape == y.shape and np.array_equal(x, y)
    for (c1, m1), (c2, m2) in zip(a.preprocessed(), b.preprocessed()):
        assert c1 == c2 and np.array_equal(m1, m2)
    da, db = a.oplog(), b.oplog()
    assert np.array_equal(vp.np_u32(da.cpu, da.n_cpu, 12), vp.np_u32(db.cpu, db.n_cpu, 12))
    assert np.array_equal(vp.np_u32(da.mem, da.n_mem, 4), vp.np_u32(db.mem, db.n_mem, 4))
    for k in range(4):
        assert np.array_equal(vp.np_u32(da.alu[k], da.n_alu[k], 4), vp.np_u32(db.alu[k], db.n_alu[k], 4))
        assert np.array_equal(vp.np_u32(da.alu2[k], da.n_alu2[k], 4), vp.np_u32(db.alu2[k], db.n_alu2[k], 4))
    assert int(da.n_static) == int(db.n_static) and (not da.n_static or np.array_equal(vp.np_u32(da.static_cells, da.n_static, 2), vp.np_u32(db.static_cells, db.n_static, 2)))
    assert np.array_equal(vp.np_u32(da.output, da.n_output, 2), vp.np_u32(db.output, db.n_output, 2)) and a.output() == b.output()


@pytest.mark.parametrize("make", [lambda: va.Workload.fib(25), lambda: va.Workload.alu(100), lambda: va.Workload.named("left_imm_ops"),
                                  lambda: va.Workload.named("signed_inequality"), lambda: va.Workload.named("loadfp"),
                                  lambda: va.Workload.named("mixed_ops:40")])
def test_machine_code_of_a_builtin_is_the_same_workload(make):
    w = make()
    _same(load(vp.machine_code_of(w), stack_height=SH), w)


def test_elf_with_static_data_is_the_static_data_workload():
    w = va.Workload.named("static_data")
    img = vp.elf([(".text", vp.SHT_PROGBITS, 6, 0, vp.machine_code_of(w)), (".data", vp.SHT_PROGBITS, 3, 0x10, bytes([0, 0, 0, 0x25, 0, 0, 0, 0x32]))])
    _same(load(img, stack_height=SH), w)


def test_verify_cli_takes_a_program_file(tmp_path):
    from valida_amd import verify_cli

    exe = tmp_path / "fib25.bin"
    exe.write_bytes(vp.machine_code_of(va.Workload.fib(25)))
    proof = os.path.join(ROOT, "tests", "golden", "fib25_q4_proof.cbor")
    assert verify_cli.main([proof, "--program-file", str(exe), "--queries", "4"]) == 0
    other = tmp_path / "fib26.bin"
    other.write_bytes(vp.machine_code_of(va.Workload.alu(3)))
    assert verify_cli.main([proof, "--program-file", str(other), "--queries", "4"]) == 1  # another ROM: another preprocessed commitment
    assert verify_cli.main([proof, "--program-file", str(tmp_path / "missing"), "--queries", "4"]) == 1


# ---- verdicts ----------------------------------------------------------------------------------------------------------------------------
# The reference's CPU AIR constrains none of the four flags except is_advice in the pc increment (cpu/src/stark.rs:70-240): READ_ADVICE,
# LOADU8 and LOADS8 with complete chips are accepted.  A STOREU8 logs three reads into two read channels (cpu/src/lib.rs:253-296): one read
# never reaches the memory bus, whose cumulative sums then do not cancel.
VERDICT_PROGRAMS = [("byte_loads", vp.byte_loads_program(), b"", True), ("advice", vp.advice_program(5), b"\x01\x80\xff", True),
                    ("byte_loop", vp.byte_loop_program(50), bytes(range(30)), True), ("store_byte", vp.store_byte_program(), b"", False)]


@pytest.mark.parametrize("name,prog,advice,accepted", VERDICT_PROGRAMS, ids=[v[0] for v in VERDICT_PROGRAMS])
def test_verdicts_of_the_new_instructions(rc, machine, name, prog, advice, accepted):
    w = load(vp.machine_code(prog), advice=advice)
    mt, prep = w.main_traces(), w.preprocessed()
    proof = po.prove_basic(mt, prep[0][1], prep[1][1], rc)
    ours = va.verify(machine, rc, proof.words, va.host_commit_root([m for _, m in prep], rc))
    oracle = po.verify_basic(prep[0][1], prep[1][1], proof.words, rc)
    assert (ours is None) == (oracle is None) == accepted, (ours, oracle)
    if not accepted:
        assert "cumulative sums" in ours and "cumulative sums" in oracle


# ---- the kernel source under emulation ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tg_emu():
    src = os.path.join(ROOT, "tests", "emu", "tracegen_emu.cpp")
    out = os.path.join(ROOT, "build", "libtracegenemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp")] + [
        os.path.join(csrc, "kernels", f) for f in ("tracegen.hip", "launch.hpp", "device_common.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.mark.parametrize("name,prog,advice", [(v[0], v[1], v[2]) for v in VERDICT_PROGRAMS] + [("echo", vp.echo_program(3), b"ab")])
def test_k_tracegen_cpu_source_matches_the_host_cpu_trace(tg_emu, name, prog, advice):
    w = load(vp.machine_code(prog), advice=advice, stack_height=SH)
    d = w.oplog()
    want = w.main_trace(0)
    got = np.zeros_like(want)
    c_u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = tg_emu.emu_tracegen_cpu(ctypes.cast(d.cpu, c_u32p), ctypes.c_uint64(d.n_cpu), ctypes.cast(d.mem, c_u32p), ctypes.c_uint64(d.n_mem),
                                 ctypes.c_uint64(want.shape[0]), got.ctypes.data_as(c_u32p))
    assert rc == 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


# ---- operation-log checks --------------------------------------------------------------------------------------------------------------
def test_upload_validation_accepts_the_new_kinds_and_refuses_kind_15():
    for prog in (vp.byte_loads_program(), vp.store_byte_program(), vp.advice_program(2)):
        w = load(vp.machine_code(prog), advice=b"x", stack_height=SH)
        d = w.oplog()
        kinds = set(vp.np_u32(d.cpu, d.n_cpu, 12)[:, 8].tolist())
        assert kinds & {11, 12, 13, 14}
        va.validate_oplog(d)
    cpu = vp.np_u32(d.cpu, d.n_cpu, 12)
    cpu[0, 8] = 15
    bad = va.OplogDesc()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(d), ctypes.sizeof(d))
    bad.cpu = cpu.ctypes.data
    with pytest.raises(va.VgpuError, match="cpu record 0 is malformed"):
        va.validate_oplog(bad)
    cpu[0, 8], cpu[0, 2] = 7, 9  # a BUS record carrying READ_ADVICE's opcode
    with pytest.raises(va.VgpuError, match="no bus operation"):
        va.validate_oplog(bad)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=300)


def test_cli_run_writes_the_output_bytes(tmp_path):
    exe, adv, out = tmp_path / "echo.bin", tmp_path / "advice", tmp_path / "out"
    exe.write_bytes(vp.machine_code(vp.echo_program(6)))
    adv.write_bytes(b"hello")
    r = _cli("run", exe, out, adv)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b"hello\xff"
    r = _cli("run", exe, out)  # no advice file: an empty tape
    assert r.returncode == 0 and out.read_bytes() == b"\xff" * 6
    bad = tmp_path / "bad.bin"
    bad.write_bytes(vp.machine_code([(14, [])]))
    r = _cli("run", bad, out)
    assert r.returncode == 1 and "unrecognized opcode 14, pc = 0" in r.stderr
    r = _cli("run", exe, out, "--max-cycles", "5")
    assert r.returncode == 1 and "cycle limit" in r.stderr


def test_cli_prove_without_a_gpu_fails_with_a_message(tmp_path):
    import conftest

    if conftest.has_gpu():
        pytest.skip("this box has a GPU (tests/test_executable_gpu.py proves through the CLI)")
    exe = tmp_path / "loads.bin"
    exe.write_bytes(vp.machine_code(vp.byte_loads_program()))
    r = _cli("prove", exe, tmp_path / "proof.cbor")
    assert r.returncode == 1 and r.stderr.startswith("prove: ") and not (tmp_path / "proof.cbor").exists()
