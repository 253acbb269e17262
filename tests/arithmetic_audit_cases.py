"""Inputs the arithmetic audit's CPU and GPU tests share: the VM witnesses of the BasicMachine, tiny purpose-built programs, the planted
quotient, the captured `alu` machine (one chip: a receive on global bus 0 of 13 bare columns opcode, x[0..3], y[0..3], z[0..3] with count
column 13; `alu_pair` adds a second chip that SENDS the same shape), the edge corpus planted at any height, and synthetic traces.  Everything
is built in numpy and plain integers, nothing is random beyond fixed seeds."""
import numpy as np

import arithmetic_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from domain_audit_cases import capture

P = va.P
CPU, MEM, DIV, SHIFT, COM = 0, 2, 6, 7, 9
BUS = 0
WIDTH = 14
HEIGHTS = (1, 63, 64, 65, 255, 256, 257)
WORDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x00FF00FF)
M32 = 0xFFFFFFFF


def word_bytes(v):
    return [(v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255]


# ---- the captured machines ------------------------------------------------------------------------------------------------------------------
def _record(is_send, fields=13, bus=BUS):
    return (is_send, True, bus, [[(k, 1)] for k in range(fields)], [(13, 1)])


_machines = {}


def machine(kind="alu"):
    """alu: one receiving chip; alu_pair: the receiving chip and a sending chip `tx`; short: a receive of 12 fields; tx_only: only the sender;
    clk: a receive of 14 fields (the last one ignored, as the clk of output and cpu)."""
    if kind not in _machines:
        _machines[kind] = {"alu": lambda: capture([(b"alu", WIDTH, [_record(False)])]),
                           "alu_pair": lambda: capture([(b"alu", WIDTH, [_record(False)]), (b"tx", WIDTH, [_record(True)])]),
                           "short": lambda: capture([(b"short", WIDTH, [_record(False, fields=12)])]),
                           "tx_only": lambda: capture([(b"tx", WIDTH, [_record(True)])]),
                           "clk": lambda: capture([(b"alu", WIDTH, [(False, True, BUS, [[(k, 1)] for k in range(13)] + [[(0, 1)]], [(13, 1)])])])}[kind]()
    return _machines[kind]


def record(opcode, x, y, z, count=1):
    """A row of the `alu` chip from the three words."""
    return [opcode % P] + word_bytes(x) + word_bytes(y) + word_bytes(z) + [count % P]


def honest(opcode, x, y, count=1):
    """The record the opcode computes (z = 0 where the operation is undefined)."""
    idx = opcode - 100
    undefined = (idx in (ref.DIV, ref.SDIV) and y == 0) or (idx == ref.SDIV and (x, y) == (0x80000000, M32)) or (idx in (ref.SHL, ref.SHR, ref.SRA) and y >= 32)
    return record(opcode, x, y, 0 if undefined else ref.expected(idx, x, y), count)


def corpus():
    """The edge corpus as rows of the `alu` chip: every opcode over WORDS x WORDS (honest results; every fifth record with one byte of z changed;
    where SDIV by 2^k or SHR meets a negative x also the record that holds the arithmetic shift), the shift amounts 0, 1, 31, 32, 255, 256, the
    divisors 0, 1, -1 and 2^k for k = 0, 1, 31, a field of 256 and of p - 1 in each of the twelve positions, the opcodes 99, 100, 118, 119, 300
    and p - 1, and the counts 0, 1, 2 and p - 1."""
    rows, k = [], 0
    for opcode in range(100, 119):
        for x in WORDS:
            for y in WORDS:
                r = honest(opcode, x, y)
                if k % 5 == 4:
                    r[9 + k % 4] ^= 1 + k % 7
                k += 1
                rows.append(r)
    for opcode in (105, 106, 113):
        for x in WORDS:
            for y in (0, 1, 31, 32, 255, 256):
                rows.append(honest(opcode, x, y))
                if opcode == 106 and y < 32:
                    rows.append(record(106, x, y, ref.sra(x, y)))  # the SRA row the reference logs as Shr32
    for opcode in (103, 110):
        for x in WORDS:
            for y in (0, 1, M32, 2, 0x80000000):
                rows.append(honest(opcode, x, y))
                if opcode == 110 and y and y & (y - 1) == 0:
                    rows.append(record(110, x, y, ref.sra(x, y.bit_length() - 1)))  # shift's delegation of SRA to div
    for j in range(12):
        for v in (256, P - 1):
            r = honest(100 + j, 0x01020304, 0x00000005)
            r[1 + j] = v
            rows.append(r)
    for opcode in (99, 100, 118, 119, 300, P - 1):
        rows.append(record(opcode, 7, 9, 1))
    for count in (0, 1, 2, P - 1):
        rows.append(record(102, 3, 5, 16, count))  # a wrong product: a finding iff live
    return np.array(rows, dtype=np.uint32)


def padded(rows):
    """The rows in a trace of the next power-of-two height; the rows behind them are dead (count 0) but hold a wrong sum."""
    n = 1
    while n < len(rows):
        n *= 2
    t = np.tile(np.array(record(100, 1, 1, 3, 0), dtype=np.uint32), (n, 1))
    t[:len(rows)] = rows
    return t


def edge_trace(h, seed=7):
    """h records of the corpus (a fixed permutation of it, cycled), planted on the first h rows."""
    c = corpus()
    perm = np.random.RandomState(seed).permutation(len(c))
    return padded(c[perm[np.arange(h) % len(c)]])


def full_corpus_trace():
    return padded(corpus())


def many_findings(k=300, n=1024):
    """k wrong sums on the even rows and k SHR records that hold the arithmetic shift on the odd ones."""
    rows = []
    for r in range(k):
        rows.append(record(100, r, 1, r + 2))
        rows.append(record(106, 0x80000000 + r, 4, ref.sra(0x80000000 + r, 4)))
    t = padded(rows)
    assert t.shape[0] == n
    return t


def synthetic(n, seed=5):
    """n live records (n a power of two) of ADD, SUB, MUL, AND, OR, XOR, LT, NE, MULHU and MULHS over fixed-seed words, honest but for the first
    and the last row of every workgroup of 256, whose low result byte is changed: 2 n / 256 wrong results (n = 1: none)."""
    rs = np.random.RandomState(seed)
    x, y = rs.randint(0, 1 << 32, size=n, dtype=np.uint64), rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
    ops = np.array([100, 101, 102, 107, 108, 109, 104, 111, 112, 114])[np.arange(n) % 10]
    m = np.uint64(M32)
    z = np.select([ops == 100, ops == 101, ops == 102, ops == 107, ops == 108, ops == 109, ops == 104, ops == 111],
                  [(x + y) & m, (x - y) & m, (x * y) & m, x & y, x | y, x ^ y, (x < y).astype(np.uint64), (x != y).astype(np.uint64)], default=(x * y) >> np.uint64(32))
    t = np.zeros((n, WIDTH), dtype=np.uint32)
    t[:, 0], t[:, 13] = ops, 1
    for k, v in enumerate((x, y, z)):
        for j in range(4):
            t[:, 1 + 4 * k + j] = (v >> np.uint64(24 - 8 * j)) & np.uint64(255)
    if n >= 256:
        rows = np.arange(n)
        t[(rows % 256 == 0) | (rows % 256 == 255), 12] ^= 1
    return t


# ---- the BasicMachine's witnesses ---------------------------------------------------------------------------------------------------------
def div_program(x=100, y=7):
    return [vp.imm32(-4, x), vp.imm32(-8, y), (vp.DIV32, [-12, -4, -8, 0, 0]), (vp.STOP, [])]


def op_program(opcode, x, y):
    """imm32 x; imm32 y; the operation into fp - 12; stop."""
    return [vp.imm32(-4, x), vp.imm32(-8, y), (opcode, [-12, -4, -8, 0, 0]), (vp.STOP, [])]


VM = {"fib25": lambda: va.Workload.fib(25), "fib582": lambda: va.Workload.fib(582), "alu100": lambda: va.Workload.alu(100),
      "signed_inequality": lambda: va.Workload.named("signed_inequality"), "left_imm_ops": lambda: va.Workload.named("left_imm_ops")}
# beside the five: thirteen opcodes run in mixed_ops, and the reference's div and com traces hold no operands (div/mod.rs:84-103, com/mod.rs:87-103)
EXTRA = {"mixed_ops8": lambda: va.Workload.named("mixed_ops:8"), "div_100_7": lambda: va.Workload.from_executable(vp.machine_code(div_program())),
         "mulhs": lambda: va.Workload.from_executable(vp.machine_code(op_program(vp.MULHS32, 0xFFFFFFFE, 3))),
         "sra": lambda: va.Workload.from_executable(vp.machine_code(op_program(vp.SRA32, 0xFFFFFFF5, 1)))}
_witness = {}


def workload(name):
    if name not in _witness:
        w = (VM.get(name) or EXTRA[name])()
        _witness[name] = (w, w.main_traces(), w.preprocessed())
    return _witness[name][0]


def witness(name):
    """(main traces, preprocessed)"""
    workload(name)
    return _witness[name][1:]


def completed_div(x=100, y=7):
    """The witness of div_program with the div chip's row completed: the reference's generator writes only the opcode flag there, so the honest
    row (x, y, x / y) is written here as a finished div chip would.  (main, prep, the cpu row of the division)."""
    main, prep = witness("div_100_7") if (x, y) == (100, 7) else (lambda w: (w.main_traces(), w.preprocessed()))(va.Workload.from_executable(vp.machine_code(div_program(x, y))))
    main = [m.copy() for m in main]
    main[DIV][0, 0:12] = word_bytes(x) + word_bytes(y) + word_bytes(x // y)
    cpu_row = int(np.flatnonzero(main[CPU][:, 3] == vp.DIV32)[0])
    return main, prep, cpu_row


def planted_quotient(x=100, y=7, q=15):
    """completed_div with the quotient replaced by q, byte for byte, in the three places that hold it: the div chip's row (columns 8..11), the
    cpu's write channel (columns 46..49: the value of its third memory send and of its general-bus send) and the memory table's write row."""
    main, prep, cpu_row = completed_div(x, y)
    old, new = word_bytes(x // y), word_bytes(q)
    main[DIV][0, 8:12] = new
    assert main[CPU][cpu_row, 46:50].tolist() == old
    main[CPU][cpu_row, 46:50] = new
    mem = main[MEM]
    clk = int(main[CPU][cpu_row, 0])
    rows = np.flatnonzero((mem[:, 8] == 1) & (mem[:, 5] == clk) & (mem[:, 1:5] == np.array(old)).all(axis=1))
    assert len(rows) == 1
    mem[rows[0], 1:5] = new
    return main, prep, cpu_row
