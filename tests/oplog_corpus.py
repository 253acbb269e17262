"""Operation logs at the edges of the device trace generators (valida_amd/csrc/kernels/tracegen.hip): synthetic logs built directly as arrays, each
with a name and the chips it is generated for, and the named boundary vectors the tests assert to be present ("Trace generators at
their edges").  Every log passes validate_oplog.  The expected traces come from tests/tracegen_ref.py, never from the code under test."""
import functools

import numpy as np

import tracegen_ref as tr
from tracegen_ref import P

M32 = 0xFFFFFFFF
# ---- the ALU words ---------------------------------------------------------------------------------------------------------------------
W = [0, 1, 0xFF, 0x100, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, P - 1, P, P + 1,
     0x00FF00FF, 0xFF00FF00, 0x01010101, 0xFEFEFEFE]
SHIFT_AMOUNTS = [0, 1, 7, 8, 15, 16, 24, 31]
# cpu log: immediates, frame pointers and memory addresses; operands
EDGE_U32 = [0, 1, P - 1, P, P + 1, 0x80000000, 0xFFFFFFFF]
EDGE_I32 = [0, 1, -1, 2**31 - 1, -2**31, -P, P - 1]
# constants of tracegen.hip the cases are built around
PC_LDS_BINS, PC_BLOCK_ITEMS, RS_BLOCK, RANGE_GRID_CAP, MUL_MIN_LENGTH = 4096, 256 * 16, 8192, 1024, 1024


def s32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def _tdiv(b, c):  # i32 division truncates toward zero and wraps on overflow
    q = abs(b) // abs(c)
    return (q if (b < 0) == (c < 0) else -q) & M32


# the true 32-bit result of every ALU opcode; a division by zero has no result in the reference (the VM panics) and the div chip's rows do not
# read a, so the log carries all ones there
RESULT = {
    tr.ADD32: lambda b, c: (b + c) & M32, tr.SUB32: lambda b, c: (b - c) & M32,
    tr.LT32: lambda b, c: int(b < c), tr.LTE32: lambda b, c: int(b <= c), tr.SLT32: lambda b, c: int(s32(b) < s32(c)), tr.SLE32: lambda b, c: int(s32(b) <= s32(c)),
    tr.AND32: lambda b, c: b & c, tr.OR32: lambda b, c: b | c, tr.XOR32: lambda b, c: b ^ c,
    tr.MUL32: lambda b, c: (b * c) & M32, tr.MULHU32: lambda b, c: (b * c) >> 32, tr.MULHS32: lambda b, c: ((s32(b) * s32(c)) >> 32) & M32,
    tr.DIV32: lambda b, c: b // c if c else M32, tr.SDIV32: lambda b, c: _tdiv(s32(b), s32(c)) if c else M32,
    tr.NE32: lambda b, c: int(b != c), tr.EQ32: lambda b, c: int(b == c),
    tr.SHL32: lambda b, c: (b << c) & M32, tr.SHR32: lambda b, c: b >> c, tr.SRA32: lambda b, c: (s32(b) >> c) & M32,
}
# the opcodes of each ALU log, in the order of vgpu_oplog_desc_t: alu = add, sub, lt, bitwise; alu2 = mul, div, shift, com
ALU_OPCODES = [[tr.ADD32], [tr.SUB32], [tr.LT32, tr.LTE32, tr.SLT32, tr.SLE32], [tr.AND32, tr.OR32, tr.XOR32]]
ALU2_OPCODES = [[tr.MUL32, tr.MULHS32, tr.MULHU32], [tr.DIV32, tr.SDIV32], [tr.SHL32, tr.SHR32, tr.SRA32], [tr.NE32, tr.EQ32]]
ALU_CHIPS = (tr.ADD, tr.SUB, tr.LT, tr.BITWISE, tr.MUL, tr.DIV, tr.SHIFT, tr.COM)


def alu_ops(opcodes, seconds=None):
    """Every ordered pair (b, c) of W (or b in W, c in `seconds`) for every opcode, the opcode varying fastest so that a prefix holds them all."""
    return np.array([[op, RESULT[op](b, c), b, c] for b in W for c in (seconds or W) for op in opcodes], dtype=np.int64)


class Case:
    def __init__(self, name, log, chips):
        self.name, self.log, self.chips = name, log, tuple(chips)

    def __repr__(self):
        return self.name


def cpu_record(pc=0, fp=0, opcode=tr.STOP, operands=(0, 0, 0, 0, 0), kind=tr.K_STOP, has_imm=0, imm=0, mem_first=0):
    return [pc, fp, opcode] + [int(x) & M32 for x in operands] + [kind, has_imm, imm, mem_first]


STOP_ONLY = [cpu_record()]  # the smallest cpu log validate_oplog takes: one STOP at pc 0


def alu_cases():
    full = [alu_ops(o) for o in ALU_OPCODES]
    full2 = [alu_ops(o, SHIFT_AMOUNTS if o[0] == tr.SHL32 else None) for o in ALU2_OPCODES]
    out = [Case("alu_all_pairs", tr.OpLog(STOP_ONLY, alu=full, alu2=full2, rom_len=1), ALU_CHIPS)]
    for n in (0, 1, 256, 257):  # 256 is an exact power of two (no padding row), 257 a power of two plus one
        out.append(Case("alu_len_%d" % n, tr.OpLog(STOP_ONLY, alu=[a[:n] for a in full], alu2=[a[:n] for a in full2], rom_len=1), ALU_CHIPS))
    return out


# ---- cpu logs --------------------------------------------------------------------------------------------------------------------------
BUS_OPCODES = list(range(tr.ADD32, tr.SLE32 + 1)) + [tr.WRITE]
# (kind, opcode, has_imm, reads, writes): every Operation variant, with the immediates only where the variant carries Some(imm); the shapes cover
# 0, 1, 2, 3 and 4 memory operations per cycle, the four-operation one being STOREU8's three reads and a write
CPU_SHAPES = [
    (tr.K_BUS, None, 0, 2, 1), (tr.K_BUS, None, 1, 1, 1), (tr.K_BUS_LEFT_IMM, None, 1, 1, 1), (tr.K_STORE32, 2, 0, 2, 1), (tr.K_LOAD32, 1, 0, 2, 1),
    (tr.K_JAL, 3, 0, 0, 1), (tr.K_JALV, 4, 0, 2, 1), (tr.K_BEQ, 5, 0, 2, 0), (tr.K_BEQ, 5, 1, 1, 0), (tr.K_BNE, 6, 0, 2, 0), (tr.K_BNE, 6, 1, 1, 0),
    (tr.K_IMM32, 7, 0, 0, 1), (tr.K_STOP, 8, 0, 0, 0), (tr.K_LOADFP, 10, 0, 0, 1), (tr.K_LOAD_U8, 11, 0, 2, 1), (tr.K_LOAD_S8, 12, 0, 2, 1),
    (tr.K_STORE_U8, 13, 0, 3, 1), (tr.K_READ_ADVICE, 9, 0, 0, 1), (tr.K_BUS, None, 0, 0, 0), (tr.K_BUS, None, 0, 2, 0),
]
# the second read word against the first: equal, or different in exactly one byte (each position), or unrelated
READ_PAIR_MASKS = [0, 0xFF000000, 0x00010000, 0x00008000, 0x00000001, None]
CPU_ROM_LEN = 64


def cpu_log(n, seed):
    """n cycles walking CPU_SHAPES; immediates, frame pointers, addresses and operands drawn from the edge sets; the memory records carry the
    cycle as their clk."""
    rng = np.random.default_rng(seed)
    pick = lambda s: int(s[rng.integers(len(s))])
    cpu, mem = [], []
    for i in range(n):
        kind, opcode, has_imm, reads, writes = CPU_SHAPES[i % len(CPU_SHAPES)]
        if opcode is None:
            opcode = BUS_OPCODES[(i // len(CPU_SHAPES)) % len(BUS_OPCODES)]
        imm = pick(EDGE_U32 + W)
        cpu.append(cpu_record(i % CPU_ROM_LEN, pick(EDGE_U32), opcode, [pick(EDGE_I32) for _ in range(5)], kind, has_imm, imm, len(mem)))
        first = pick(W + EDGE_U32)
        mask = READ_PAIR_MASKS[(i // 3) % len(READ_PAIR_MASKS)]
        other = pick(W) if mask is None else first ^ mask
        if has_imm and (i // len(CPU_SHAPES)) % 2:  # the read beside an immediate: the immediate's own word on every other lap (diff = 0)
            first = imm
        values = [first, other, pick(W)]
        for k in range(reads):
            mem.append([i, pick(EDGE_U32), values[k], 0])
        for _ in range(writes):
            mem.append([i, pick(EDGE_U32), pick(W), 1])
    return tr.OpLog(cpu, mem, rom_len=CPU_ROM_LEN)


def cpu_cases():
    return [Case("cpu_n%d" % n, cpu_log(n, 100 + n), (tr.CPU, tr.PROGRAM, tr.MEM, tr.RANGE)) for n in (1, 255, 256, 257, 4096, 4097)]


# ---- program histogram -----------------------------------------------------------------------------------------------------------------
def pc_log(pcs, rom_len):
    cpu = np.zeros((len(pcs), 12), dtype=np.int64)
    cpu[:, tr.C_PC], cpu[:, tr.C_OPCODE], cpu[:, tr.C_KIND] = pcs, 7, tr.K_IMM32
    cpu[-1, tr.C_OPCODE], cpu[-1, tr.C_KIND] = tr.STOP, tr.K_STOP
    return tr.OpLog(cpu, rom_len=rom_len)


def program_cases():
    chips = (tr.PROGRAM, tr.CPU, tr.RANGE)
    sweep = lambda n: np.arange(n)
    hot_global = np.concatenate([np.full(5000, 4999), [4095, 4096], np.arange(8192 - 5003) % 5000, [4999]])  # 8192 fetches: no padding, last pc on the global path
    hot_lds = np.concatenate([np.full(5000, 7), [4095, 4096, 4999, 7]])                                      # 5004 fetches: padding at a pc on the LDS path
    return [
        Case("pc_rom1", pc_log(np.zeros(5, dtype=np.int64), 1), chips),
        Case("pc_rom4095_sweep", pc_log(sweep(4095), 4095), chips),   # last pc 4094 (LDS), one padding row
        Case("pc_rom4096_sweep", pc_log(sweep(4096), 4096), chips),   # last pc 4095 (LDS), padded_n == n, the log ends on a 4096-item block
        Case("pc_rom4097_sweep", pc_log(sweep(4097), 4097), chips),   # last pc 4096 (global), 4095 padding rows
        Case("pc_rom5000_hot_global", pc_log(hot_global, 5000), chips),
        Case("pc_rom5000_hot_lds", pc_log(hot_lds, 5000), chips),
        Case("pc_rom5000_last", pc_log(np.concatenate([sweep(5000), [4999]]), 5000), chips),  # fetches at rom_len - 1, padding there too
    ]


# ---- range histogram -------------------------------------------------------------------------------------------------------------------
COUNTED, UNCOUNTED = list(tr.RANGE_CHECKED), [tr.LT32, tr.AND32, tr.SHL32, tr.WRITE]


def range_small_log():
    cpu, mem = [], []

    def cycle(opcode, kind=tr.K_BUS, reads=(), write=None, has_imm=0):
        cpu.append(cpu_record(len(cpu) % CPU_ROM_LEN, 0x1000, opcode, (-4, -8, -12, 0, has_imm), kind, has_imm, 5, len(mem)))
        for v in reads:
            mem.append([len(cpu) - 1, 0x0FF8, v, 0])
        if write is not None:
            mem.append([len(cpu) - 1, 0x0FFC, write, 1])

    cycle(tr.ADD32)                                        # a counted op with no memory operation as the FIRST record: end == 0
    for k, op in enumerate(COUNTED):
        cycle(op, reads=(W[k], W[k + 7]), write=W[2 * k + 3])
        cycle(op, kind=tr.K_BUS_LEFT_IMM, reads=(W[k],), write=0x01020304 * (k + 1), has_imm=1)
    for k, op in enumerate(UNCOUNTED):
        cycle(op, reads=(1, 2), write=0xA0B0C0D0 + k)      # never counted
    cycle(tr.SUB32, reads=(0x11111111, 0x22222222))        # a counted op whose cycle ends in a read
    cycle(tr.MUL32, reads=(3,))
    for _ in range(300):                                   # one byte value hit 1200 times in a block
        cycle(tr.ADD32, reads=(0,), write=0x00000000, has_imm=1)
    for _ in range(300):
        cycle(tr.SUB32, reads=(0,), write=0xFFFFFFFF, has_imm=1)
    cpu.append(cpu_record(5, 0x1000, 7, (-4, 1, 2, 3, 4), tr.K_IMM32, 0, 0, len(mem)))
    mem.append([len(cpu) - 1, 0x0FFC, 0x77777777, 1])      # a write of another instruction: not a bus op
    cycle(tr.DIV32)                                        # a counted op with no memory operation as the LAST record
    return tr.OpLog(cpu, mem, rom_len=CPU_ROM_LEN)


def range_stride_log():
    """2^18 + 300 bus cycles of one write each: more records than RANGE_GRID_CAP blocks of 256 threads take in one step, so the histogram
    kernel's grid-stride loop runs twice for the first 300 threads."""
    n = (1 << 18) + 300
    rng = np.random.default_rng(18)
    i = np.arange(n)
    cpu = np.zeros((n, 12), dtype=np.int64)
    ops = np.array(COUNTED + UNCOUNTED)
    cpu[:, tr.C_PC], cpu[:, tr.C_FP], cpu[:, tr.C_OPCODE], cpu[:, tr.C_KIND], cpu[:, tr.C_MEM_FIRST] = i % 5000, 0x1000, ops[i % len(ops)], tr.K_BUS, i
    mem = np.stack([i, np.full(n, 0x0FFC), rng.integers(0, 1 << 32, size=n), np.ones(n, dtype=np.int64)], axis=1)
    mem[-300:, 2] = 0xFE00FE01  # the records of the second stride are told apart from the rest
    return tr.OpLog(cpu, mem, rom_len=5000)


def range_cases():
    return [Case("range_small", range_small_log(), (tr.RANGE, tr.CPU, tr.MEM, tr.PROGRAM)),
            Case("range_stride", range_stride_log(), (tr.RANGE, tr.PROGRAM))]


# ---- memory log ------------------------------------------------------------------------------------------------------------------------
MEM_EDGE_ADDRS = [0x80000000, 0xFFFFFFFC, P - 1, P, 0, 4, 0x01020304, 0xFEDCBA98]
STATIC3 = [[4, 0x01020304], [P + 8, 0xFFFEFD00], [0xFFFFFFF0, 0x000000FF]]  # ascending addresses, one at or above p
HOT_ADDR, BLOCK_ADDR, FAR_ADDR = 0x80000000, 0xFFFFFFFC, P


def mem_log(n, n_static, seed):
    """n memory records, clocks non-decreasing (three per cycle); addresses vary in all four bytes.  Where n allows: records 0-63 (one wave)
    share HOT_ADDR, 64-127 have 64 distinct low digits, 261 / 326 / 391 / 456 (the four waves of the second 256-record round) share BLOCK_ADDR,
    and FAR_ADDR returns at distances above RS_BLOCK."""
    rng = np.random.default_rng(seed)
    addr = rng.integers(0, 1 << 32, size=n, dtype=np.int64)
    edge = rng.integers(0, 4, size=n) == 0
    addr[edge] = np.array(MEM_EDGE_ADDRS)[rng.integers(0, len(MEM_EDGE_ADDRS), size=int(edge.sum()))]
    addr[:64] = HOT_ADDR
    addr[64:128] = (0x7F3C5500 + np.arange(64) * 3)[: max(0, min(n, 128) - 64)]
    for k in (261, 326, 391, 456):
        if k < n:
            addr[k] = BLOCK_ADDR
    for k in range(130, n, RS_BLOCK + 1):
        addr[k] = FAR_ADDR
    mem = np.stack([np.arange(n) // 3, addr, rng.integers(0, 1 << 32, size=n, dtype=np.int64), rng.integers(0, 2, size=n)], axis=1)
    return tr.OpLog(STOP_ONLY, mem, static=STATIC3[:n_static], rom_len=1)


MEM_LENGTHS = (0, 1, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 37)


def mem_cases():
    chips = (tr.MEM, tr.STATIC_DATA)
    out = [Case("mem_n%d_static%d" % (n, s), mem_log(n, s, 7 * n + s), chips) for n in MEM_LENGTHS for s in (0, 3)]
    out.append(Case("mem_n8189_static3", mem_log(8189, 3, 5), chips))  # n_static + n_mem an exact power of two
    return out


# ---- output tape -----------------------------------------------------------------------------------------------------------------------
def out_log(entries):
    return tr.OpLog(STOP_ONLY, output=entries, rom_len=1)


def output_cases():
    n = 5
    gaps = [0, n - 1, n, 3 * n + n - 1]
    clk5 = np.concatenate([[1000], 1000 + np.cumsum(gaps)])
    tapes = {
        "out_n0": [],
        "out_n1": [[P + 5, 255]],                                  # a single entry: the final row alone
        "out_n2_gap0": [[7, 0], [7, 255]],                         # two rows: an exact power of two
        "out_n2_gap_n_minus_1": [[7, 1], [8, 2]],
        "out_n2_gap_n": [[7, 3], [9, 4]],
        "out_n5_gaps": [[int(c), b] for c, b in zip(clk5, (0, 255, 1, 128, 254))],          # windows of 1, 1, 2, 4 rows
        "out_n5_pow2": [[3, 9], [3, 8], [4, 7], [9, 6], [60, 5]],                           # windows of 1, 1, 2, 11 rows + the last: 16
        "out_n5_long": [[0, 0], [2, 255], [5 * 1000 + 2, 17], [5 * 1000 + 2, 0], [5 * 1000 + 8, 255]],  # one window of 1001 rows
        "out_n2_clk_near_p": [[P - 3, 255], [P + 5, 0]],           # clk_1 + table_len (k + 1) passes p inside the window
    }
    return [Case(name, out_log(t), (tr.OUTPUT,)) for name, t in tapes.items()]


# ---- static data -----------------------------------------------------------------------------------------------------------------------
def static_cases():
    cells = STATIC3 + [[0xFFFFFFFC, 0x80000000]]
    return [Case("static_%d" % k, tr.OpLog(STOP_ONLY, static=cells[:k], rom_len=1), (tr.STATIC_DATA, tr.MEM)) for k in (0, 1, 3, 4)]


@functools.lru_cache(maxsize=None)
def cases():
    out = alu_cases() + cpu_cases() + program_cases() + range_cases() + mem_cases() + output_cases() + static_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name, chip):
    """The expected trace of a case, computed once and shared; callers must not write into it."""
    t = tr.generate_trace(case(name).log, chip)
    t.setflags(write=False)
    return t


def case(name):
    return next(c for c in cases() if c.name == name)


# ---- the named boundary vectors: what each name means is a predicate over the corpus, so a thinned corpus fails the presence test ---------
def _alu(k, alu2=False):
    return np.concatenate([(c.log.alu2 if alu2 else c.log.alu)[k] for c in cases()]).astype(np.int64)


def _has(ops, opcode, b, c):
    return bool(((ops[:, 0] == opcode) & (ops[:, 2] == b) & (ops[:, 3] == c)).any())


def _cpu_rows(pred):
    for c in cases():
        if tr.CPU in c.chips:
            cpu, mem = c.log.cpu.astype(np.int64), c.log.mem.astype(np.int64)
            end = np.append(cpu[1:, tr.C_MEM_FIRST], mem.shape[0])
            for i in range(cpu.shape[0]):
                if pred(cpu[i], mem[cpu[i, tr.C_MEM_FIRST]:end[i]]):
                    return True
    return False


def _reads(m):
    return m[m[:, 3] == 0]


def _one_byte(m, k):
    r = _reads(m)
    return r.shape[0] == 2 and (int(r[0, 2]) ^ int(r[1, 2])) & ~(0xFF << (24 - 8 * k)) == 0 and r[0, 2] != r[1, 2]


def _lengths(get):
    return {int(get(c.log)) for c in cases()}


def _pc(name):
    log = case(name).log
    n = log.cpu.shape[0]
    return int(log.cpu[-1, tr.C_PC]), tr.next_pow2(n) - n, n, log


def _mem_addrs(name):
    return case(name).log.mem[:, 1].astype(np.int64)


def _out_rows(name):
    return [int(x) for x in tr.output_window_rows(case(name).log)]


NAMED_VECTORS = {
    # k_tracegen_alu
    "add: a carry produced only by a carry-in (0x0000FFFF + 1)": lambda: _has(_alu(0), tr.ADD32, 0xFFFF, 1),
    "add: carries through every byte (0xFFFFFFFF + 1)": lambda: _has(_alu(0), tr.ADD32, M32, 1),
    "sub: a borrow without an incoming borrow (0x100 - 0xFF, 0 - 1)": lambda: _has(_alu(1), tr.SUB32, 0x100, 0xFF) and _has(_alu(1), tr.SUB32, 0, 1),
    "sub: an incoming borrow into equal bytes (0x10000 - 1)": lambda: _has(_alu(1), tr.SUB32, 0x10000, 1),
    "lt: equal operands, every opcode": lambda: all(_has(_alu(2), op, w, w) for op in ALU_OPCODES[2] for w in (0, M32, 0x80000000)),
    "lt: first difference in byte 0": lambda: _has(_alu(2), tr.LT32, 0x01000000, 0x00FFFFFF),
    "lt: first difference in byte 3": lambda: _has(_alu(2), tr.LT32, 0xFFFFFFFE, 0xFFFFFFFF) and _has(_alu(2), tr.LT32, 0x80000000, 0x80000001),
    "lt: differences in every byte, the first one deciding": lambda: _has(_alu(2), tr.LT32, 0x00FF00FF, 0xFF00FF00) and _has(_alu(2), tr.LT32, 0x01010101, 0xFEFEFEFE),
    "lt: signed compares across the sign bit": lambda: all(_has(_alu(2), op, b, c) for op in (tr.SLT32, tr.SLE32) for b, c in ((0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (M32, 0), (0, M32))),
    "bitwise: all ones against all zeros, every opcode": lambda: all(_has(_alu(3), op, M32, 0) and _has(_alu(3), op, 0x00FF00FF, 0xFF00FF00) for op in ALU_OPCODES[3]),
    "alu words at p - 1, p, p + 1": lambda: all(_has(_alu(0), tr.ADD32, w, w) for w in (P - 1, P, P + 1)),
    "alu log lengths 0, 1, 256, 257": lambda: all({0, 1, 256, 257} <= _lengths(lambda g, k=k: g.alu[k].shape[0]) and {0, 1, 256, 257} <= _lengths(lambda g, k=k: g.alu2[k].shape[0]) for k in range(4)),
    # k_tracegen_alu2
    "shift: amounts 0 and 31, every opcode": lambda: all(_has(_alu(2, True), op, 0x80000001, c) for op in ALU2_OPCODES[2] for c in (0, 31)),
    "shift: TEMP_1 of 7 and a POWER_OF_TWO in each byte": lambda: all(_has(_alu(2, True), tr.SHL32, 1, c) for c in (7, 8, 15, 16, 24, 31)),
    "mul: an empty log (MIN_LENGTH rows of counter) and one above MIN_LENGTH": lambda: 0 in _lengths(lambda g: g.alu2[0].shape[0]) and max(_lengths(lambda g: g.alu2[0].shape[0])) > MUL_MIN_LENGTH,
    "div: division by zero and the signed overflow": lambda: _has(_alu(1, True), tr.DIV32, 1, 0) and _has(_alu(1, True), tr.SDIV32, 0x80000000, M32),
    # k_tracegen_cpu
    "cpu: n_cpu of 1, 255, 256, 257, 4096, 4097": lambda: {1, 255, 256, 257, 4096, 4097} <= {c.log.cpu.shape[0] for c in cases() if tr.CPU in c.chips},
    "cpu: all fifteen kinds": lambda: set(range(15)) <= set(np.concatenate([c.log.cpu[:, tr.C_KIND] for c in cases() if tr.CPU in c.chips]).tolist()),
    "cpu: fp, imm and addr at p - 1, p, p + 1, 2^31, 2^32 - 1": lambda: all(
        _cpu_rows(lambda r, m, v=v: r[tr.C_FP] == v) and _cpu_rows(lambda r, m, v=v: r[tr.C_HAS_IMM] and r[tr.C_KIND] in tr.KINDS_WITH_IMM and r[tr.C_IMM] == v)
        and _cpu_rows(lambda r, m, v=v: bool((m[:, 1] == v).any())) for v in EDGE_U32),
    "cpu: operands INT32_MIN, -1, INT32_MAX, -p, p - 1": lambda: all(_cpu_rows(lambda r, m, v=v: (v & M32) in r[tr.C_OPS:tr.C_OPS + 5]) for v in EDGE_I32),
    "cpu: equal read channels (diff = 0)": lambda: _cpu_rows(lambda r, m: _reads(m).shape[0] == 2 and _reads(m)[0, 2] == _reads(m)[1, 2] and r[tr.C_KIND] == tr.K_BEQ),
    "cpu: an immediate equal to the word read beside it": lambda: _cpu_rows(lambda r, m: r[tr.C_HAS_IMM] and r[tr.C_KIND] in (tr.K_BUS, tr.K_BNE) and _reads(m).shape[0] == 1 and _reads(m)[0, 2] == r[tr.C_IMM]),
    "cpu: read channels that differ in exactly one byte, each position": lambda: all(_cpu_rows(lambda r, m, k=k: _one_byte(m, k)) for k in range(4)),
    "cpu: cycles with 0, 1, 2, 3 and 4 memory operations": lambda: all(_cpu_rows(lambda r, m, k=k: m.shape[0] == k) for k in range(5)),
    "cpu: STOREU8 as three reads, then the write": lambda: _cpu_rows(lambda r, m: r[tr.C_KIND] == tr.K_STORE_U8 and m[:, 3].tolist() == [0, 0, 0, 1]),
    "cpu: a left-immediate bus op with a single read": lambda: _cpu_rows(lambda r, m: r[tr.C_KIND] == tr.K_BUS_LEFT_IMM and r[tr.C_HAS_IMM] and m[:, 3].tolist() == [0, 1]),
    "cpu: a bus cycle with no memory operation": lambda: _cpu_rows(lambda r, m: r[tr.C_KIND] == tr.K_BUS and m.shape[0] == 0),
    # k_tg_pc_histogram
    "pc: rom_len of 1, 4095, 4096, 4097, 5000": lambda: {1, 4095, 4096, 4097, 5000} <= {c.log.rom_len for c in cases() if tr.PROGRAM in c.chips},
    "pc: fetches at 4095, 4096 and rom_len - 1": lambda: {4095, 4096, 4999} <= set(case("pc_rom5000_hot_global").log.cpu[:, tr.C_PC].tolist()),
    "pc: one pc fetched 5000 times, on each path": lambda: int((case("pc_rom5000_hot_global").log.cpu[:, tr.C_PC] == 4999).sum()) >= 5000 and int((case("pc_rom5000_hot_lds").log.cpu[:, tr.C_PC] == 7).sum()) >= 5000,
    "pc: last record below 4096 with padding": lambda: _pc("pc_rom4095_sweep")[0] < PC_LDS_BINS and _pc("pc_rom4095_sweep")[1] > 0,
    "pc: last record below 4096 without padding, on a 4096-item block": lambda: _pc("pc_rom4096_sweep")[0] < PC_LDS_BINS and _pc("pc_rom4096_sweep")[1] == 0 and _pc("pc_rom4096_sweep")[2] % PC_BLOCK_ITEMS == 0,
    "pc: last record at or above 4096 with padding": lambda: _pc("pc_rom4097_sweep")[0] >= PC_LDS_BINS and _pc("pc_rom4097_sweep")[1] > 0,
    "pc: last record at or above 4096 without padding": lambda: _pc("pc_rom5000_hot_global")[0] >= PC_LDS_BINS and _pc("pc_rom5000_hot_global")[1] == 0,
    # k_tg_range_histogram
    "range: every counted and uncounted bus opcode": lambda: set(COUNTED + UNCOUNTED) <= set(case("range_small").log.cpu[:, tr.C_OPCODE].tolist()),
    "range: a counted op with no memory operation first and last": lambda: all(
        case("range_small").log.cpu[i, tr.C_OPCODE] in COUNTED and case("range_small").log.cpu[i, tr.C_MEM_FIRST] == e for i, e in ((0, 0), (-1, case("range_small").log.mem.shape[0]))) and case("range_small").log.cpu[1, tr.C_MEM_FIRST] == 0,
    "range: a counted op whose cycle ends in a read": lambda: any(
        _cpu_rows(lambda r, m, op=op: r[tr.C_OPCODE] == op and r[tr.C_KIND] == tr.K_BUS and m.shape[0] > 0 and m[-1, 3] == 0) for op in COUNTED),
    "range: 300 writes of 0x00000000 and 300 of 0xFFFFFFFF": lambda: all(int(((case("range_small").log.mem[:, 2] == v) & (case("range_small").log.mem[:, 3] == 1)).sum()) >= 300 for v in (0, M32)),
    "range: more records than 1024 blocks of 256 threads": lambda: case("range_stride").log.cpu.shape[0] == (1 << 18) + 300 > RANGE_GRID_CAP * 256,
    # the radix sort
    "mem: n_mem of 0, 1, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 37": lambda: set(MEM_LENGTHS) <= {c.log.mem.shape[0] for c in cases() if c.name.startswith("mem_")},
    "mem: n_static of 0 and 3 at every length": lambda: all(case("mem_n%d_static%d" % (n, s)).log.static.shape[0] == s for n in MEM_LENGTHS for s in (0, 3)),
    "mem: n_static + n_mem an exact power of two": lambda: case("mem_n8189_static3").log.mem.shape[0] + 3 == 8192,
    "mem: addresses 0x80000000, 0xFFFFFFFC, p - 1 and p": lambda: {0x80000000, 0xFFFFFFFC, P - 1, P} <= set(_mem_addrs("mem_n24613_static0").tolist()),
    "mem: every digit of every pass varies": lambda: all(len(set(((_mem_addrs("mem_n24613_static0") >> s) & 255).tolist())) == 256 for s in (0, 8, 16, 24)),
    "mem: 64 equal addresses in one wave": lambda: set(_mem_addrs("mem_n257_static0")[:64].tolist()) == {HOT_ADDR},
    "mem: a wave of 64 distinct low digits": lambda: len(set((_mem_addrs("mem_n257_static0")[64:128] & 255).tolist())) == 64,
    "mem: one address in the four waves of a round": lambda: [int(_mem_addrs("mem_n8191_static0")[k]) for k in (261, 326, 391, 456)] == [BLOCK_ADDR] * 4 and [k % 256 // 64 for k in (261, 326, 391, 456)] == [0, 1, 2, 3],
    "mem: one address at distances above 8192": lambda: int((_mem_addrs("mem_n24613_static0") == FAR_ADDR).sum()) >= 3 and all(_mem_addrs("mem_n24613_static0")[130 + k * (RS_BLOCK + 1)] == FAR_ADDR for k in range(3)),
    # k_tracegen_output and the row0 sums
    "out: n_output of 0, 1, 2, 5": lambda: {0, 1, 2, 5} <= {c.log.output.shape[0] for c in cases() if tr.OUTPUT in c.chips},
    "out: clock gaps of 0, n - 1, n, 3n + n - 1": lambda: _out_rows("out_n5_gaps") == [1, 1, 2, 4] and _out_rows("out_n2_gap0") == [1] and _out_rows("out_n2_gap_n_minus_1") == [1] and _out_rows("out_n2_gap_n") == [2],
    "out: about a thousand dummy rows in one window": lambda: max(_out_rows("out_n5_long")) == 1001,
    "out: a total row count that is an exact power of two": lambda: sum(_out_rows("out_n5_pow2")) + 1 == 16 and sum(_out_rows("out_n2_gap0")) + 1 == 2,
    "out: bytes 0 and 255": lambda: {0, 255} <= set(case("out_n5_gaps").log.output[:, 1].tolist()),
    "out: a clock near p whose dummy rows wrap": lambda: int(case("out_n2_clk_near_p").log.output[0, 0]) < P < int(case("out_n2_clk_near_p").log.output[0, 0]) + 2 * _out_rows("out_n2_clk_near_p")[0],
    # static data
    "static: 0, 1, 3 and 4 cells, one address at or above p": lambda: {0, 1, 3, 4} <= {c.log.static.shape[0] for c in cases() if c.name.startswith("static_")} and bool((case("static_4").log.static[:, 0] >= P).any()),
}


# ---- reference quirks: rules of the reference's generate_trace whose rows fail the reference's own AIR.  Mirrored, not repaired. ---------------
def sub_borrows(b, c):
    """(witness, true): the borrow out of bytes 3, 2, 1 as sub/mod.rs:104-112 writes it (b[k] < c[k], the incoming borrow ignored), and the borrow
    out of bytes 3, 2, 1, 0 of the subtraction itself."""
    byte = lambda w, k: (w >> (24 - 8 * k)) & 255
    witness = [int(byte(b, k) < byte(c, k)) for k in (3, 2, 1)]
    true, carry = [], 0
    for k in (3, 2, 1, 0):
        carry = int(byte(b, k) - carry < byte(c, k))
        true.append(carry)
    return witness, true


def _sub_rule(k):
    # constraint k of the sub AIR (alu_u32/src/sub/stark.rs:31-46) is the byte equation of byte 3 - k.  With w the witness and t the true
    # borrows, the equation of byte 2 holds iff w2 = t2; of byte 1 iff w2 = t2 and w3 = t3 (256 (w3 - t3) = w2 - t2 has no other solution in
    # {-1, 0, 1}); of byte 0, which has no borrow column of its own, iff w3 = t3 and the subtraction does not wrap (t4 = 0).
    def rule(b, c):
        w, t = sub_borrows(b, c)
        return [False, w[1] != t[1], w[1] != t[1] or w[2] != t[2], w[2] != t[2] or t[3] == 1][k]
    return rule


# chip, constraint (the index constraint_audit_host reports), the operations (b, c) whose row fails it, how many rows of alu_all_pairs do, and why
REFERENCE_QUIRKS = [
    dict(chip=tr.SUB, constraint=1, rule=_sub_rule(1), rows=51,
         why="sub/mod.rs:107-109 sets borrow[1] = b[2] < c[2] without the borrow out of byte 3: wrong when that borrow reaches b[2] == c[2]"),
    dict(chip=tr.SUB, constraint=2, rule=_sub_rule(2), rows=85,
         why="sub/mod.rs:110-112 sets borrow[2] = b[1] < c[1] without the incoming borrow; the byte-1 equation also carries a wrong borrow[1]"),
    dict(chip=tr.SUB, constraint=3, rule=_sub_rule(3), rows=217,
         why="sub/stark.rs:43-46 gives the top byte no borrow out, so no b < c (a wrapping b - c, core.rs:121-126) satisfies it; and a wrong borrow[2]"),
]

# ---- VM programs (tests/valida_programs.py) and the verdicts the oracle's verifier returned for the proofs of their traces; `audit` lists what
# constraint_audit_host names on the host traces: (chip, constraint, failing rows).  The stub chips (mul, shift, com: SURVEY.md 0.6) fail their
# AIR on any program that uses them, so alu_edges_borrow_free is rejected too, at mul instead of at sub.
_STUB_AUDIT = [("mul", 0, 67), ("mul", 1, 49), ("shift", 9, 48), ("shift", 10, 48), ("shift", 11, 24), ("shift", 12, 24), ("shift", 13, 48), ("com", 7, 28)]
VM_PROGRAMS = {
    "alu_edges": dict(oracle="out-of-domain constraint mismatch", rejected_at="sub", audit=[("sub", 1, 7), ("sub", 2, 7), ("sub", 3, 11)] + _STUB_AUDIT),
    "alu_edges_borrow_free": dict(oracle="out-of-domain constraint mismatch", rejected_at="mul", audit=_STUB_AUDIT),
    "long_rom": dict(oracle=None, rejected_at=None, audit=[]),
}


def vm_program(name):
    import valida_programs as vp

    return {"alu_edges": vp.alu_edges_program, "alu_edges_borrow_free": lambda: vp.alu_edges_program(borrow_free=True), "long_rom": vp.long_rom_program}[name]()


@functools.lru_cache(maxsize=None)
def vm_workload(name):
    import valida_amd as va
    import valida_programs as vp

    return va.Workload.from_executable(vp.machine_code(vm_program(name)), stack_height=0x1000)
