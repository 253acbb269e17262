"""Valida executables for the executable tests: machine code and ELF images written here with struct, and small new programs that use the
byte and advice instructions (READ_ADVICE, LOADU8, LOADS8, STOREU8).  Nothing here is taken from the reference's test programs."""
import struct

import numpy as np

P = 2013265921
IMM32, LOADFP, STOP, BNE = 7, 10, 8, 6
READ_ADVICE, LOADU8, LOADS8, STOREU8 = 9, 11, 12, 13
ADD32, AND32, WRITE = 100, 107, 300


def machine_code(instrs):
    """24-byte little-endian records: u32 opcode, i32 operands[5] (ProgramROM::from_machine_code)."""
    return b"".join(struct.pack("<I5i", op, *(list(ops) + [0] * (5 - len(ops)))) for op, ops in instrs)


def machine_code_of(workload):
    """The machine code of a built-in workload, rebuilt from its preprocessed ROM (operands stored as field elements)."""
    rom = workload.preprocessed()[0][1]
    return machine_code([(int(r[1]), [int(v) - P if int(v) > P // 2 else int(v) for v in r[2:7]]) for r in rom[: workload.program_len]])


def imm32(a, v):
    return (IMM32, [a, (v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255])


# ---- ELF ---------------------------------------------------------------------------------------------------------------------------------
SHT_PROGBITS, SHT_STRTAB, SHT_NOBITS = 1, 3, 8


def elf(sections, is64=True, e_shnum=None, big_endian=False, elf_class=None):
    """A relocatable-style ELF image with a section table: sections = [(name, sh_type, sh_flags, sh_addr, data bytes or NOBITS size)].
    A null section comes first and .shstrtab last."""
    names = b"\0"
    offs = []
    for name, *_ in sections:
        offs.append(len(names))
        names += name.encode() + b"\0"
    shstr_name = len(names)
    names += b".shstrtab\0"
    ehsize, shentsize = (64, 64) if is64 else (52, 40)
    body = b""
    placed = []  # (name_off, type, flags, addr, offset, size)
    for (name, typ, flags, addr, data), no in zip(sections, offs):
        if typ == SHT_NOBITS:
            placed.append((no, typ, flags, addr, ehsize + len(body), data))
            continue
        while len(body) % 4:
            body += b"\0"
        placed.append((no, typ, flags, addr, ehsize + len(body), len(data)))
        body += data
    placed.append((shstr_name, SHT_STRTAB, 0, 0, ehsize + len(body), len(names)))
    body += names
    while len(body) % 8:
        body += b"\0"
    shoff = ehsize + len(body)
    n = len(placed) + 1
    end = ">" if big_endian else "<"
    if is64:
        sh = [struct.pack(end + "IIQQQQIIQQ", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)]
        sh += [struct.pack(end + "IIQQQQIIQQ", no, t, f, a, o, s, 0, 0, 4, 0) for no, t, f, a, o, s in placed]
    else:
        sh = [struct.pack(end + "IIIIIIIIII", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)]
        sh += [struct.pack(end + "IIIIIIIIII", no, t, f, a, o, s, 0, 0, 4, 0) for no, t, f, a, o, s in placed]
    cls = elf_class if elf_class is not None else (2 if is64 else 1)
    ident = b"\x7fELF" + bytes([cls, 2 if big_endian else 1, 1, 0]) + b"\0" * 8
    shnum = n if e_shnum is None else e_shnum
    if is64:
        hdr = ident + struct.pack(end + "HHIQQQIHHHHHH", 1, 0xF3, 1, 0, 0, shoff, 0, ehsize, 0, 0, shentsize, shnum, n - 1)
    else:
        hdr = ident + struct.pack(end + "HHIIIIIHHHHHH", 1, 0xF3, 1, 0, 0, shoff, 0, ehsize, 0, 0, shentsize, shnum, n - 1)
    assert len(hdr) == ehsize
    return hdr + body + b"".join(sh)


# ---- new programs ------------------------------------------------------------------------------------------------------------------------
DATA_WORD = 0x1182_33F4  # big-endian bytes 11 82 33 F4: little-endian byte offsets 0..3 hold F4, 33, 82 (negative), 11


def byte_loads_program():
    """LOADU8 and LOADS8 of each byte offset 0-3 of the word at fp - 4: unsigned into fp - 16 - 8k, signed into fp - 20 - 8k."""
    p = [imm32(-4, DATA_WORD), (LOADFP, [-8, -4])]  # fp - 8 = the address of the word
    for k in range(4):
        p += [(ADD32, [-12, -8, k, 0, 1]), (LOADU8, [-16 - 8 * k, 0, -12]), (LOADS8, [-20 - 8 * k, 0, -12])]
    return p + [(STOP, [])]


def advice_program(reads):
    """`reads` READ_ADVICE into fp - 4, fp - 8, ..."""
    return [(READ_ADVICE, [-4 - 4 * i]) for i in range(reads)] + [(STOP, [])]


def store_byte_program():
    """STOREU8 of the low byte of fp - 12 (0xAA) into byte offsets 0-3 of the written word at fp - 4, then into byte 1 of the never-written
    word at fp - 24."""
    p = [imm32(-4, 0x11223344), (LOADFP, [-8, -4]), imm32(-12, 0xAA)]
    for k in range(4):
        p += [(ADD32, [-16, -8, k, 0, 1]), (STOREU8, [0, -16, -12])]
    return p + [(LOADFP, [-20, -24]), (ADD32, [-28, -20, 1, 0, 1]), (STOREU8, [0, -28, -12]), (STOP, [])]


def echo_program(n):
    """n times: READ_ADVICE, WRITE its low byte."""
    return [ins for _ in range(n) for ins in ((READ_ADVICE, [-4]), (WRITE, [0, -4, 0, 0, 1]))] + [(STOP, [])]


def byte_loop_program(iters):
    """8 instructions per iteration: an advice read, (i & 3) as the byte offset into the data word, LOADU8 and LOADS8 of that byte, a running
    sum of the unsigned bytes, the counter, the branch (add and bitwise chips beside cpu and memory).  4 + 8 * iters + 1 cycles."""
    loop = 4 * 24
    return [imm32(-4, 0), imm32(-8, DATA_WORD), (LOADFP, [-12, -8]), imm32(-16, 0),
            (READ_ADVICE, [-20]), (AND32, [-24, -4, 3, 0, 1]), (ADD32, [-28, -12, -24]), (LOADU8, [-32, 0, -28]), (LOADS8, [-36, 0, -28]),
            (ADD32, [-16, -16, -32]), (ADD32, [-4, -4, 1, 0, 1]), (BNE, [loop, -4, iters, 0, 1]), (STOP, [])]


# ---- programs at the edges of the ALU chips and of the program chip's histogram (tests/test_tracegen_edges_*.py) -------------------------------
SUB32, MUL32, DIV32, LT32, SHL32, SHR32, OR32, XOR32, SDIV32, NE32, MULHU32, SRA32, MULHS32, LTE32, EQ32, SLT32, SLE32 = 101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117, 118
ALU_EDGE_WORDS = [0, 1, 0xFF, 0x100, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF, P - 1, P, P + 1,
                  0x00FF00FF, 0xFF00FF00, 0x01010101, 0xFEFEFEFE]
# (b, c): carries made by a carry-in, borrows with and without an incoming borrow, equal operands, a first difference in byte 0 and in byte 3,
# differences in every byte, compares across the sign bit, the words around p
ALU_EDGE_PAIRS = [(0xFFFF, 1), (0xFFFFFFFF, 1), (0x00FFFFFF, 1), (0x100, 0xFF), (0, 1), (0x10000, 1), (0x01000000, 1), (0x100, 1), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF),
                  (0x80000000, 0x80000000), (0x01000000, 0x00FFFFFF), (0x00FFFFFF, 0x01000000), (0xFFFFFFFE, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFE),
                  (0x80000000, 0x80000001), (0x00FF00FF, 0xFF00FF00), (0xFF00FF00, 0x00FF00FF), (0x01010101, 0xFEFEFEFE), (0xFEFEFEFE, 0x01010101),
                  (0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (P - 1, P), (P, P + 1), (P + 1, P - 1), (P, P)]
ALU_EDGE_SHIFTS = [(b, c) for b in (1, 0x80000001, 0xFFFFFFFF, 0x7FFFFFFF) for c in (0, 1, 7, 8, 15, 16, 24, 31)]


def borrows_through_a_byte(b, c):
    """Whether b - c borrows out of any of its four bytes (byte-wise b[i] < c[i] somewhere, or a borrow that reaches an equal byte)."""
    borrow = 0
    for k in range(4):
        x, y = (b >> 8 * k) & 255, (c >> 8 * k) & 255
        borrow = int(x - borrow < y)
        if borrow:
            return True
    return False


def alu_edges_program(borrow_free=False):
    """Straight-line: the words of ALU_EDGE_WORDS (and the shift amounts) loaded with IMM32 into fp - 4 (k + 1), then every ALU opcode over
    ALU_EDGE_PAIRS, the result into one scratch cell.  A division leaves out the pairs on which the reference's VM panics (a zero divisor, the
    signed overflow); borrow_free leaves out the subtractions that borrow."""
    slot = {w: -4 * (k + 1) for k, w in enumerate(ALU_EDGE_WORDS)}
    amount = {c: -4 * (len(ALU_EDGE_WORDS) + 1 + k) for k, c in enumerate(sorted({c for _, c in ALU_EDGE_SHIFTS}))}
    dst = -4 * (len(slot) + len(amount) + 1)
    p = [imm32(a, w) for w, a in slot.items()] + [imm32(a, c) for c, a in amount.items()]
    for b, c in ALU_EDGE_PAIRS:
        for op in (ADD32, SUB32, LT32, LTE32, SLT32, SLE32, AND32, OR32, XOR32, MUL32, MULHS32, MULHU32, DIV32, SDIV32, NE32, EQ32):
            if op in (DIV32, SDIV32) and (c == 0 or (op == SDIV32 and (b, c) == (0x80000000, 0xFFFFFFFF))):
                continue
            if op == SUB32 and borrow_free and borrows_through_a_byte(b, c):
                continue
            p.append((op, [dst, slot[b], slot[c], 0, 0]))
    for b, c in ALU_EDGE_SHIFTS:
        p += [(op, [dst, slot[b], amount[c], 0, 0]) for op in (SHL32, SHR32, SRA32)]
    return p + [(STOP, [])]


def long_rom_program(n=5000):
    """n straight-line IMM32 and a STOP: the pcs run past the 4096 bins the program chip's histogram keeps in LDS, the last fetch among them."""
    return [imm32(-4 * (1 + i % 16), i) for i in range(n)] + [(STOP, [])]


def np_u32(desc_ptr, n, w):
    import ctypes

    if not int(n):
        return np.zeros((0, w), dtype=np.uint32)
    return np.ctypeslib.as_array(ctypes.cast(desc_ptr, ctypes.POINTER(ctypes.c_uint32)), shape=(int(n), w)).copy()
