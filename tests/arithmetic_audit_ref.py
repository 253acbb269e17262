"""A numpy and plain-integer restatement of the arithmetic audit's contract (include/vgpu.h, "Arithmetic audit"), written from its text: the
entries of the audited bus from the machine's interaction lists, their vcols over whole columns, the live records in slot order, Python
integers for the arithmetic, and the report's word image.  Nothing here calls the audit under test."""
import numpy as np

import valida_amd as va

P = va.P
KINDS = ("malformed", "undefined", "wrong_result", "shift_quotient", "arithmetic_shr")
(ADD, SUB, MUL, DIV, LT, SHL, SHR, AND, OR, XOR, SDIV, NE, MULHU, SRA, MULHS, LTE, EQ, SLT, SLE) = range(19)
M32 = 0xFFFFFFFF


def vcol(v, main, prep):
    const, terms = v
    acc = np.full(main.shape[0], const % P, dtype=np.uint64)
    for is_prep, col, weight in terms:
        src = prep if is_prep else main
        acc = (acc + np.uint64(weight % P) * (src[:, col].astype(np.uint64) % np.uint64(P))) % np.uint64(P)
    return acc


def entries(machine, bus=(True, 0), sides=1):
    """[(chip, interaction, is_send, n_fields)] in ascending (chip, interaction) order"""
    return [(c, m, int(bool(i["send"])), len(i["fields"])) for c in range(machine.num_chips) for m, i in enumerate(machine.interactions(c))
            if (bool(i["global"]), i["bus"]) == (bool(bus[0]), bus[1]) and sides & (2 if i["send"] else 1)]


def signed(v):
    return v - (1 << 32) if v >> 31 else v


def sra(x, k):
    return (signed(x) >> k) & M32


def expected(idx, x, y):
    """The word the opcode computes; the operation is defined."""
    if idx in (DIV, SDIV):
        if idx == DIV:
            return x // y
        q = abs(signed(x)) // abs(signed(y))  # truncated toward zero
        return (q if (signed(x) < 0) == (signed(y) < 0) else -q) & M32
    return {ADD: (x + y) & M32, SUB: (x - y) & M32, MUL: (x * y) & M32, MULHU: (x * y) >> 32, MULHS: (x * y) >> 32, SHL: (x << y) & M32 if y < 32 else 0, SHR: x >> y, SRA: sra(x, min(y, 31)),
            AND: x & y, OR: x | y, XOR: x ^ y, LT: int(x < y), LTE: int(x <= y), SLT: int(signed(x) < signed(y)), SLE: int(signed(x) <= signed(y)), NE: int(x != y), EQ: int(x == y)}[idx]


def judge(opcode, f):
    """(kind or 0, mask or reason, expected word, the MULHS sign flag) of one live judged record; f = the twelve byte fields."""
    idx = opcode - 100
    bad = sum(1 << j for j in range(12) if f[j] >= 256)
    if bad:
        return 1, bad, 0, False
    x, y, z = (int.from_bytes(bytes(f[4 * k:4 * k + 4]), "big") for k in range(3))
    reason = 1 if idx in (DIV, SDIV) and y == 0 else 2 if idx == SDIV and (x, y) == (0x80000000, M32) else 3 if idx in (SHL, SHR, SRA) and y >= 32 else 0
    if reason:
        return 2, reason, 0, False
    e = expected(idx, x, y)
    sign = idx == MULHS and ((signed(x) * signed(y)) >> 32) & M32 != e
    if z == e:
        return 0, 0, e, sign
    diff = sum(1 << j for j in range(4) if (z >> (24 - 8 * j)) & 255 != (e >> (24 - 8 * j)) & 255)
    if idx == SDIV and y & (y - 1) == 0 and z == sra(x, y.bit_length() - 1):
        return 4, diff, e, sign
    if idx == SHR and z == sra(x, y):
        return 5, diff, e, sign
    return 3, diff, e, sign


def audit(machine, main, preprocessed, max_findings=64, bus=(True, 0), sides=1):
    prep_of = {c: np.asarray(m, dtype=np.uint64) for c, m in preprocessed}
    c = dict(slots=0, live=0, judged=0, other=0, hard=0, malformed=0, undefined=0, wrong_result=0, soft=0, shift_quotient=0, arithmetic_shr=0, mulhs_sign_matters=0, division_by_zero=0,
             signed_overflow=0, shift_range=0)
    opcodes, ents, hard, soft = [0] * 19, [], [], []
    for chip, m, is_send, nf in entries(machine, bus, sides):
        it = machine.interactions(chip)[m]
        assert nf >= 13
        t = np.asarray(main[chip], dtype=np.uint64) % np.uint64(P)
        cols = np.stack([vcol(v, t, prep_of.get(chip)).astype(np.int64) for v in [it["count"]] + it["fields"][:13]], axis=1)
        e = dict(chip=chip, interaction=m, is_send=is_send, n_fields=nf, live=0, hard=0)
        c["slots"] += t.shape[0]
        for row in np.flatnonzero(cols[:, 0]).tolist():
            count, opcode, f = int(cols[row, 0]), int(cols[row, 1]), [int(x) for x in cols[row, 2:]]
            e["live"] += 1
            if not 100 <= opcode <= 118:
                c["other"] += 1
                continue
            c["judged"] += 1
            opcodes[opcode - 100] += 1
            kind, mask, want, sign = judge(opcode, f)
            c["mulhs_sign_matters"] += int(sign)
            if not kind:
                continue
            c[KINDS[kind - 1]] += 1
            if kind == 2:
                c[("division_by_zero", "signed_overflow", "shift_range")[mask - 1]] += 1
            e["hard"] += kind <= 3
            (hard if kind <= 3 else soft).append(dict(kind=kind, mask=mask, chip=chip, interaction=m, row=row, opcode=opcode, f=f, expected=want, count=count, is_send=is_send))
        c["live"] += e["live"]
        ents.append(e)
    c["hard"], c["soft"] = len(hard), len(soft)
    return dict(bus=bus, sides=sides, max_findings=max_findings, counters=c, opcodes=opcodes, entries=ents, hard=hard[:max_findings], soft=soft[:max_findings],
                truncated=int(len(hard) > max_findings) | int(len(soft) > max_findings) << 1)


def words(a):
    c = a["counters"]
    u64 = lambda v: [int(v) & 0xFFFFFFFF, int(v) >> 32]
    w = [0x31524156, 0, int(bool(a["bus"][0])), a["bus"][1], a["sides"], a["truncated"], len(a["hard"]), len(a["soft"]), a["max_findings"], len(a["entries"])]
    for k in ("slots", "live", "judged", "other", "hard", "malformed", "undefined", "wrong_result", "soft", "shift_quotient", "arithmetic_shr", "mulhs_sign_matters", "division_by_zero",
              "signed_overflow", "shift_range"):
        w += u64(c[k])
    for n in a["opcodes"]:
        w += u64(n)
    w += [0, 0]
    for e in a["entries"]:
        w += [e["chip"], e["interaction"], e["is_send"], e["n_fields"]] + u64(e["live"]) + u64(e["hard"])
    for f in a["hard"] + a["soft"]:
        w += [f["kind"], f["mask"], f["chip"], f["interaction"], f["row"], f["opcode"]] + f["f"] + [f["expected"], f["count"], f["is_send"], 0, 0, 0]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
