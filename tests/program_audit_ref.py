"""The program audit's contract (include/vgpu.h, "Program audit") in numpy: np.bincount and plain comparisons over the fetching chip's main
trace and the table chip's two traces.  audit() returns a dict of plain values, words() its report image as the library would write it."""
import numpy as np

import valida_amd as va

P = va.P
TWO32 = (1 << 32) % P
DEFAULT_FETCH = (0, 1, [3, 4, 5, 6, 7, 8])
DEFAULT_TABLE = (1, 0, [1, 2, 3, 4, 5, 6], 0)


def _finding(kind, mask, row, pc, found, expected):
    pad = lambda v: [int(x) for x in v] + [0] * (8 - len(v))
    return dict(kind=kind, mask=int(mask), row=int(row), pc=int(pc), found=pad(found), expected=pad(expected))


def audit(main, prep, rom_len=0, max_findings=64, max_ranges=64, fetch=None, table=None):
    fchip, pc_col, fcols = fetch or DEFAULT_FETCH
    tchip, key_col, tcols, mult_col = table or DEFAULT_TABLE
    fm, tm, tp = np.asarray(main[fchip], dtype=np.int64) % P, np.asarray(main[tchip], dtype=np.int64) % P, np.asarray(dict(prep)[tchip], dtype=np.int64) % P
    H, T, nf = fm.shape[0], tm.shape[0], len(fcols)
    rom_len = rom_len or T
    pc, f = fm[:, pc_col], fm[:, fcols]
    K, W, m = tp[:, key_col], tp[:, tcols], tm[:, mult_col]
    c = np.bincount(pc[pc < T], minlength=T)
    # the fetches
    out = pc >= rom_len
    w = np.zeros_like(f)
    w[~out] = W[pc[~out]]
    differs = (f != w) & ~out[:, None]
    other = differs & ((f - w) % P != TWO32)
    mask = (differs * (1 << np.arange(nf))).sum(axis=1)
    kind = np.where(out, 2, np.where(other.any(axis=1), 3, np.where(differs.any(axis=1), 4, 0)))
    fetch_hard = [_finding(int(kind[r]), mask[r], r, pc[r], f[r], w[r]) for r in np.flatnonzero((kind == 2) | (kind == 3))]
    wrapped = [_finding(4, mask[r], r, pc[r], f[r], w[r]) for r in np.flatnonzero(kind == 4)]
    # the table
    rows = np.arange(T)
    keys = [_finding(1, 0, i, i, [K[i]], [i]) for i in np.flatnonzero(K != rows)]
    mult = [_finding(5, 0, i, i, [m[i]], [c[i] % P, c[i]]) for i in np.flatnonzero(m != c % P)]
    unf = (c[:rom_len] == 0).astype(np.int64)
    edge = np.diff(np.r_[0, unf, 0])
    ranges = list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))
    d = (pc[1:] - pc[:-1]) % P
    hot = int(np.argmax(c)) if c.max() > 0 else 0  # argmax: the lowest index on a tie
    hard = keys + fetch_hard + mult
    counters = dict(fetches=H, table_rows=T, rom_len=rom_len, fetched_words=int(rom_len - unf.sum()), unfetched_words=int(unf.sum()), unfetched_ranges=len(ranges), hottest_pc=hot,
                    hottest_count=int(c[hot]), first_pc=int(pc[0]), last_pc=int(pc[-1]), sequential=int((d == 1).sum()), stay=int((d == 0).sum()), jumps=int((d > 1).sum()), hard=len(hard),
                    table_key=len(keys), pc_out_of_rom=int((kind == 2).sum()), wrong_instruction=int((kind == 3).sum()), wrapped_operand=len(wrapped), multiplicity=len(mult))
    return dict(fetch_chip=fchip, table_chip=tchip, n_fields=nf, max_findings=max_findings, max_ranges=max_ranges, counters=counters, hard=hard[:max_findings], wrapped=wrapped[:max_findings],
                unfetched=ranges[:max_ranges], truncated=(len(hard) > max_findings) | (len(wrapped) > max_findings) << 1 | (len(ranges) > max_ranges) << 2)


def words(a):
    c = a["counters"]
    u64 = lambda v: [int(v) & 0xFFFFFFFF, int(v) >> 32]
    w = [0x31475056, 0, a["fetch_chip"], a["table_chip"], a["n_fields"], int(a["truncated"]), len(a["hard"]), len(a["wrapped"]), len(a["unfetched"]), a["max_findings"], a["max_ranges"],
         c["rom_len"]]
    for k in ("fetches", "table_rows", "fetched_words", "unfetched_words", "unfetched_ranges"):
        w += u64(c[k])
    w += [c["hottest_pc"], 0] + u64(c["hottest_count"]) + [c["first_pc"], c["last_pc"]]
    for k in ("sequential", "stay", "jumps", "hard", "table_key", "pc_out_of_rom", "wrong_instruction", "wrapped_operand", "multiplicity"):
        w += u64(c[k])
    w += [0, 0]
    for f in a["hard"] + a["wrapped"]:
        w += [f["kind"], f["mask"], f["row"], f["pc"]] + f["found"] + f["expected"] + [0, 0, 0, 0]
    for lo, hi in a["unfetched"]:
        w += [lo, hi]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
