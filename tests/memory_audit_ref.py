"""A numpy restatement of the memory audit's contract (include/vgpu.h, "Memory audit"), written from its text: the receives of the audited bus
from the machine's interaction lists, their vcols over whole columns, the live records in seq order, np.lexsort by (addr, clk, !static, seq), a
dictionary walk for the state, and the report's word image.  Nothing here calls the audit under test."""
import numpy as np

import valida_amd as va

P = va.P
KINDS = ("malformed", "duplicate_static", "stale_read", "uninit_read")
NONE = 0xFFFFFFFF


def vcol(v, main, prep):
    const, terms = v
    acc = np.full(main.shape[0], const % P, dtype=np.uint64)
    for is_prep, col, weight in terms:
        src = prep if is_prep else main
        acc = (acc + np.uint64(weight % P) * (src[:, col].astype(np.uint64) % np.uint64(P))) % np.uint64(P)
    return acc


def receives(machine, bus=(True, 2)):
    """[(chip, interaction)] of the receives on `bus`, in seq order"""
    return [(c, m) for c in range(machine.num_chips) for m, i in enumerate(machine.interactions(c)) if not i["send"] and (bool(i["global"]), i["bus"]) == (bool(bus[0]), bus[1])]


def records(machine, main, preprocessed, bus=(True, 2)):
    """The live records in seq order as an int64 array of rows (chip, row, interaction, count, is_read, clk, addr, is_static, v0..v3, key); the
    slot count; the layout descents and the first (chip, row) of one."""
    prep_of = {c: np.asarray(m, dtype=np.uint64) for c, m in preprocessed}
    parts, slots, descents, first = [], 0, 0, None
    for c, m in receives(machine, bus):
        it = machine.interactions(c)[m]
        assert len(it["fields"]) == 8
        t = np.asarray(main[c], dtype=np.uint64) % np.uint64(P)
        n = t.shape[0]
        slots += n
        cols = [vcol(v, t, prep_of.get(c)).astype(np.int64) for v in [it["count"]] + it["fields"]]
        key = (cols[3] << 32) | (cols[2] << 1) | (cols[4] != 1)
        live = cols[0] != 0
        down = np.nonzero(live[:-1] & live[1:] & (key[:-1] > key[1:]))[0]
        descents += len(down)
        if len(down) and (first is None or (c, int(down[0])) < first):
            first = (c, int(down[0]))
        rows = np.nonzero(live)[0]
        parts.append(np.stack([np.full(len(rows), c), rows, np.full(len(rows), m)] + [k[rows] for k in cols] + [key[rows]], axis=1).reshape(-1, 13))
    rec = np.concatenate(parts) if parts else np.zeros((0, 13), dtype=np.int64)
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))], slots, descents, first


def audit(machine, main, preprocessed, max_findings=64, bus=(True, 2)):
    rec, slots, descents, first_descent = records(machine, main, preprocessed, bus)
    rec = rec[np.lexsort((np.arange(len(rec)), rec[:, 12]))]  # by key, ties in seq order
    L = len(rec)
    c = dict(slots=slots, live=L, reads=0, writes=0, statics=0, addresses=0, min_addr=0, max_addr=0, max_clk=0, max_clk_gap=0, uninit_zero_reads=0, same_cycle_pairs=0, dummy_reads_clk=0,
             dummy_reads_addr=0, layout_descents=descents, findings=0, malformed=0, duplicate_static=0, stale_read=0, uninit_read=0)
    if L:
        c["min_addr"], c["max_addr"], c["max_clk"] = int(rec[:, 6].min()), int(rec[:, 6].max()), int(rec[:, 5].max())
    state, seen, findings, prev = {}, set(), [], None
    for pos, r in enumerate(rec.tolist()):
        chip, row, inter, count, is_read, clk, addr, is_static = r[:8]
        v = r[8:12]
        read, stat = is_read == 1, is_static == 1
        c["reads" if read else "writes"] += 1
        c["statics"] += stat
        if addr not in seen:
            seen.add(addr)
            c["addresses"] += 1
        if prev is not None:
            if prev["addr"] == addr:
                gap = clk - prev["clk"]
                c["max_clk_gap"] = max(c["max_clk_gap"], gap)
                if gap > L:
                    c["dummy_reads_clk"] += gap // L
                if gap == 0 and not stat and not prev["stat"] and not (read and prev["read"]):
                    c["same_cycle_pairs"] += 1
            elif addr - prev["addr"] > L:
                c["dummy_reads_addr"] += (addr - prev["addr"]) // L
        last = state.get(addr)
        if read and last is None and not any(v):
            c["uninit_zero_reads"] += 1
        reason = (count != 1) | (is_read > 1) << 1 | (is_static > 1) << 2 | (stat and (read or clk != 0)) << 3 | any(x >= 256 for x in v) << 4
        kind = 0
        if reason:
            kind = 1
        elif stat and prev is not None and prev["addr"] == addr and prev["stat"]:
            kind = 2
        elif read and last is not None and last[0] != v:
            kind = 3
        elif read and last is None and any(v):
            kind = 4
        if kind:
            c["findings"] += 1
            c[KINDS[kind - 1]] += 1
            if len(findings) < max_findings:
                findings.append(dict(kind=KINDS[kind - 1], reason=int(reason), chip=chip, interaction=inter, row=row, addr=addr, clk=clk, value=v, expected=last[0] if last else [0, 0, 0, 0],
                                     last_write=last[1] if last else None, position=pos))
        if not read:
            state[addr] = (v, (chip, inter, row))
        prev = dict(addr=addr, clk=clk, stat=stat, read=read)
    return dict(bus=(bool(bus[0]), bus[1]), max_findings=max_findings, receives=receives(machine, bus), counters=c, first_descent=first_descent, findings=findings)


def words(d):
    """The report's word image (include/vgpu.h)"""
    c = d["counters"]
    w = [0x314D4D56, 0, int(d["bus"][0]), d["bus"][1], len(d["receives"]), int(c["findings"] > len(d["findings"])), len(d["findings"]), d["max_findings"]]

    def u64(x):
        w.extend([x & 0xFFFFFFFF, x >> 32])

    for k in ("slots", "live", "reads", "writes", "statics", "addresses"):
        u64(c[k])
    w += [c["min_addr"], c["max_addr"], c["max_clk"], c["max_clk_gap"]]
    for k in ("uninit_zero_reads", "same_cycle_pairs", "dummy_reads_clk", "dummy_reads_addr", "layout_descents"):
        u64(c[k])
    w += list(d["first_descent"]) if d["first_descent"] is not None else [NONE, NONE]
    for k in ("findings",) + KINDS:
        u64(c[k])
    u64(0)
    for r in d["receives"]:
        w += list(r)
    for f in d["findings"]:
        w += [KINDS.index(f["kind"]) + 1, f["reason"], f["chip"], f["interaction"], f["row"], f["addr"], f["clk"]] + list(f["value"]) + list(f["expected"])
        w += (list(f["last_write"]) if f["last_write"] is not None else [NONE] * 3) + [f["position"], 0]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
