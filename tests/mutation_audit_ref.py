"""An independent restatement of the mutation audit's contract (include/vgpu.h, "Mutation audit"), by brute force: for every (chip, row, main
column, delta) the cell is changed in a copy of the trace, oracle.pyoracle.eval_constraints — the oracle's own transcription of the chips
(oracle/chips.hpp), which shares no code with valida_amd/csrc/chips — is called on rows r and (r - 1) mod n of the changed trace (one call for
n = 1, where the cell is local and next at once) and compared with its values on the unchanged trace (a NEWLY non-zero constraint detects), and
Machine.interactions(chip) is evaluated on the row before and after (a record is (count, fields) when count != 0, else nothing).  No shortcut
of the product is used: every column is evaluated at both rows whether or not a constraint reads it.  The one economy: the bus records of a row
depend on that row alone, so the interactions are evaluated with numpy over all rows at once, on the trace whose whole column has the delta
added.  About 27 microseconds per evaluation: 8 s for fib(25), 17 s for alu(50) at two deltas."""
import numpy as np

from oracle import pyoracle as po

import constraint_audit_ref as car

NUM_CHIPS = 14
P = 2013265921


def _vcol(v, m, p):
    const, terms = v
    acc = np.full(m.shape[0], const % P, dtype=np.uint64)
    for is_prep, col, weight in terms:
        acc = (acc + (p if is_prep else m)[:, col].astype(np.uint64) % P * (weight % P)) % P
    return acc


def bus_detected(interactions, m, m2, p):
    """Per row: does the record of some interaction differ between trace m and trace m2?"""
    det = np.zeros(m.shape[0], dtype=bool)
    for it in interactions:
        c0, c1 = _vcol(it["count"], m, p), _vcol(it["count"], m2, p)
        live0, live1 = c0 != 0, c1 != 0
        differ = c0 != c1
        for f in it["fields"]:
            differ |= _vcol(f, m, p) != _vcol(f, m2, p)
        det |= (live0 != live1) | (live0 & live1 & differ)
    return det


def _eval(chip, t, p, q):
    n = t.shape[0]
    nx = (q + 1) % n
    return po.eval_constraints(chip, t[q], t[nx], p[q] if p is not None else None, p[nx] if p is not None else None, is_first=int(q == 0), is_last=int(q == n - 1),
                               is_transition=int(q != n - 1))


def chip_counts(machine, chip, trace, prep, deltas):
    """{(column, delta index): (free rows as a sorted list, air count, bus count)} of one chip."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    n, w = t.shape
    K = car.n_constraints(chip, t, p)
    inter = machine.interactions(chip)
    base = [_eval(chip, t, p, q) != 0 for q in range(n)] if K else None
    out = {}
    for c in range(w):
        for di, d in enumerate(deltas):
            air = np.zeros(n, dtype=bool)
            if K:
                for r in range(n):
                    keep = t[r, c]
                    t[r, c] = (int(keep) + d) % P
                    for q in {r, (r - 1) % n}:
                        if np.any((_eval(chip, t, p, q) != 0) & ~base[q]):
                            air[r] = True
                    t[r, c] = keep
            t2 = t.copy()
            t2[:, c] = (t[:, c].astype(np.uint64) + d) % P
            bus = bus_detected(inter, t, t2, p)
            out[(c, di)] = ([int(r) for r in np.nonzero(~air & ~bus)[0]], int(air.sum()), int(bus.sum()))
    return K, out


def audit(machine, main, preprocessed, deltas=(1, P - 1), max_entries=1024, max_rows_per_entry=4):
    """The contract's report: dict(deltas, truncated, total_entries, chips=[dict(chip, width, constraints, height, unbound, free, air, bus)],
    entries=[dict(chip, column, delta, free, air, bus, rows)]) — MutationReport's attributes."""
    prep_of = dict(preprocessed)
    deltas = [int(d) for d in deltas]
    D = len(deltas)
    chips, entries = [], []
    for chip in range(NUM_CHIPS):
        t = np.asarray(main[chip])
        n, w = t.shape
        K, counts = chip_counts(machine, chip, t, prep_of.get(chip), deltas)
        free, air, bus, unbound = [0] * D, [0] * D, [0] * D, 0
        for c in range(w):
            unbound += all(len(counts[(c, di)][0]) == n for di in range(D))
            for di in range(D):
                rows, a, b = counts[(c, di)]
                free[di] += len(rows)
                air[di] += a
                bus[di] += b
                if rows:
                    entries.append(dict(chip=chip, column=c, delta=di, free=len(rows), air=a, bus=b, rows=rows[:max_rows_per_entry]))
        chips.append(dict(chip=chip, width=w, constraints=K, height=n, unbound=unbound, free=free, air=air, bus=bus))
    return dict(deltas=deltas, truncated=len(entries) > max_entries, total_entries=len(entries), chips=chips, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["free"], max_rows_per_entry) for e in entries)
    return dict(want, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def unbound_columns(want, chip):
    D, n = len(want["deltas"]), want["chips"][chip]["height"]
    cols = sorted(set(e["column"] for e in want["entries"] if e["chip"] == chip))
    return [c for c in cols if sum(1 for e in want["entries"] if e["chip"] == chip and e["column"] == c and e["free"] == n) == D]


def assert_report_equals(rep, want):
    """A MutationReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.deltas, rep.truncated, rep.total_entries, rep.reported) == (want["deltas"], want["truncated"], want["total_entries"], len(want["entries"]))
    assert rep.chips == want["chips"]
    assert rep.entries == want["entries"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    D = len(want["deltas"])
    w = [0x31524D56, 0, D, int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"])] + (want["deltas"] + [0] * 4)[:4]
    for c in want["chips"]:
        w += [c["width"], c["constraints"]] + u64(c["height"]) + [c["unbound"], 0]
        for i in range(D):
            w += u64(c["free"][i]) + u64(c["air"][i]) + u64(c["bus"][i])
    for e in want["entries"]:
        w += [e["chip"], e["column"], e["delta"], len(e["rows"])] + u64(e["free"]) + u64(e["air"]) + u64(e["bus"]) + e["rows"]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
