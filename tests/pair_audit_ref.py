"""An independent restatement of the pair audit's contract (include/vgpu.h, "Pair audit"), by brute force: for every (chip, row, pair of main
columns c1 < c2, delta pair q) both cells are changed in a copy of the trace, oracle.pyoracle.eval_constraints — the oracle's own transcription
of the chips (oracle/chips.hpp), which shares no code with valida_amd/csrc/chips — is called on rows r and (r - 1) mod n of the changed trace
(one call for n = 1) and compared with its values on the unchanged trace (a NEWLY non-zero constraint detects), and Machine.interactions(chip)
is evaluated before and after.  The single mutations are the mutation audit's reference (tests/mutation_audit_ref.py).  EVERY pair is evaluated
at both rows: no coupling shortcut is used for a count.  The coupling sets, which the report only counts, are restated independently too: a
constraint reads a column when its value at random points (random rows, every selector combination) changes with that column — polynomial
identity testing of the oracle's chips, not a walk over the product's compiled program.  The one economy is mutation_audit_ref's: bus records
depend on one row, so the interactions are evaluated with numpy over all rows at once.  The pair loop calls the oracle's entry point
(oracle_eval_constraints, what pyoracle.eval_constraints wraps) on the rows of the changed trace in place, without the wrapper's copies."""
import ctypes

import numpy as np

from oracle import pyoracle as po

import constraint_audit_ref as car
import mutation_audit_ref as mar

NUM_CHIPS = 14
P = 2013265921
MAGIC = 0x31525056


def coupling(machine, chip, width, prep_width, n, seed=12345):
    """The set of coupled pairs (c1, c2), c1 < c2, of a chip of the oracle at height n.

    The contract's coupling is syntactic (a constraint of the Program READS both columns); this one is semantic (a constraint's VALUE depends on
    both).  A column that a constraint mentions but that cancels in it (x - x) is read without being depended on, so the syntactic set can be
    the larger one; neither changes a count, since a cancelled column cannot compensate.  The report's `coupled` word is therefore pinned by
    this reference only on inputs where the two agree, which they do on every BasicMachine chip: none has a cancelling column."""
    if n == 1:
        return {(a, b) for a in range(width) for b in range(a + 1, width)}
    rng = np.random.RandomState(seed + chip)
    out = set()
    rows = lambda w: rng.randint(1, P, size=w).astype(np.uint32)
    for first, last, trans in ((0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0)):
        for _ in range(2):
            loc, nxt = rows(width), rows(width)
            pl, pn = (rows(prep_width), rows(prep_width)) if prep_width else (None, None)
            ev = lambda a, b: po.eval_constraints(chip, a, b, pl, pn, is_first=first, is_last=last, is_transition=trans)
            base = ev(loc, nxt)
            if base.size == 0:
                break
            reads = np.zeros((base.size, width), dtype=bool)
            for c in range(width):
                for which in (0, 1):
                    a, b = loc.copy(), nxt.copy()
                    (a if which == 0 else b)[c] = (int((a if which == 0 else b)[c]) + 1 + int(rng.randint(0, P - 1))) % P
                    reads[:, c] |= ev(a, b) != base
            for k in range(base.size):
                cols = np.nonzero(reads[k])[0]
                out |= {(int(a), int(b)) for i, a in enumerate(cols) for b in cols[i + 1:]}
    for it in machine.interactions(chip):
        cols = sorted({col for v in [it["count"]] + list(it["fields"]) for is_prep, col, _ in v[1] if not is_prep})
        out |= {(a, b) for i, a in enumerate(cols) for b in cols[i + 1:]}
    return out


_counts = {}


def chip_counts(machine, chip, trace, prep, deltas):
    """K, M, {(c1, c2, q): (free rows as a boolean array, compensated rows as a boolean array)} of one chip, every pair evaluated.  Computed
    once per (chip, trace contents, deltas): fib(25) and alu(50) have the same idle mul trace."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    key = (chip, t.shape, t.tobytes(), p.tobytes() if p is not None else None, tuple(deltas))
    if key not in _counts:
        _counts[key] = _chip_counts(machine, chip, t, p, deltas)
    return _counts[key]


def _chip_counts(machine, chip, t, p, deltas):
    n, w = t.shape
    D = len(deltas)
    K = car.n_constraints(chip, t, p)
    inter = machine.interactions(chip)
    _, single = mar.chip_counts(machine, chip, t, p, deltas)
    free1 = {}
    for (c, di), (rows, _, _) in single.items():
        f = np.zeros(n, dtype=bool)
        f[rows] = True
        free1[(c, di)] = f
    base = [mar._eval(chip, t, p, q) != 0 for q in range(n)] if K else None
    # oracle_eval_constraints on rows `row` and row + 1 of t (and p) where they lie: the values mar._eval gives
    f = po.lib().oracle_eval_constraints
    f.restype = ctypes.c_uint32
    vals = np.zeros(max(1, K), dtype=np.uint32)
    none = np.zeros(8, dtype=np.uint32)
    tb, pb, vp, u = t.ctypes.data, (p.ctypes.data if p is not None else none.ctypes.data), ctypes.c_void_p(vals.ctypes.data), ctypes.c_uint32
    ts, pstr = t.strides[0], (p.strides[0] if p is not None else 0)
    assert t.flags.c_contiguous and (p is None or p.flags.c_contiguous)

    def newly(row):
        nx = (row + 1) % n
        f(u(chip), ctypes.c_void_p(tb + row * ts), ctypes.c_void_p(tb + nx * ts), ctypes.c_void_p(pb + row * pstr), ctypes.c_void_p(pb + nx * pstr), u(int(row == 0)), u(int(row == n - 1)),
          u(int(row != n - 1)), vp, u(K))
        return bool(np.any((vals[:K] != 0) & ~base[row]))

    out = {}
    for c1 in range(w):
        for c2 in range(c1 + 1, w):
            for q in range(D * D):
                d1, d2 = deltas[q // D], deltas[q % D]
                air = np.zeros(n, dtype=bool)
                if K:
                    for r in range(n):
                        k1, k2 = t[r, c1], t[r, c2]
                        t[r, c1], t[r, c2] = (int(k1) + d1) % P, (int(k2) + d2) % P
                        for row in {r, (r - 1) % n}:
                            if newly(row):
                                air[r] = True
                        t[r, c1], t[r, c2] = k1, k2
                t2 = t.copy()
                t2[:, c1] = (t[:, c1].astype(np.uint64) + d1) % P
                t2[:, c2] = (t[:, c2].astype(np.uint64) + d2) % P
                free = ~air & ~mar.bus_detected(inter, t, t2, p)
                out[(c1, c2, q)] = (free, free & ~(free1[(c1, q // D)] & free1[(c2, q % D)]))
    return K, len(inter), out


def audit(machine, main, preprocessed, deltas=(1, P - 1), max_entries=1024, max_rows_per_entry=4, chips=None):
    """The contract's report as PairReport's attributes, plus `uncoupled_compensated` (the theorem: always 0) and the coupling sets."""
    prep_of = dict(preprocessed)
    deltas = [int(d) for d in deltas]
    D = len(deltas)
    blocks, entries, couplings, theorem = [], [], [], 0
    for chip in range(NUM_CHIPS):
        t = np.asarray(main[chip])
        n, w = t.shape
        pw = np.asarray(prep_of[chip]).shape[1] if chip in prep_of else 0
        audited = chips is None or chip in chips
        free, comp, slack, cp = [0] * (D * D), [0] * (D * D), set(), set()
        K = car.n_constraints(chip, np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None)
        M = len(machine.interactions(chip))
        if audited:
            cp = coupling(machine, chip, w, pw, n)
            K, M, counts = chip_counts(machine, chip, t, prep_of.get(chip), deltas)
            for (c1, c2, q), (f, c) in sorted(counts.items()):
                free[q] += int(f.sum())
                comp[q] += int(c.sum())
                if c.any():
                    if (c1, c2) not in cp:
                        theorem += int(c.sum())
                    slack.add((c1, c2))
                    rows = [int(r) for r in np.nonzero(c)[0]]
                    entries.append(dict(chip=chip, c1=c1, c2=c2, q=q, free=int(f.sum()), compensated=len(rows), rows=rows[:max_rows_per_entry]))
        couplings.append(cp)
        blocks.append(dict(chip=chip, width=w, constraints=K, interactions=M, audited=audited, height=n, coupled=len(cp), slack=len(slack), free=free, compensated=comp))
    return dict(deltas=deltas, truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries], uncoupled_compensated=theorem,
                coupling=couplings)


def recut(want, max_entries=1024, max_rows_per_entry=4):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["compensated"], max_rows_per_entry) for e in entries)
    return dict(want, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def assert_report_equals(rep, want):
    """A PairReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.deltas, rep.truncated, rep.total_entries, rep.reported) == (want["deltas"], want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    assert rep.entries == want["entries"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    D = len(want["deltas"])
    w = [MAGIC, 0, D, int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"])] + (want["deltas"] + [0] * 4)[:4]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"]) + [c["coupled"], c["slack"]]
        for q in range(D * D):
            w += u64(c["free"][q]) + u64(c["compensated"][q])
    for e in want["entries"]:
        w += [e["chip"], e["c1"], e["c2"], e["q"], len(e["rows"]), 0] + u64(e["free"]) + u64(e["compensated"]) + e["rows"]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
