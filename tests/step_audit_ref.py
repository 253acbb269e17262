"""An independent restatement of the step audit's contract (include/vgpu.h, "Step audit").  The directions are those of tests/rank_audit_ref.py
(chip_rows: exact interpolation of the oracle's own chip transcription, numpy RREF; its FULL null vectors, and e_c for a zero loose column).
The moves are judged as tests/mutation_audit_ref.py judges its mutations: oracle.pyoracle.eval_constraints on rows r and (r - 1) mod n of the
changed trace (one call for n = 1) against its values on the unchanged trace (a NEWLY non-zero constraint detects), and
mutation_audit_ref.bus_detected on the changed row.  Nothing of the product is used but Machine.interactions and Machine.chip_info (the
machine's max constraint degree, an input of the contract)."""
import numpy as np

import constraint_audit_ref as car
import mutation_audit_ref as mar
import rank_audit_ref as rar

NUM_CHIPS = 14
P = 2013265921
MAGIC = 0x31525356
TERMS = 8
DEFAULT_STEPS = (1, P - 1, 2)

_cache = {}


def chip_cells(machine, chip, trace, prep, steps):
    """K, M and per row {loose column: (pass mask, is zero, full vector, bus-detected steps)} of one chip."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    key = (chip, t.shape, t.tobytes(), p.tobytes() if p is not None else None, tuple(steps))
    if key in _cache:
        return _cache[key]
    n, w = t.shape
    K, M, rows = rar.chip_rows(machine, chip, t, p)
    inter = machine.interactions(chip)
    base = [mar._eval(chip, t, p, q) != 0 for q in range(n)] if K else None
    out = []
    for r, (rank, zero, loose, vectors) in enumerate(rows):
        judged, cells = {}, {}
        for c in loose:
            v = tuple(vectors[c]) if c in vectors else ((c, 1),)
            assert (c in zero) == (c not in vectors)
            if v not in judged:
                mask, bus = 0, 0
                for s, step in enumerate(steps):
                    keep = t[r].copy()
                    for col, coef in v:
                        t[r, col] = (int(keep[col]) + step * coef) % P
                    air = False
                    if K:
                        for q in {r, (r - 1) % n}:
                            air = air or bool(np.any((mar._eval(chip, t, p, q) != 0) & ~base[q]))
                    moved = t[r:r + 1].copy()
                    t[r] = keep
                    b = bool(mar.bus_detected(inter, t[r:r + 1], moved, p[r:r + 1] if p is not None else None)[0])
                    mask |= int(not air and not b) << s
                    bus += int(b)
                judged[v] = (mask, bus)
            cells[c] = (judged[v][0], c in zero, list(v), judged[v][1])
        out.append(cells)
    _cache[key] = (K, M, out)
    return _cache[key]


def audit(machine, main, preprocessed, steps=DEFAULT_STEPS, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The contract's report as StepReport's attributes."""
    prep_of = dict(preprocessed)
    S, full = len(steps), (1 << len(steps)) - 1
    blocks, entries = [], []
    for chip in range(len(main)):
        t = np.asarray(main[chip])
        n, w = t.shape
        audited = chips is None or chip in chips
        K = car.n_constraints(chip, np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None) if chip < NUM_CHIPS else None
        deg = machine.chip_info(chip)["max_degree"]
        b = dict(chip=chip, width=w, constraints=K, interactions=len(machine.interactions(chip)), audited=audited, height=n, max_degree=deg, line_exact=audited and S >= deg,
                 loose_cells=0, zero_cells=0, exact_cells=0, coupled_exact_cells=0, confirmed_rows=0, refuted_rows=0, passes=[0] * S, bus=0, loose=[0] * w, zeros=[0] * w,
                 exact=[0] * w, coupled_exact=[0] * w)
        if audited:
            K, M, rows = chip_cells(machine, chip, t, prep_of.get(chip), steps)
            listed, curved = {}, [0] * w
            for r, cells in enumerate(rows):
                confirmed = refuted = False
                for c, (mask, zero, v, bus) in sorted(cells.items()):
                    exact = mask == full
                    b["loose"][c] += 1
                    b["zeros"][c] += int(zero)
                    b["exact"][c] += int(exact)
                    b["coupled_exact"][c] += int(exact and not zero)
                    curved[c] += int(not exact)
                    confirmed |= exact and not zero
                    refuted |= not exact
                    b["bus"] += bus
                    for s in range(S):
                        b["passes"][s] += (mask >> s) & 1
                    if not zero or not exact:
                        listed.setdefault(c, []).append(dict(row=r, pass_mask=mask, zero=zero, exact=exact, n_support=len(v), terms=v[:TERMS]))
                b["confirmed_rows"] += int(confirmed)
                b["refuted_rows"] += int(refuted)
            for k in ("loose", "zeros", "exact", "coupled_exact"):
                b[{"loose": "loose_cells", "zeros": "zero_cells", "exact": "exact_cells", "coupled_exact": "coupled_exact_cells"}[k]] = sum(b[k])
            for c in sorted(listed):
                assert len(listed[c]) == b["coupled_exact"][c] + curved[c]
                entries.append(dict(chip=chip, column=c, coupled_exact=b["coupled_exact"][c], curved=curved[c], rows=listed[c][:max_rows_per_entry]))
        blocks.append(b)
    return dict(steps=list(steps), truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["coupled_exact"] + e["curved"], max_rows_per_entry) for e in entries)
    return dict(want, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def confirmed_columns(want, chip):
    return [k for k, x in enumerate(want["chips"][chip]["coupled_exact"]) if x]


def refuted_columns(want, chip):
    c = want["chips"][chip]
    return [k for k in range(c["width"]) if c["loose"][k] > c["exact"][k]]


def assert_report_equals(rep, want):
    """A StepReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.steps, rep.truncated, rep.total_entries, rep.reported) == (want["steps"], want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    assert rep.entries == want["entries"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    S = len(want["steps"])
    w = [MAGIC, 0, TERMS, int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"]), S, 0] + list(want["steps"]) + [0] * (4 - S)
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"]) + [c["max_degree"], int(c["line_exact"])]
        for k in ("loose_cells", "zero_cells", "exact_cells", "coupled_exact_cells", "confirmed_rows", "refuted_rows"):
            w += u64(c[k])
        for s in range(4):
            w += u64(c["passes"][s] if s < S else 0)
        w += u64(c["bus"])
        for k in range(c["width"]):
            w += u64(c["loose"][k]) + u64(c["zeros"][k]) + u64(c["exact"][k]) + u64(c["coupled_exact"][k])
    for e in want["entries"]:
        w += [e["chip"], e["column"], len(e["rows"]), 0] + u64(e["coupled_exact"]) + u64(e["curved"])
        for r in e["rows"]:
            flat = [x for term in r["terms"] for x in term]
            w += [r["row"], r["pass_mask"], int(r["zero"]), r["n_support"]] + flat + [0] * (2 * TERMS - len(flat))
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
