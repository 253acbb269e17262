"""An independent restatement of the field audit's contract (include/vgpu.h, "Field audit").  The Jacobian rows are the rank audit
reference's: the derivative of every constraint by a main cell by EXACT INTERPOLATION of the oracle's own chips (rank_audit_ref: the same five
evaluations per cell and the same degree check, its helpers imported), the count and field rows from Machine.interactions.  The leave-one-out
question is asked literally: per live record and per field one numpy RREF of S = C + counts + the record's OTHER fields, then the field's row
reduced against it; nothing is shared between the fields of a record (identical (S, phi) pairs are eliminated once)."""
import ctypes

import numpy as np

from oracle import pyoracle as po

import constraint_audit_ref as car
import rank_audit_ref as rr

NUM_CHIPS = rr.NUM_CHIPS
P = rr.P
MAGIC = 0x31414656
TERMS = 8


def constraint_rows(chip, t, p):
    """K and a function r -> the constraint rows of J_r, a (rows, w) uint64 matrix: q = r, then q = r - 1 (n = 1: one evaluation).  Rows are
    interpolated when asked for: a row without a live record is never looked at."""
    n, w = t.shape
    K = car.n_constraints(chip, t, p)
    if not K:
        return K, lambda r: np.zeros((0, w), dtype=np.uint64)
    f = po.lib().oracle_eval_constraints
    f.restype = ctypes.c_uint32
    vals = np.zeros(max(1, K), dtype=np.uint32)
    none = np.zeros(8, dtype=np.uint32)
    tb, pb, vp, u = t.ctypes.data, (p.ctypes.data if p is not None else none.ctypes.data), ctypes.c_void_p(vals.ctypes.data), ctypes.c_uint32
    ts, pstr = t.strides[0], (p.strides[0] if p is not None else 0)
    assert t.flags.c_contiguous and (p is None or p.flags.c_contiguous)

    def ev(row):
        nx = (row + 1) % n
        f(u(chip), ctypes.c_void_p(tb + row * ts), ctypes.c_void_p(tb + nx * ts), ctypes.c_void_p(pb + row * pstr), ctypes.c_void_p(pb + nx * pstr), u(int(row == 0)), u(int(row == n - 1)),
          u(int(row != n - 1)), vp, u(K))
        return vals[:K].astype(np.int64)

    base = [ev(q) for q in range(n)]

    def rows(r):
        blocks = []
        for q in ([r] if n == 1 else [r, (r - 1) % n]):
            D = np.zeros((K, w), dtype=np.uint64)
            for c in range(w):
                keep = int(t[r, c])
                g = {0: base[q]}
                for x in (1, -1, 2, -2, 3):
                    t[r, c] = (keep + x) % P
                    g[x] = ev(q)
                t[r, c] = keep
                assert np.array_equal(g[3] % P, (g[-2] - 5 * g[-1] + 10 * g[0] - 10 * g[1] + 5 * g[2]) % P), "a constraint of chip %d has degree above 4 in one cell" % chip
                D[:, c] = ((8 * ((g[1] - g[-1]) % P) - (g[2] - g[-2]) % P) % P * rr.INV12 % P).astype(np.uint64)
            blocks.append(D)
        return np.concatenate(blocks)

    return K, rows


def leave_one_out(S, phi, w):
    """None when phi lies in the row space of S, else the direction v as [(column, coefficient)]: R = RREF(S), the smallest non-pivot column f
    with phi . b_f != 0, v = b_f / (phi . b_f)."""
    R, piv = rr.rref(S) if S.shape[0] else (np.zeros((0, w), dtype=np.uint64), [])
    row_of = {c: i for i, c in enumerate(piv)}
    for f in range(w):
        if f in row_of:
            continue
        b = {f: 1}
        for p_, i in row_of.items():
            if R[i, f]:
                b[p_] = (P - int(R[i, f])) % P
        dot = sum(int(phi[c]) * x for c, x in b.items()) % P
        if dot:
            inv = pow(dot, P - 2, P)
            return sorted((c, x * inv % P) for c, x in b.items())
    return None


_cache = {}


def chip_rows(machine, chip, trace, prep):
    """Per row of one chip: {interaction: {field: direction}} for its live interactions (an empty dict: live, nothing floats)."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    key = (chip, t.shape, t.tobytes(), p.tobytes() if p is not None else None)
    if key not in _cache:
        n, w = t.shape
        inter = machine.interactions(chip)
        K, C = constraint_rows(chip, t, p) if inter else (0, None)
        counts = [rr._vcol(it["count"], t, p) for it in inter]
        psi = [rr._weights(it["count"], w) for it in inter]
        phi = [[rr._weights(fl, w) for fl in it["fields"]] for it in inter]
        done, rows = {}, []
        for r in range(n):
            row, Cr = {}, None
            for m in range(len(inter)):
                if not counts[m][r]:
                    continue
                row[m] = {}
                Cr = C(r) if Cr is None else Cr
                for j, ph in enumerate(phi[m]):
                    if not ph.any():
                        continue  # a constant field
                    S = np.concatenate([Cr] + [np.stack(psi)] + ([np.stack([x for i, x in enumerate(phi[m]) if i != j])] if len(phi[m]) > 1 else []))
                    k = (S.tobytes(), ph.tobytes())
                    if k not in done:
                        done[k] = leave_one_out(S, ph, w)
                    if done[k] is not None:
                        row[m][j] = done[k]
            rows.append(row)
        _cache[key] = rows
    return _cache[key]


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The contract's report as FieldReport's attributes."""
    prep_of = dict(preprocessed)
    blocks, entries = [], []
    for chip in range(len(main)):
        t = np.asarray(main[chip])
        n, w = t.shape
        audited = chips is None or chip in chips
        inter = machine.interactions(chip)
        K = car.n_constraints(chip, np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None)
        recs = [dict(interaction=m, is_send=bool(it["send"]), is_global=bool(it["global"]), bus_index=it["bus"], fields=len(it["fields"]), live_rows=0,
                     constant=[not rr._weights(fl, w).any() for fl in it["fields"]], floating=[0] * len(it["fields"])) for m, it in enumerate(inter)]
        b = dict(chip=chip, width=w, constraints=K, interactions=len(inter), audited=audited, height=n, live_records=0, floating_fields=0, floating_rows=0, records=recs)
        if audited:
            listed = {}
            for r, row in enumerate(chip_rows(machine, chip, t, prep_of.get(chip))):
                b["live_records"] += len(row)
                b["floating_rows"] += int(any(row.values()))
                for m, fl in row.items():
                    recs[m]["live_rows"] += 1
                    b["floating_fields"] += len(fl)
                    for j, v in fl.items():
                        recs[m]["floating"][j] += 1
                        listed.setdefault((m, j), []).append(dict(row=r, n_support=len(v), terms=v[:TERMS]))
            for (m, j) in sorted(listed):
                entries.append(dict(chip=chip, interaction=m, field=j, floating=len(listed[(m, j)]), rows=listed[(m, j)][:max_rows_per_entry]))
        blocks.append(b)
    return dict(truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["floating"], max_rows_per_entry) for e in entries)
    return dict(want, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def assert_report_equals(rep, want):
    """A FieldReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.truncated, rep.total_entries, rep.reported) == (want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    assert rep.entries == want["entries"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [MAGIC, 0, TERMS, int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"])]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"]) + u64(c["live_records"]) + u64(c["floating_fields"]) + u64(c["floating_rows"])
        for r in c["records"]:
            w += [int(r["is_send"]), int(r["is_global"]), r["bus_index"], r["fields"]] + u64(r["live_rows"])
            for j in range(r["fields"]):
                w += [int(r["constant"][j])] + u64(r["floating"][j])
    for e in want["entries"]:
        w += [e["chip"], e["interaction"], e["field"], len(e["rows"])] + u64(e["floating"])
        for r in e["rows"]:
            flat = [x for term in r["terms"] for x in term]
            w += [r["row"], r["n_support"]] + flat + [0] * (2 * TERMS - len(flat))
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
