"""An independent restatement of the rank audit's contract (include/vgpu.h, "Rank audit").  It uses neither dual numbers nor the product's chips:
the derivative of every constraint by a main cell is taken by EXACT INTERPOLATION of oracle.pyoracle.eval_constraints — the oracle's own
transcription of the chips (oracle/chips.hpp), which shares no code with valida_amd/csrc/chips — on a trace with the one cell set to
M[r][c] + t:  g'(0) = (8 (g(1) - g(-1)) - (g(2) - g(-2))) / 12 mod p, exact for degree <= 4.  A sixth evaluation at t = 3 must agree with the
degree-4 interpolant through t = -2 .. 2 (g(3) = g(-2) - 5 g(-1) + 10 g(0) - 10 g(1) + 5 g(2)); that is asserted on every run, so a chip of
higher degree fails loudly.  Both rows (q = r and q = r - 1) are evaluated for every column: nothing is pruned by which columns a constraint
reads.  The interaction rows come from Machine.interactions.  RREF is plain Gaussian elimination with numpy on uint64 (identical Jacobians are
eliminated once).  The evaluations call the oracle's entry point (oracle_eval_constraints, what pyoracle.eval_constraints wraps) on the rows
of the changed trace in place, as tests/pair_audit_ref.py does."""
import ctypes

import numpy as np

from oracle import pyoracle as po

import constraint_audit_ref as car

NUM_CHIPS = 14
P = 2013265921
MAGIC = 0x31525256
TERMS = 8
INV12 = pow(12, P - 2, P)


def rref(J):
    """(R, pivot columns) of a uint64 matrix over F_p."""
    R = J.copy() % P
    rows, w = R.shape
    piv, i = [], 0
    for c in range(w):
        nz = np.nonzero(R[i:, c])[0]
        if nz.size == 0:
            continue
        k = i + int(nz[0])
        if k != i:
            R[[i, k]] = R[[k, i]]
        R[i] = R[i] * pow(int(R[i, c]), P - 2, P) % P
        for x in range(rows):
            if x != i and R[x, c]:
                R[x] = (R[x] + (P - R[x, c]) * R[i]) % P
        piv.append(c)
        i += 1
        if i == rows:
            break
    return R[:i], piv


def analyse(J, w):
    """Per-row facts of a Jacobian: rank, zero columns, loose columns, {loose non-zero column: null vector as [(column, coefficient)]}."""
    J = J.reshape(-1, w)
    zero = [c for c in range(w) if not J[:, c].any()] if J.shape[0] else list(range(w))
    R, piv = rref(J) if J.shape[0] else (np.zeros((0, w), dtype=np.uint64), [])
    row_of = {c: i for i, c in enumerate(piv)}
    nonpiv = [c for c in range(w) if c not in row_of]
    loose, vectors = [], {}

    def basis(f):
        v = {f: 1}
        for p_, i in row_of.items():
            if R[i, f]:
                v[p_] = (P - int(R[i, f])) % P
        return sorted(v.items())

    for c in range(w):
        if c in row_of:
            others = [f for f in nonpiv if R[row_of[c], f]]
            if not others:
                continue  # pinned
            f = others[0]
        else:
            f = c
        loose.append(c)
        if c not in zero:
            vectors[c] = basis(f)
    return len(piv), zero, loose, vectors


def _vcol(v, m, p):
    const, terms = v
    acc = np.full(m.shape[0], const % P, dtype=np.uint64)
    for is_prep, col, weight in terms:
        acc = (acc + (p if is_prep else m)[:, col].astype(np.uint64) % P * (weight % P)) % P
    return acc


def _weights(v, w):
    row = np.zeros(w, dtype=np.uint64)
    for is_prep, col, weight in v[1]:
        if not is_prep:
            row[col] = (row[col] + weight % P) % P
    return row


_cache = {}


def chip_rows(machine, chip, trace, prep):
    """K, M and per row (rank, zero columns, loose columns, vectors) of one chip.  Computed once per (chip, trace contents)."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    key = (chip, t.shape, t.tobytes(), p.tobytes() if p is not None else None)
    if key not in _cache:
        _cache[key] = _chip_rows(machine, chip, t, p)
    return _cache[key]


def _chip_rows(machine, chip, t, p):
    n, w = t.shape
    K = car.n_constraints(chip, t, p)
    inter = machine.interactions(chip)
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

    base = [ev(q) for q in range(n)] if K else None
    counts = [_vcol(it["count"], t, p) for it in inter]
    bus = [[_weights(it["count"], w)] + [_weights(fl, w) for fl in it["fields"]] for it in inter]
    done, out = {}, []
    for r in range(n):
        blocks = []
        if K:
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
                    D[:, c] = ((8 * ((g[1] - g[-1]) % P) - (g[2] - g[-2]) % P) % P * INV12 % P).astype(np.uint64)
                blocks.append(D)
        for m, it in enumerate(inter):
            blocks.append(np.stack(bus[m] if counts[m][r] else bus[m][:1]))
        J = np.concatenate(blocks) if blocks else np.zeros((0, w), dtype=np.uint64)
        k = J.tobytes()
        if k not in done:
            done[k] = analyse(J, w)
        out.append(done[k])
    return K, len(inter), out


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The contract's report as RankReport's attributes."""
    prep_of = dict(preprocessed)
    blocks, entries = [], []
    for chip in range(NUM_CHIPS):
        t = np.asarray(main[chip])
        n, w = t.shape
        audited = chips is None or chip in chips
        K = car.n_constraints(chip, np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None)
        M = len(machine.interactions(chip))
        b = dict(chip=chip, width=w, constraints=K, interactions=M, audited=audited, height=n, nullity=0, zero=0, coupled_rows=0, max_nullity=0, loose_columns=0,
                 pinned_columns=0, coupled_columns=0, loose=[0] * w, zeros=[0] * w)
        if audited:
            K, M, rows = chip_rows(machine, chip, t, prep_of.get(chip))
            listed = {}
            for r, (rank, zero, loose, vectors) in enumerate(rows):
                b["nullity"] += w - rank
                b["zero"] += len(zero)
                b["coupled_rows"] += int(w - rank > len(zero))
                b["max_nullity"] = max(b["max_nullity"], w - rank)
                assert set(zero) <= set(loose) and set(vectors) == set(loose) - set(zero) and (w - rank > len(zero)) == bool(vectors)
                for c in loose:
                    b["loose"][c] += 1
                for c in zero:
                    b["zeros"][c] += 1
                for c, v in vectors.items():
                    listed.setdefault(c, []).append(dict(row=r, n_support=len(v), terms=v[:TERMS]))
            b["loose_columns"] = sum(1 for x in b["loose"] if x)
            b["pinned_columns"] = w - b["loose_columns"]
            b["coupled_columns"] = len(listed)
            for c in sorted(listed):
                entries.append(dict(chip=chip, column=c, coupled=len(listed[c]), rows=listed[c][:max_rows_per_entry]))
        blocks.append(b)
    return dict(truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["coupled"], max_rows_per_entry) for e in entries)
    return dict(want, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def assert_report_equals(rep, want):
    """A RankReport (valida_amd) against audit()'s dict made with the same limits."""
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
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"]) + u64(c["nullity"]) + u64(c["zero"]) + u64(c["coupled_rows"])
        w += [c["max_nullity"], c["loose_columns"], c["pinned_columns"], c["coupled_columns"]]
        for k in range(c["width"]):
            w += u64(c["loose"][k]) + u64(c["zeros"][k])
    for e in want["entries"]:
        w += [e["chip"], e["column"], len(e["rows"]), 0] + u64(e["coupled"])
        for r in e["rows"]:
            flat = [x for term in r["terms"] for x in term]
            w += [r["row"], r["n_support"]] + flat + [0] * (2 * TERMS - len(flat))
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
