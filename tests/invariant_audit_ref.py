"""An independent restatement of the invariant audit's contract (include/vgpu.h, "Invariant audit").  The invariant space is the numpy RREF of
the augmented matrix (1 | M) over F_p, the canonical vector of every non-pivot column read off it.  Enforcement at a row is judged on the
NULL SPACE side: c = (l_1 .. l_w) is enforced iff c . v = 0 for every v of a spanning set of the null space of the row's Jacobian.  For the
BasicMachine's chips that spanning set comes from tests/rank_audit_ref.py (chip_rows: exact interpolation of the oracle's own chip
transcription, which shares no code with valida_amd/csrc): e_z for every zero column z and the full null vector of every other loose column —
every non-pivot column is loose, so these span the null space.  For captured AIRs the caller states the Jacobian in closed form
(`jacobians`: chip -> (constraints, interactions, row -> matrix)) and the null space is computed here."""
import numpy as np

import constraint_audit_ref as car
import rank_audit_ref as rar

NUM_CHIPS = 14
P = 2013265921
MAGIC = 0x31524956


def rref(A):
    """(R, pivot columns) of a uint64 matrix over F_p; every row is eliminated at once per pivot."""
    R = np.unique(A % P, axis=0)  # the row space is that of the distinct rows
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
        f = R[:, c].copy()
        f[i] = 0
        R = (R + (P - f)[:, None] * R[i][None, :] % P) % P
        piv.append(c)
        i += 1
        if i == rows:
            break
    return R[:i], piv


def invariants(t):
    """rho_A and {non-pivot main column f: canonical vector l as a list of w + 1 ints} of one trace."""
    n, w = t.shape
    A = np.concatenate([np.ones((n, 1), dtype=np.uint64), t.astype(np.uint64)], axis=1)
    R, piv = rref(A)
    assert piv[0] == 0
    out = {}
    for f in range(1, w + 1):
        if f in piv:
            continue
        l = [0] * (w + 1)
        l[f] = 1
        for i, p_ in enumerate(piv):
            l[p_] = (P - int(R[i, f])) % P
        assert all(l[p_] == 0 for p_ in piv if p_ > f)
        assert not ((A * np.array(l, dtype=np.uint64)[None, :]) % P).sum(axis=1).astype(np.uint64).__mod__(P).any()
        out[f - 1] = l
    return len(piv), out


def null_spanning(J, w):
    """A spanning set of { v : J v = 0 } as dense vectors."""
    J = np.asarray(J, dtype=np.uint64).reshape(-1, w)
    if J.shape[0] == 0:
        return [[int(k == f) for k in range(w)] for f in range(w)]
    R, piv = rref(J)
    vs = []
    for f in range(w):
        if f in piv:
            continue
        v = [0] * w
        v[f] = 1
        for i, p_ in enumerate(piv):
            v[p_] = (P - int(R[i, f])) % P
        vs.append(v)
    return vs


def _oracle_spans(machine, chip, t, p):
    w = t.shape[1]
    K, M, rows = rar.chip_rows(machine, chip, t, p)
    out, done = [], {}
    for rank, zero, loose, vectors in rows:
        key = id(vectors)  # chip_rows shares one analysis among rows of equal Jacobians
        if key not in done:
            vs = [[int(k == z) for k in range(w)] for z in zero]
            for c, terms in vectors.items():
                v = [0] * w
                for col, coef in terms:
                    v[col] = coef
                vs.append(v)
            assert len(set(map(tuple, vs))) >= w - rank
            done[key] = np.array(vs, dtype=np.uint64).reshape(-1, w)
        out.append(done[key])
    return K, M, out


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None, jacobians=None):
    """The contract's report as InvariantReport's attributes.  jacobians: None for the BasicMachine, otherwise per chip (K, M, fn(row) -> J_r)."""
    prep_of = dict(preprocessed)
    blocks, entries = [], []
    for chip in range(len(main)):
        t = np.ascontiguousarray(main[chip], dtype=np.uint32)
        n, w = t.shape
        audited = chips is None or chip in chips
        p = np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None
        if jacobians is None:
            K, M = car.n_constraints(chip, t, p), len(machine.interactions(chip))
        else:
            K, M = jacobians[chip][0], jacobians[chip][1]
        b = dict(chip=chip, width=w, constraints=K, interactions=M, audited=audited, height=n, rank=0, invariants=0, constant_columns=0, relations=0, every=0, some=0, never=0)
        if audited and w:
            rank, inv = invariants(t)
            b["rank"], b["invariants"] = rank, len(inv)
            spans = None
            if inv:
                if jacobians is None:
                    spans = _oracle_spans(machine, chip, t, p)[2]
                else:
                    spans = [np.array(null_spanning(jacobians[chip][2](r), w), dtype=np.uint64).reshape(-1, w) for r in range(n)]
            for f in sorted(inv):
                l = inv[f]
                c = np.array(l[1:], dtype=np.uint64)
                terms = [(k, x) for k, x in enumerate(l[1:]) if x]
                verdict = {}
                free = []
                for r in range(n):
                    V = spans[r]
                    key = id(V)
                    if key not in verdict:
                        verdict[key] = bool(((V * c[None, :]) % P).sum(axis=1).__mod__(P).any()) if V.shape[0] else False
                    if verdict[key]:
                        free.append(r)
                kind = "relation" if len(terms) > 1 else "constant"
                b["relations" if kind == "relation" else "constant_columns"] += 1
                b["every" if not free else ("never" if len(free) == n else "some")] += 1
                entries.append(dict(chip=chip, column=f, kind=kind, l0=l[0], support=len(terms), terms=terms[:max_terms], enforced_rows=n - len(free), free_rows=len(free),
                                    rows=free[:max_rows_per_entry]))
        blocks.append(b)
    return dict(max_terms=max_terms, truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4, max_terms=8):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry], terms=e["terms"][:max_terms]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["free_rows"], max_rows_per_entry) and len(e["terms"]) == min(e["support"], max_terms) for e in entries)
    return dict(want, max_terms=max_terms, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def assert_report_equals(rep, want):
    """An InvariantReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.max_terms, rep.truncated, rep.total_entries, rep.reported) == (want["max_terms"], want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    assert rep.entries == want["entries"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [MAGIC, 0, want["max_terms"], int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"])]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"])
        w += [c["rank"], c["invariants"], c["constant_columns"], c["relations"], c["every"], c["some"], c["never"], 0]
    for e in want["entries"]:
        w += [e["chip"], e["column"], int(e["kind"] == "relation"), e["l0"], e["support"], len(e["terms"]), len(e["rows"]), 0] + u64(e["enforced_rows"]) + u64(e["free_rows"])
        w += [x for term in e["terms"] for x in term] + list(e["rows"])
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
