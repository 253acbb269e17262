"""An independent restatement of the product audit's contract (include/vgpu.h, "Product audit").  The pivot columns Pi are those of the numpy
RREF of the augmented matrix (1 | M) over F_p.  A pair (i, j) of independent columns is judged by the numpy RREF of (the Pi columns of A | the
product column): it is a relation iff the last column is no pivot, and beta is read off the RREF.  The pairs of a chip share the elimination
of the Pi columns (every product column is carried along as a right-hand side, none is ever a pivot of another), which is the same RREF per
pair at a fraction of the time; no inverse and no basis rows, the product's method, occur.  Enforcement at a row is judged on the NULL SPACE
side: g_r is enforced iff g_r . v = 0 for every v of a spanning set of the null space of the row's Jacobian, which tests/rank_audit_ref.py
(chip_rows) gives for the BasicMachine's chips, as tests/invariant_audit_ref.py does it; for captured AIRs the caller states the Jacobian in
closed form (`jacobians`: chip -> (constraints, interactions, row -> matrix))."""
import numpy as np

import constraint_audit_ref as car
import invariant_audit_ref as iar

P = 2013265921
MAGIC = 0x31525156
KINDS = ("boolean", "zero", "select", "other")


def relations(t):
    """(Pi as augmented columns, {(i, j): beta as a list of w + 1 ints}) of one trace; i <= j main columns, both independent."""
    n, w = t.shape
    A = np.concatenate([np.ones((n, 1), dtype=np.uint64), t.astype(np.uint64) % P], axis=1)
    _, piv = iar.rref(A)
    assert piv[0] == 0
    ind = [p_ - 1 for p_ in piv[1:]]
    pairs = [(i, j) for a, i in enumerate(ind) for j in ind[a:]]
    if not pairs:
        return piv, {}
    rho = len(piv)
    Y = np.stack([A[:, 1 + i] * A[:, 1 + j] % P for i, j in pairs], axis=1)
    R = np.concatenate([A[:, piv], Y], axis=1)
    for c in range(rho):  # the Pi columns are independent: each of them gets a pivot, the product columns only follow
        k = c + int(np.nonzero(R[c:, c])[0][0])
        if k != c:
            R[[c, k]] = R[[k, c]]
        R[c] = R[c] * pow(int(R[c, c]), P - 2, P) % P
        f = R[:, c].copy()
        f[c] = 0
        R = (R + (P - f)[:, None] * R[c][None, :] % P) % P
    out = {}
    for x, (i, j) in enumerate(pairs):
        if R[rho:, rho + x].any():  # the product column would be a pivot
            continue
        beta = [0] * (w + 1)
        for a, p_ in enumerate(piv):
            beta[p_] = int(R[a, rho + x])
        assert not ((A * np.array(beta, dtype=np.uint64)[None, :] % P).sum(axis=1) % P != Y[:, x]).any()
        out[(i, j)] = beta
    return piv, out


def kind_of(i, j, beta):
    unit = lambda k: all(b == int(c == k + 1) for c, b in enumerate(beta))
    if not any(beta):
        return "zero"
    if i == j and unit(i):
        return "boolean"
    if i != j and (unit(i) or unit(j)):
        return "select"
    return "other"


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None, jacobians=None):
    """The contract's report as ProductReport's attributes.  jacobians: None for the BasicMachine, otherwise per chip (K, M, fn(row) -> J_r)."""
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
        b = dict(chip=chip, width=w, constraints=K, interactions=M, audited=audited, height=n, rank=0, independent=0, pairs=0, relations=0, boolean=0, zero=0, select=0, other=0,
                 every=0, some=0, never=0)
        if audited and w:
            piv, rel = relations(t)
            q = len(piv) - 1
            b["rank"], b["independent"], b["pairs"], b["relations"] = len(piv), q, q * (q + 1) // 2, len(rel)
            groups = None
            if rel:
                if jacobians is None:
                    spans = iar._oracle_spans(machine, chip, t, p)[2]
                else:
                    spans = [np.array(iar.null_spanning(jacobians[chip][2](r), w), dtype=np.uint64).reshape(-1, w) for r in range(n)]
                groups = {}  # rows of one spanning set (chip_rows shares one analysis among rows of equal Jacobians)
                for r in range(n):
                    groups.setdefault(id(spans[r]), (spans[r], []))[1].append(r)
            tt = t.astype(np.uint64) % P
            for (i, j) in sorted(rel):
                beta = rel[(i, j)]
                neg = np.array([(P - x) % P for x in beta[1:]], dtype=np.uint64)
                xi, xj = tt[:, i], tt[:, j]
                # g_r = neg + x_j e_i + x_i e_j
                gi = (neg[i] + xj + (xi if i == j else 0)) % P
                gj = (neg[j] + xi + (xj if i == j else 0)) % P
                rest = neg.copy()
                rest[i] = rest[j] = 0
                flat = np.zeros(n, dtype=bool) if rest.any() else ((gi == 0) & (gj == 0))
                free = np.zeros(n, dtype=bool)
                for V, rows in groups.values():
                    if not V.shape[0]:
                        continue
                    rows = np.array(rows)
                    base = (V * neg[None, :] % P).sum(axis=1) % P  # V . neg
                    if i == j:
                        dots = (base[:, None] + V[:, i][:, None] * (2 * xi[rows] % P)[None, :]) % P
                    else:
                        dots = (base[:, None] + V[:, i][:, None] * xj[rows][None, :] % P + V[:, j][:, None] * xi[rows][None, :] % P) % P
                    free[rows] = dots.any(axis=0)
                assert not (free & flat).any()
                free = [int(r) for r in np.nonzero(free)[0]]
                terms = [(k, x) for k, x in enumerate(beta[1:]) if x]
                kind = kind_of(i, j, beta)
                b[kind] += 1
                b["every" if not free else ("never" if len(free) == n else "some")] += 1
                entries.append(dict(chip=chip, i=i, j=j, kind=kind, b0=beta[0], support=len(terms), terms=terms[:max_terms], enforced_rows=n - len(free), free_rows=len(free),
                                    flat_rows=int(flat.sum()), rows=free[:max_rows_per_entry]))
        blocks.append(b)
    return dict(max_terms=max_terms, truncated=len(entries) > max_entries, total_entries=len(entries), chips=blocks, entries=entries[:max_entries])


def recut(want, max_entries=1024, max_rows_per_entry=4, max_terms=8):
    """audit()'s dict made with limits at least as large, cut to smaller limits (the counts do not depend on the limits)."""
    entries = [dict(e, rows=e["rows"][:max_rows_per_entry], terms=e["terms"][:max_terms]) for e in want["entries"]]
    assert not want["truncated"] and all(len(e["rows"]) == min(e["free_rows"], max_rows_per_entry) and len(e["terms"]) == min(e["support"], max_terms) for e in entries)
    return dict(want, max_terms=max_terms, truncated=len(entries) > max_entries, entries=entries[:max_entries])


def assert_report_equals(rep, want):
    """A ProductReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.max_terms, rep.truncated, rep.total_entries, rep.reported) == (want["max_terms"], want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    for got, exp in zip(rep.entries, want["entries"]):
        assert got == exp, (got, exp)
    assert len(rep.entries) == len(want["entries"])


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [MAGIC, 0, want["max_terms"], int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"])]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"])
        w += [c["rank"], c["pairs"], c["relations"], c["boolean"], c["zero"], c["select"], c["other"], c["every"], c["some"], c["never"]]
    for e in want["entries"]:
        w += [e["chip"], e["i"], e["j"], KINDS.index(e["kind"]), e["b0"], e["support"], len(e["terms"]), len(e["rows"])]
        w += u64(e["enforced_rows"]) + u64(e["free_rows"]) + u64(e["flat_rows"]) + [0, 0]
        w += [x for term in e["terms"] for x in term] + list(e["rows"])
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
