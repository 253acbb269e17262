"""An independent restatement of the transition audit's contract (include/vgpu.h, "Transition audit").  The windows are the numpy matrix
(1 | M[:-1] | M[1:]); a gate's space is the numpy RREF (tests/invariant_audit_ref.py: rref) of the windows on which it holds, the canonical
vector of every non-pivot column read off it.  The verdict at a window is judged on the NULL SPACE side, as the invariant audit's reference
does: a half c of a vector is outside the row space of J_r iff c . v != 0 for some v of a spanning set of the null space of J_r.  For the
BasicMachine's chips the spanning sets come from tests/rank_audit_ref.py through invariant_audit_ref._oracle_spans (the oracle's own chip
transcription, no code shared with valida_amd/csrc); for captured AIRs the caller states the Jacobian in closed form (`jacobians`: chip ->
(constraints, interactions, row -> matrix))."""
import numpy as np

import constraint_audit_ref as car
import invariant_audit_ref as iar

P = 2013265921
MAGIC = 0x31525456
KINDS = ("constant", "one_block", "both_blocks")


def windows(t):
    t = t.astype(np.uint64) % P
    return np.concatenate([np.ones((t.shape[0] - 1, 1), dtype=np.uint64), t[:-1], t[1:]], axis=1)


def gate_list(A):
    """[(window column, value, windows)] of a window matrix, gate 0 = (0, 0, all) first."""
    out = [(0, 0, A.shape[0])]
    for j in range(1, A.shape[1]):
        col = A[:, j]
        ones = int((col == 1).sum())
        if ((col == 0) | (col == 1)).all() and 0 < ones < A.shape[0]:
            out += [(j, 1, ones), (j, 0, A.shape[0] - ones)]
    return out


def space(A):
    """(pivot columns, {non-pivot column f: canonical vector as a list of ints}) of the rows of A."""
    AW = A.shape[1]
    R, piv = iar.rref(A)
    out = {}
    for f in range(AW):
        if f in piv:
            continue
        l = [0] * AW
        l[f] = 1
        for i, p_ in enumerate(piv):
            l[p_] = (P - int(R[i, f])) % P
        assert all(l[p_] == 0 for p_ in piv if p_ > f)
        out[f] = l
    return piv, out


def _span_index(machine, chip, t, p, jacobian):
    """(distinct spanning sets, index of each row's set)."""
    n, w = t.shape
    if jacobian is None:
        spans = iar._oracle_spans(machine, chip, t, p)[2]
        keys = [id(V) for V in spans]
    else:
        cache, spans, keys = {}, [], []
        for r in range(n):
            J = np.asarray(jacobian(r), dtype=np.uint64).reshape(-1, w)
            k = J.tobytes()
            if k not in cache:
                cache[k] = np.array(iar.null_spanning(J, w), dtype=np.uint64).reshape(-1, w)
            spans.append(cache[k])
            keys.append(k)
    index, distinct, idx = {}, [], np.zeros(n, dtype=np.int64)
    for r, k in enumerate(keys):
        if k not in index:
            index[k] = len(distinct)
            distinct.append(spans[r])
        idx[r] = index[k]
    return distinct, idx


def _outside(distinct, c):
    c = np.array(c, dtype=np.uint64)
    return np.array([bool(((V * c[None, :]) % P).sum(axis=1).__mod__(P).any()) if V.shape[0] else False for V in distinct], dtype=bool)


def audit(machine, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, min_gate_windows=64, max_gates=256, chips=None, jacobians=None):
    """The contract's report as TransitionReport's attributes.  jacobians: None for the BasicMachine, otherwise per chip (K, M, fn(row) -> J_r)."""
    prep_of = dict(preprocessed)
    blocks, gates, entries, judge = [], [], [], {}
    for chip in range(len(main)):
        t = np.ascontiguousarray(main[chip], dtype=np.uint32)
        n, w = t.shape
        audited = chips is None or chip in chips
        p = np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None
        if jacobians is None:
            K, M = car.n_constraints(chip, t, p), len(machine.interactions(chip))
        else:
            K, M = jacobians[chip][0], jacobians[chip][1]
        b = dict(chip=chip, width=w, constraints=K, interactions=M, audited=audited, height=n, n_bool=0, n_gates=0, gates_listed=0, gates_audited=0, rank=0, dim=0, local_only=0,
                 next_only=0, transitions=0, gated=0)
        blocks.append(b)
        if not (audited and w and n >= 2):
            continue
        A = windows(t)
        AW = 2 * w + 1
        gl = gate_list(A)
        b["n_gates"], b["n_bool"] = len(gl), (len(gl) - 1) // 2
        piv0 = None
        for j, v, cnt in gl[:max_gates]:
            g = dict(chip=chip, column=j, value=v, audited=j == 0 or cnt >= min_gate_windows, windows=cnt, rank=0, dim=0, entries=0)
            gates.append(g)
            b["gates_listed"] += 1
            if not g["audited"]:
                continue
            b["gates_audited"] += 1
            mask = np.ones(A.shape[0], dtype=bool) if j == 0 else A[:, j] == v
            piv, vec = space(A[mask])
            g["rank"], g["dim"] = len(piv), AW - len(piv)
            if j == 0:
                piv0 = set(piv)
                b["rank"], b["dim"] = g["rank"], g["dim"]
            assert set(piv) <= piv0
            for f in sorted(vec):
                l = vec[f]
                loc, nxt = any(l[1:w + 1]), any(l[w + 1:])
                if j == 0:
                    if f <= w:
                        b["local_only"] += 1
                        continue
                    if not loc:
                        b["next_only"] += 1
                        continue
                    b["transitions"] += 1
                else:
                    if f not in piv0 or f == j:
                        continue
                    b["gated"] += 1
                g["entries"] += 1
                terms = [(k, x) for k, x in enumerate(l) if x and k]
                assert not (((A[mask] * np.array(l, dtype=np.uint64)[None, :]) % P).sum(axis=1) % P).any()
                entries.append(dict(chip=chip, gate=(j, v) if j else None, column=f, kind=KINDS[0 if len(terms) == 1 else (2 if loc and nxt else 1)], l0=l[0], support=len(terms),
                                    terms=terms[:max_terms], free_windows=0, held_windows=0, rows=[]))
                judge[len(entries) - 1] = (l, mask)
    total = len(entries)
    entries = entries[:max_entries]
    spans = {}
    for i, e in enumerate(entries):
        chip = e["chip"]
        t = np.ascontiguousarray(main[chip], dtype=np.uint32)
        w = t.shape[1]
        if chip not in spans:
            p = np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None
            spans[chip] = _span_index(machine, chip, t, p, None if jacobians is None else jacobians[chip][2])
        distinct, idx = spans[chip]
        l, mask = judge[i]
        fa, fb = _outside(distinct, l[1:w + 1]), _outside(distinct, l[w + 1:])
        free = (fa[idx[:-1]] | fb[idx[1:]]) & mask
        rows = np.nonzero(free)[0]
        e["free_windows"], e["held_windows"], e["rows"] = int(rows.size), int(mask.sum() - rows.size), [int(r) for r in rows[:max_rows_per_entry]]
    return dict(max_terms=max_terms, min_gate_windows=min_gate_windows, max_gates=max_gates, truncated=total > max_entries, total_entries=total, chips=blocks, gates=gates,
                entries=entries)


def assert_report_equals(rep, want):
    """A TransitionReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.max_terms, rep.min_gate_windows, rep.max_gates, rep.truncated, rep.total_entries, rep.reported) == (
        want["max_terms"], want["min_gate_windows"], want["max_gates"], want["truncated"], want["total_entries"], len(want["entries"]))
    for got, exp in zip(rep.chips, want["chips"]):
        assert got == exp, (got, exp)
    for got, exp in zip(rep.gates, want["gates"]):
        assert got == exp, (got, exp)
    assert len(rep.gates) == len(want["gates"])
    for got, exp in zip(rep.entries, want["entries"]):
        assert got == exp, (got, exp)


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [MAGIC, 0, want["max_terms"], int(want["truncated"])] + u64(want["total_entries"]) + [len(want["entries"]), len(want["chips"]), len(want["gates"]), want["min_gate_windows"],
                                                                                            want["max_gates"], 0]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], int(c["audited"])] + u64(c["height"])
        w += [c["n_bool"], c["n_gates"], c["gates_listed"], c["gates_audited"], c["rank"], c["dim"], c["local_only"], c["next_only"], c["transitions"], c["gated"]]
    for g in want["gates"]:
        w += [g["chip"], g["column"], g["value"], int(g["audited"])] + u64(g["windows"]) + [g["rank"], g["dim"], g["entries"], 0]
    for e in want["entries"]:
        gj, gv = e["gate"] if e["gate"] else (0, 0)
        w += [e["chip"], gj, gv, e["column"], KINDS.index(e["kind"]), e["l0"], e["support"], len(e["terms"]), len(e["rows"]), 0] + u64(e["free_windows"]) + u64(e["held_windows"])
        w += [x for term in e["terms"] for x in term] + list(e["rows"])
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
