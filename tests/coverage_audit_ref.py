"""An independent restatement of the coverage audit's contract (include/vgpu.h, "Coverage audit"), by brute force: the mutation reference's loop
(tests/mutation_audit_ref.py) keeping the SET of detectors instead of one bit.  For every (chip, row, main column, delta) the cell is changed in
a copy of the trace, oracle.pyoracle.eval_constraints — the oracle's own transcription of the chips, which shares no code with
valida_amd/csrc/chips — is called on rows r and (r - 1) mod n of the changed trace and compared with its values on the unchanged trace
(constraint k kills when it is NEWLY non-zero at one of them), and Machine.interactions(chip) is evaluated on the row before and after
(interaction m kills when its record — (count, fields) when count != 0, else nothing — differs).  No shortcut: every column is evaluated at both
rows whether or not a constraint reads it.  The one economy is the mutation reference's: the bus records of a row depend on that row alone, so
the interactions are evaluated with numpy over all rows at once on the trace whose whole column has the delta added."""
import numpy as np

import constraint_audit_ref as car
import mutation_audit_ref as mref

NUM_CHIPS = 14
P = 2013265921
NO_ROW = 0xFFFFFFFF


def bus_kills(interactions, m, m2, p):
    """[rows, M] bool: does the record of interaction j differ between trace m and trace m2 on that row?"""
    out = np.zeros((m.shape[0], len(interactions)), dtype=bool)
    for j, it in enumerate(interactions):
        c0, c1 = mref._vcol(it["count"], m, p), mref._vcol(it["count"], m2, p)
        live0, live1 = c0 != 0, c1 != 0
        differ = c0 != c1
        for f in it["fields"]:
            differ |= mref._vcol(f, m, p) != mref._vcol(f, m2, p)
        out[:, j] = (live0 != live1) | (live0 & live1 & differ)
    return out


def chip_cells(machine, chip, trace, prep, deltas):
    """K, M and {(column, delta index): S} with S the [rows, K + M] bool matrix of the detectors that kill the mutation of each row."""
    t = np.ascontiguousarray(trace, dtype=np.uint32).copy()
    p = np.ascontiguousarray(prep, dtype=np.uint32) if prep is not None else None
    n, w = t.shape
    K = car.n_constraints(chip, t, p)
    inter = machine.interactions(chip)
    M = len(inter)
    base = [mref._eval(chip, t, p, q) != 0 for q in range(n)] if K else None
    out = {}
    for c in range(w):
        for di, d in enumerate(deltas):
            S = np.zeros((n, K + M), dtype=bool)
            if K:
                for r in range(n):
                    keep = t[r, c]
                    t[r, c] = (int(keep) + d) % P
                    for q in {r, (r - 1) % n}:
                        S[r, :K] |= (mref._eval(chip, t, p, q) != 0) & ~base[q]
                    t[r, c] = keep
            t2 = t.copy()
            t2[:, c] = (t[:, c].astype(np.uint64) + d) % P
            S[:, K:] = bus_kills(inter, t, t2, p)
            out[(c, di)] = S
    return K, M, out


def audit(machine, main, preprocessed, deltas=(1, P - 1), max_cells=8192):
    """The contract's report as CoverageReport's attributes: dict(deltas, truncated, total_cells, chips=[..], cells=[..])."""
    prep_of = dict(preprocessed)
    deltas = [int(d) for d in deltas]
    D = len(deltas)
    chips, cells = [], []
    for chip in range(NUM_CHIPS):
        t = np.asarray(main[chip])
        n, w = t.shape
        K, M, S = chip_cells(machine, chip, t, prep_of.get(chip), deltas)
        kills, sole = [[0] * D for _ in range(K + M)], [[0] * D for _ in range(K + M)]
        detected = [0] * D
        mine = {}
        for c in range(w):
            for di in range(D):
                s = S[(c, di)]
                size = s.sum(axis=1)
                detected[di] += int((size > 0).sum())
                alone = s & (size == 1)[:, None]
                for det in np.nonzero(s.any(axis=0))[0]:
                    det = int(det)
                    k, so = int(s[:, det].sum()), int(alone[:, det].sum())
                    kills[det][di] += k
                    sole[det][di] += so
                    mine[(det, c, di)] = dict(chip=chip, detector=det, column=c, delta=di, kills=k, sole=so, first_row=int(np.argmax(s[:, det])),
                                              first_sole_row=int(np.argmax(alone[:, det])) if so else NO_ROW)
        cells += [mine[k] for k in sorted(mine)]
        cls = ["dead" if sum(k) == 0 else "shadowed" if sum(s) == 0 else "essential" for k, s in zip(kills, sole)]
        chips.append(dict(chip=chip, width=w, constraints=K, interactions=M, height=n, dead_constraints=cls[:K].count("dead"), shadowed_constraints=cls[:K].count("shadowed"),
                          dead_interactions=cls[K:].count("dead"), shadowed_interactions=cls[K:].count("shadowed"), detected=detected, free=[n * w - x for x in detected],
                          kills=kills, sole=sole))
    return dict(deltas=deltas, truncated=len(cells) > max_cells, total_cells=len(cells), chips=chips, cells=cells[:max_cells])


def recut(want, max_cells=8192):
    """audit()'s dict made with a limit at least as large, cut to a smaller one (the chip blocks and totals do not depend on it)."""
    assert not want["truncated"]
    return dict(want, truncated=len(want["cells"]) > max_cells, cells=want["cells"][:max_cells])


def classes(want, chip):
    """(dead constraints, dead interactions, shadowed constraints, shadowed interactions) of a chip of audit()'s dict, by index."""
    c = want["chips"][chip]
    K = c["constraints"]
    dead = [t for t in range(len(c["kills"])) if sum(c["kills"][t]) == 0]
    shadowed = [t for t in range(len(c["kills"])) if sum(c["kills"][t]) > 0 and sum(c["sole"][t]) == 0]
    return [t for t in dead if t < K], [t - K for t in dead if t >= K], [t for t in shadowed if t < K], [t - K for t in shadowed if t >= K]


def assert_report_equals(rep, want):
    """A CoverageReport (valida_amd) against audit()'s dict made with the same limit."""
    assert (rep.deltas, rep.truncated, rep.total_cells, rep.reported) == (want["deltas"], want["truncated"], want["total_cells"], len(want["cells"]))
    assert rep.chips == want["chips"]
    assert rep.cells == want["cells"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    D = len(want["deltas"])
    w = [0x31524B56, 0, D, int(want["truncated"])] + u64(want["total_cells"]) + [len(want["cells"]), len(want["chips"])] + (want["deltas"] + [0] * 4)[:4]
    for c in want["chips"]:
        w += [c["width"], c["constraints"], c["interactions"], 0] + u64(c["height"])
        w += [c["dead_constraints"], c["shadowed_constraints"], c["dead_interactions"], c["shadowed_interactions"]]
        for i in range(D):
            w += u64(c["detected"][i]) + u64(c["free"][i])
        for t in range(c["constraints"] + c["interactions"]):
            for i in range(D):
                w += u64(c["kills"][t][i]) + u64(c["sole"][t][i])
    for e in want["cells"]:
        w += [e["chip"], e["detector"], e["column"], e["delta"]] + u64(e["kills"]) + u64(e["sole"]) + [e["first_row"], e["first_sole_row"]]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
