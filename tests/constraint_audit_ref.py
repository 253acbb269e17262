"""An independent restatement of the constraint audit's contract (include/vgpu.h, "Constraint audit"): a Python loop over the rows of every chip
that calls oracle.pyoracle.eval_constraints — the oracle's own transcription of the chips (oracle/chips.hpp), which shares no code with
valida_amd/csrc/chips — on the trace domain itself: next = (row + 1) mod height, is_first / is_last / is_transition as 0/1 values.  Produces the
report as plain Python values; about 27 microseconds per row, so whole witnesses up to cpu height 2^18 are affordable and larger ones are done on
row windows (`rows=`)."""
import numpy as np

from oracle import pyoracle as po

NUM_CHIPS = 14


def chip_rows(chip, trace, prep, rows=None):
    """{row: values of all constraints of `chip` on that row} for the given rows (default: all); {} for a chip without constraints."""
    n = trace.shape[0]
    out = {}
    for r in (range(n) if rows is None else rows):
        r = int(r)
        nx = (r + 1) % n
        v = po.eval_constraints(chip, trace[r], trace[nx], prep[r] if prep is not None else None, prep[nx] if prep is not None else None,
                                is_first=int(r == 0), is_last=int(r == n - 1), is_transition=int(r != n - 1))
        if v.size == 0:
            return {}
        out[r] = v
    return out


def n_constraints(chip, trace, prep):
    return int(po.eval_constraints(chip, trace[0], trace[1 % trace.shape[0]], prep[0] if prep is not None else None, prep[1 % trace.shape[0]] if prep is not None else None).size)


def audit(main, preprocessed, max_constraints=64, max_rows_per_constraint=4):
    """The contract's report: dict(satisfied, truncated, total_failing, chips=[dict(chip, constraints, failing_constraints, height, failing_rows)],
    constraints=[dict(chip, constraint, failing_rows, rows=[(row, value)])])."""
    prep_of = dict(preprocessed)
    chips, entries = [], []
    for chip in range(NUM_CHIPS):
        t = np.ascontiguousarray(main[chip], dtype=np.uint32)
        p = np.ascontiguousarray(prep_of[chip], dtype=np.uint32) if chip in prep_of else None
        K = n_constraints(chip, t, p)
        count, first, failing_rows = [0] * K, [[] for _ in range(K)], 0
        if K:
            for r, v in chip_rows(chip, t, p).items():
                bad = np.nonzero(v)[0]
                failing_rows += bool(bad.size)
                for k in bad:
                    count[k] += 1
                    if len(first[k]) < max_rows_per_constraint:
                        first[k].append((r, int(v[k])))
        chips.append(dict(chip=chip, constraints=K, failing_constraints=sum(1 for c in count if c), height=int(t.shape[0]), failing_rows=failing_rows))
        entries += [dict(chip=chip, constraint=k, failing_rows=count[k], rows=first[k]) for k in range(K) if count[k]]
    return dict(satisfied=not entries, truncated=len(entries) > max_constraints, total_failing=len(entries), chips=chips, constraints=entries[:max_constraints])


def assert_report_equals(rep, want):
    """A ConstraintReport (valida_amd) against audit()'s dict made with the same limits."""
    assert (rep.satisfied, rep.truncated, rep.total_failing, rep.reported) == (want["satisfied"], want["truncated"], want["total_failing"], len(want["constraints"]))
    assert rep.chips == want["chips"]
    assert rep.constraints == want["constraints"]


def words(want):
    """The report's flat word image (include/vgpu.h) of audit()'s dict."""
    def u64(v):
        return [v & 0xffffffff, v >> 32]

    w = [0x31524356, 0, int(want["satisfied"]), int(want["truncated"])] + u64(want["total_failing"]) + [len(want["constraints"]), len(want["chips"])]
    for c in want["chips"]:
        w += [c["constraints"], c["failing_constraints"]] + u64(c["height"]) + u64(c["failing_rows"])
    for e in want["constraints"]:
        w += [e["chip"], e["constraint"]] + u64(e["failing_rows"]) + [len(e["rows"])]
        for row, value in e["rows"]:
            w += [row, value]
    w[1] = len(w)
    return np.array(w, dtype=np.uint32)
