"""Stage cases of tests/test_lazy_sums_gpu.py and their ORACLE halves (run without a GPU by tests/test_lazy_sums_cpu.py: the oracle aborts the
process on an inverse of zero, so a case that passes there has none).  The smallest shapes that take the paths whose sums are folded lazily:

openings     LDE heights 1024 and 2048 (the first that take k_reduce_openings_rows) and 512 (k_reduce_openings), one to three matrices per height,
             widths {1, 3, 4, 5, 6, 7, 8, 9, 13, 17, 23} — every mix of the rows kernel's 8- / 4- / 1-column steps, both parities of the folds —
             and one to four distinct points per height (four rows per thread up to two points, two rows above);
quotient,    all fourteen chips, one vgpu_quotient / vgpu_perm_trace_device call each.  k_quotient_pt is dispatched at every height, so the
permutation  heights are the smallest legal ones, the next ones, and 512 rows (the first heights whose launches are tiled, log_n >= 9).

Columns / traces: constant at the stored words p - 1 and 0x77FFFFFF (a constant column's LDE is constant: every LDE row holds the word) and the
edge mix of tests/edge_corpus.py.
"""
import functools

import numpy as np

import edge_corpus as ec
import edge_stage_cases as sc
import valida_amd as va
from oracle import pyoracle as po

P = ec.P
KINDS = ["const_%08x" % (P - 1), "const_77ffffff", "edge_mix"]
case_id = sc.case_id

# layout: [(trace rows, [(width, point names)])]; LDE height = 2 x rows.  Points: a = every stored limb p - 1; b, c, d drawn from the edge set.
OPEN_LAYOUTS = {
    "np4_np1_row2": [(1024, [(3, "ab"), (8, "ac"), (13, "bd")]), (512, [(1, "a")]), (256, [(4, "a"), (17, "ab")])],
    "np3_np2_row4": [(1024, [(23, "abc")]), (512, [(5, "ab"), (9, "ab")]), (256, [(7, "abcd")])],
    "np1_np3_row3": [(1024, [(4, "a"), (1, "a")]), (512, [(6, "a"), (7, "b"), (17, "c")]), (256, [(3, "a"), (8, "b"), (23, "c")])],
}
OPEN_CASES = [{"layout": lay, "columns": k} for lay in OPEN_LAYOUTS for k in KINDS]
OPEN_QUERIES, OPEN_POW_BITS = 9, 3


def open_inputs(case):
    """(rounds, points, observed): ONE round holding every matrix of the layout, tallest first."""
    pts = dict(zip("abcd", [sc.ext_all(P - 1)] + sc.ext_from_edges(71, 3)))
    mats, points = [], []
    for rows, group in OPEN_LAYOUTS[case["layout"]]:
        for i, (w, names) in enumerate(group):
            mats.append(ec.stage_matrices(rows, w, seed=73 + i)[case["columns"]])
            points.append([pts[nm] for nm in names])
    observed = [int(v) for v in ec.from_words(ec.edge_words(79, 11))]
    return [mats], [points], observed


@functools.lru_cache(maxsize=None)
def _oracle_open(layout, columns):
    rounds, points, observed = open_inputs({"layout": layout, "columns": columns})
    return po.pcs_open(rounds, points, _rc(), observed=observed, num_queries=OPEN_QUERIES, pow_bits=OPEN_POW_BITS)


def oracle_open(case):
    return _oracle_open(case["layout"], case["columns"])


# ---- quotient and permutation trace, chip by chip ------------------------------------------------------------------------------------------------
STAGE_TRACES = ["edge_mix", "const_%08x" % (P - 1)]
STAGE_ROWS = [16, 32, 512]  # of every chip without a preprocessed trace (those keep the heights of their preprocessed traces: 32 and 256)
CHIP_CASES = [{"rows": r, "traces": t} for r in STAGE_ROWS for t in STAGE_TRACES]


@functools.lru_cache(maxsize=None)
def _rc():
    return va.poseidon_round_constants()


@functools.lru_cache(maxsize=None)
def _fib25():
    w = va.Workload.fib(25)
    return [m.shape[1] for m in w.main_traces()], w.preprocessed()


def chip_inputs(case):
    """(main traces, preprocessed [(chip, matrix)]).  The traces satisfy no constraint; the quotient is a function of them all the same."""
    widths, prep = _fib25()
    pre = {c: m.shape[0] for c, m in prep}
    return [ec.stage_matrices(pre.get(c, case["rows"]), w, seed=83 + c)[case["traces"]] for c, w in enumerate(widths)], prep


@functools.lru_cache(maxsize=None)
def _oracle_chips(rows, traces):
    mt, prep = chip_inputs({"rows": rows, "traces": traces})
    return po.prove_basic(mt, prep[0][1], prep[1][1], _rc())


def oracle_chips(case):
    """The oracle's whole proof of the case: perm_trace(chip) and quotient(chip) are what the device's stage calls must return."""
    return _oracle_chips(case["rows"], case["traces"])


def bitrev_rows(n):
    k = n.bit_length() - 1
    return np.array([int(format(r, "0%db" % k)[::-1], 2) if k else 0 for r in range(n)])
