"""The stage cases of tests/test_edge_values_gpu.py and their ORACLE halves: the same seeded inputs for the device run and for the CPU run of
the oracle alone (tests/test_field_edges_cpu.py, which shows before any GPU minute that no case makes the oracle invert zero — it aborts the
process there).  Inputs are canonical values chosen so that the device HOLDS the extreme stored words of tests/edge_corpus.py.
"""
import contextlib
import functools

import numpy as np

import edge_corpus as ec
import valida_amd as va
from oracle import pyoracle as po

P = ec.P
KECCAK, POSEIDON = 0, 1
MATRIX_KINDS = ["const_%08x" % w for w in ec.STAGE_WORDS] + ["alternating", "impulse_first", "impulse_last", "edge_mix"]
COLUMN_KINDS = ["const_%08x" % (P - 1), "const_77ffffff", "const_6fffffff", "edge_mix"]
CHIP_WIDTH = {2: 14, 3: 16, 10: 79}


def case_id(case):
    return "-".join("%s=%s" % (k, v) for k, v in case.items())


@contextlib.contextmanager
def oracle_mmcs(hash_kind, rc):
    po.set_mmcs_hash(1 if hash_kind == POSEIDON else 0, rc)
    try:
        yield
    finally:
        po.set_mmcs_hash(0)


def ext_all(word):
    """An Ext5 (canonical words) whose five stored words are `word`."""
    return [int(ec.from_words([word])[0])] * 5


def ext_from_edges(seed, n=1):
    """n Ext5 (canonical words) with every stored limb a NON-ZERO word of E (so no limb vanishes: a point is never in a two-adic domain)."""
    nz = np.array([w for w in ec.E if w], dtype=np.uint64)
    rng = np.random.default_rng([0xED70, seed])
    return [[int(v) for v in ec.from_words(nz[rng.integers(0, len(nz), 5)])] for _ in range(n)]


# ---- LDE and commit roots: heights 2^0, 2^4, 2^12 (one tile), 2^13 (the first four-step split), widths 1-3, both MMCS, blowups 2 and 4 ----------
LDE_CASES = [{"log_h": k, "mmcs": h, "log_blowup": b} for k in (0, 4, 12, 13) for h in (KECCAK, POSEIDON) for b in (1, 2)]


@functools.lru_cache(maxsize=None)
def lde_matrices(log_h):
    """kind -> [matrix of width 1, 2, 3], committed as one batch"""
    h = 1 << log_h
    per_w = [ec.stage_matrices(h, w, seed=7) for w in (1, 2, 3)]
    return {kind: [per_w[i][kind] for i in range(3)] for kind in MATRIX_KINDS}


def oracle_lde_commit(case, rc):
    """kind -> ([committed LDE per matrix], root)"""
    out = {}
    with oracle_mmcs(case["mmcs"], rc):
        for kind, mats in lde_matrices(case["log_h"]).items():
            out[kind] = ([po.committed_lde(m, case["log_blowup"], 31) for m in mats], po.commit_root(mats, log_blowup=case["log_blowup"]))
    for kind in MATRIX_KINDS[:4]:  # a constant column's LDE is constant
        for m, lde in zip(lde_matrices(case["log_h"])[kind], out[kind][0]):
            assert (lde == m[0, 0]).all()
    return out


# ---- permutation traces: chips 3 and 10 at 64 rows, chip 2 at 2^13 rows (the scan carries) ------------------------------------------------------
PERM_CASES = [{"chip": c, "rows": r, "main": m, "challenges": ch} for c, r in ((3, 64), (10, 64), (2, 1 << 13))
              for m in ["const_%08x" % w for w in ec.STAGE_WORDS] + ["edge_mix"] for ch in ("all_pm1", "edges")]


def perm_inputs(case):
    main = ec.stage_matrices(case["rows"], CHIP_WIDTH[case["chip"]], seed=11 + case["chip"])[case["main"]]
    if case["challenges"] == "all_pm1":
        ch = np.array(ext_all(P - 1) * 3, dtype=np.uint32)
    else:
        ch = np.array([w for e in ext_from_edges(23 + case["chip"], 3) for w in e], dtype=np.uint32)
    return main, ch


def oracle_perm_trace(case):
    main, ch = perm_inputs(case)
    return po.perm_trace(case["chip"], main, ch)


# ---- FRI fold ---------------------------------------------------------------------------------------------------------------------------------
FOLD_KINDS = ["const_%08x" % w for w in ec.STAGE_WORDS] + ["edge_mix"]
FOLD_CASES = [{"log_n": k, "f": f, "beta": b} for k in (2, 12) for f in FOLD_KINDS for b in FOLD_KINDS]


def fold_inputs(case):
    n = 1 << case["log_n"]
    f = ec.stage_matrices(n, 5, seed=31)[case["f"]]
    beta = ec.stage_matrices(1, 5, seed=37)[case["beta"]][0]
    return f, beta


def oracle_fri_fold(case):
    return po.fri_fold(*fold_inputs(case))


# ---- whole proofs: all fourteen traces corpus matrices at the smallest legal heights ----------------------------------------------------------
PROOF_KINDS = ["const_%08x" % w for w in ec.STAGE_WORDS] + ["edge_mix"]
PROOF_CASES = [{"traces": t, "mmcs": h, "log_blowup": b} for t in PROOF_KINDS for h in (KECCAK, POSEIDON) for b in (1, 2)]


@functools.lru_cache(maxsize=None)
def _fib25():
    w = va.Workload.fib(25)
    return [m.shape[1] for m in w.main_traces()], w.preprocessed()


def proof_inputs(case):
    """(main traces, preprocessed [(chip, matrix)]): program chip 32 rows and range chip 256 rows (the heights of fib(25)'s preprocessed traces), the
    others 16 or 64.  The traces satisfy no constraint; the proof is a function of them all the same."""
    widths, prep = _fib25()
    heights = [prep[0][1].shape[0] if c == prep[0][0] else prep[1][1].shape[0] if c == prep[1][0] else (16 if c % 2 == 0 else 64) for c in range(va.NUM_CHIPS)]
    assert heights[1] == 32 and heights[12] == 256
    return [ec.stage_matrices(h, w, seed=41 + c)[case["traces"]] for c, (h, w) in enumerate(zip(heights, widths))], prep


def oracle_proof(case, rc):
    mt, prep = proof_inputs(case)
    with oracle_mmcs(case["mmcs"], rc):
        return po.prove_basic(mt, prep[0][1], prep[1][1], rc, log_blowup=case["log_blowup"])


# ---- openings: the VALU column dots and Acc96 (64, 512 rows), the smallest heights of the matrix-core dots (1024, 2048), a ragged group of 16 ------
OPEN_CASES = [{"rows": r, "columns": c} for r in (64, 512, 1024, 2048) for c in COLUMN_KINDS]
OPEN_QUERIES, OPEN_POW_BITS = 9, 3


def open_inputs(case):
    """(rounds, points, observed): one round of a 3-column and a 17-column matrix, each opened at a point whose every stored limb is p - 1 and at
    points drawn from E."""
    rounds = [[ec.stage_matrices(case["rows"], w, seed=53)[case["columns"]] for w in (3, 17)]]
    a, (b, c) = ext_all(P - 1), ext_from_edges(59 + case["rows"], 2)
    points = [[[a, b], [a, c]]]
    observed = [int(v) for v in ec.from_words(ec.edge_words(61, 11))]
    return rounds, points, observed


def oracle_open(case, rc):
    rounds, points, observed = open_inputs(case)
    return po.pcs_open(rounds, points, rc, observed=observed, num_queries=OPEN_QUERIES, pow_bits=OPEN_POW_BITS)
