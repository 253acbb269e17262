"""Generated shapes for the polynomial commitment stage (vgpu_commit_batches + vgpu_open_multi_batches) at every edge of its dispatch, and their
ORACLE halves.  tests/test_pcs_shapes_cpu.py runs the oracle and the product's host verifier on every case without a GPU (the oracle aborts the
process on an inverse of zero, so a case that passes there has none); tests/test_pcs_shapes_gpu.py runs the device on the same inputs.

A case is a dict:
    name        carries the edge the case is there for
    rounds      [[(rows, width) or (rows, width, kind)]] in commit order; kind names a matrix of edge_corpus.stage_matrices, no kind = uniform words
    points      points[r][i] = a string of names into POINTS, one letter per opening point of matrix i of round r
    log_blowup  1, 2 or 3
    mmcs        KECCAK or POSEIDON
    num_queries, pow_bits, prefix (number of words observed before the opening), seed

signature(case) is the set of dispatch edges the case reaches, computed from the constants below — copies of the source's, which
test_pcs_shapes_cpu.py reads back from the source and compares, so a moved threshold fails there and names this file.  REQUIRED_EDGES is the table
of edges the designed cases must reach between them (DESIGN.md §3e holds the same table with the case that reaches each).
"""
import functools

import numpy as np

import edge_corpus as ec
import edge_stage_cases as sc
import valida_amd as va
from oracle import pyoracle as po

P = ec.P
KECCAK, POSEIDON = sc.KECCAK, sc.POSEIDON
MMCS_NAME = {KECCAK: "keccak", POSEIDON: "poseidon"}

# ---- the source's constants (valida_amd/csrc: kernels/open.hip, kernels/launch.hpp, kernels/poseidon_mmcs.hip, host/pcs.hpp, host/prover.cpp) ---------
MFMA_DOT_MIN_ROWS = 1024          # trace rows from which the opened values are computed on the matrix cores (k_col_dot_mfma), below: k_col_dot
DOT_TR = 128                      # rows per tile of k_col_dot
DOT_MAX_PASSES, DOT_THREADS = 4, 256   # k_col_dot: at most DOT_MAX_PASSES * DOT_THREADS output limbs per launch = 5 * points * columns
MAX_OPEN_POINTS_PER_LAUNCH = 4    # distinct points per reduced-openings launch; later chunks accumulate
REDUCE_ROWS_MIN_LDE = 1024        # LDE height from which launch_reduce_openings takes k_reduce_openings_rows
DROP_MIN_LEAVES = 1 << 16         # trees of that many leaves do not keep their bottom layers
TOP_FIRST_LEN = 256               # Keccak tree layers of more parents are launches of their own
POSEIDON_ROW_MAX = 16384          # Poseidon tree layers of at most that many parents are multi-layer launches
MAX_QUERIES = 256                 # open: at most 256 queries (the query number is a byte of a gather descriptor)
DOT_POINTS_PER_LAUNCH = 2
VALU_HEIGHTS = (1, 2, 128, 256, 512)


def col_dot_max_columns(np_):
    return DOT_MAX_PASSES * DOT_THREADS // (5 * np_)


assert (col_dot_max_columns(1), col_dot_max_columns(2)) == (204, 102)

# The cap on a case's work = the sum over its matrices of rows x width x points, which the oracle's barycentric sums and LDEs grow with.  Measured
# on a build machine: the largest case here (1.26 M, Keccak) takes 0.06 s; what costs most is the Poseidon tree over an LDE of 2^16 rows, 0.45 s
# whatever the widths — and no case is taller than that (rows <= 2^14 by design, <= 2^11 in the draws).  Below the cap an oracle half stays far under 2 s.
WORK_CAP = 1 << 21

# ---- the point table -------------------------------------------------------------------------------------------------------------------------------
BASE_POINT = 1234567


def _point_table():
    rng = np.random.default_rng([0x9C5, 1])
    t = {"a": sc.ext_all(P - 1)}                                    # every stored limb p - 1
    t["b"], t["c"] = sc.ext_from_edges(97, 2)                       # stored limbs drawn from the edge set
    t["f"] = [BASE_POINT, 0, 0, 0, 0]                               # in the base field: its minimal polynomial is (X - z)^5
    for nm in "uvwxyzst":
        t[nm] = [int(x) for x in rng.integers(1, P, 5)]
    return t


POINTS = _point_table()
assert len({tuple(z) for z in POINTS.values()}) == len(POINTS)
# f / 31 has no power-of-two order: f lies in no coset 31 H of a two-adic subgroup H (p - 1 = 2^27 * 15), whatever the height
assert pow(BASE_POINT * pow(31, P - 2, P) % P, 1 << 27, P) != 1


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
def _case(name, rounds, points, log_blowup=1, mmcs=KECCAK, num_queries=5, pow_bits=3, prefix=11, seed=0):
    assert len(rounds) == len(points) and all(len(r) == len(p) for r, p in zip(rounds, points)), name
    assert all(set(s) <= set(POINTS) and s for p in points for s in p), name
    return {"name": name, "rounds": rounds, "points": points, "log_blowup": log_blowup, "mmcs": mmcs, "num_queries": num_queries, "pow_bits": pow_bits,
            "prefix": prefix, "seed": seed}


def _designed():
    out = []
    add = lambda *a, **k: out.append(_case(*a, seed=len(out) + 1, **k))
    # -- opened values
    add("dot_valu_rows_1_2_128_256_512", [[(512, 3), (256, 2), (128, 4), (2, 3), (1, 5)]], [["ab", "ab", "u", "ub", "a"]])
    add("dot_mfma_rows_1024_2048_8192_widths_1_15_16_17_33_points_1_2_3_5",
        [[(8192, 1), (2048, 15), (2048, 16), (1024, 17), (1024, 33)]], [["a", "ub", "u", "abu", "abcuv"]])
    for rows, kern in ((64, "valu"), (1024, "mfma")):
        add("dot_%s_chunks_one_point_widths_204_205_409_two_points_102_103" % kern,
            [[(rows, 204), (rows, 205), (rows, 409)], [(rows, 102), (rows, 103)]], [["u", "a", "b"], ["uv", "ab"]])
    add("dot_valu_point_lists_of_1_2_3_5", [[(64, 3), (64, 4), (32, 2), (32, 6)]], [["u", "uv", "abc", "abcuv"]])
    add("points_shared_by_two_heights_and_two_rounds_and_repeated_on_one_matrix", [[(64, 3), (32, 2)], [(64, 4)]], [["u", "uvv"], ["ua"]])
    add("point_in_the_base_field", [[(16, 3), (8, 2)], [(1024, 2)]], [["f", "fu"], ["f"]])
    # -- reduced openings
    add("reduce_row_kernel_distinct_points_1_2_3_4_5_8_9",
        [[(256, 2), (128, 3), (64, 1), (32, 2), (16, 3), (16, 1), (8, 2), (8, 3), (8, 1), (4, 1), (4, 2), (4, 3)]],
        [["u", "uv", "abc", "abcu", "abcu", "av", "abcu", "avwx", "ay", "abcu", "avwx", "ayz"]])  # (every matrix is live in the first chunk)
    add("reduce_rows_kernel_distinct_points_1_2_3_4", [[(4096, 2), (2048, 3), (1024, 2), (512, 3)]], [["abcu", "abc", "uv", "u"]])
    add("reduce_rows_kernel_distinct_points_5_6_7_8_9_accumulating",
        [[(8192, 1), (8192, 2), (4096, 1), (4096, 2), (2048, 2), (2048, 1), (2048, 3), (1024, 2), (1024, 3), (1024, 1), (512, 2), (512, 1)]],
        [["abcu", "avwx", "abcu", "avw", "abcu", "avwx", "ayz", "abcu", "avwx", "ay", "abcu", "av"]])
    add("reduce_matrix_whose_only_point_falls_in_the_second_chunk", [[(1024, 3), (1024, 2), (16, 3), (16, 2)]], [["abcu", "v", "abcu", "v"]])
    for lb, (lo, hi) in ((1, (256, 512)), (2, (128, 256)), (3, (64, 128))):
        add("reduce_lde_heights_512_1024_at_blowup_%d_rows_%d_%d" % (1 << lb, lo, hi),
            [[(hi, 9, "edge_mix"), (hi, 3), (lo, 5, "const_%08x" % (P - 1)), (lo, 4)]], [["ab", "ab", "au", "u"]], log_blowup=lb)
    add("reduce_three_matrices_of_one_height_over_two_rounds", [[(64, 3), (64, 4)], [(64, 2), (16, 1)]], [["u", "uv"], ["v", "a"]])
    # -- FRI and queries
    for lb in (1, 2, 3):
        add("fri_every_matrix_one_row_at_blowup_%d" % (1 << lb), [[(1, 3), (1, 1)], [(1, 4), (1, 2)]], [["u", "ab"], ["u", "v"]], log_blowup=lb)
    add("fri_heights_1_and_2_only", [[(2, 3), (1, 2)], [(2, 1)]], [["ab", "u"], ["b"]])
    add("fri_only_the_tallest_height_and_height_1", [[(1024, 2), (1, 3)]], [["u", "uv"]])
    add("fri_every_height_from_1_to_1024", [[(1024 >> k, 1 + k % 3) for k in range(11)]], [["u" if k % 2 else "ab" for k in range(11)]])
    add("queries_1_on_64_rows_pow_bits_0", [[(64, 3), (16, 2)]], [["ab", "u"]], num_queries=1, pow_bits=0)
    add("queries_256_on_64_rows", [[(64, 3), (16, 2)]], [["ab", "u"]], num_queries=256)
    add("pow_bits_10", [[(64, 3), (16, 2)]], [["ab", "u"]], pow_bits=10)
    for n in (0, 7, 8, 9):
        add("observed_prefix_of_%d_words" % n, [[(16, 2), (4, 3)]], [["u", "ab"]], prefix=n)
    # -- MMCS
    add("mmcs_round_in_ascending_height_order", [[(4, 2), (16, 3), (64, 1), (256, 2)]], [["u", "ab", "u", "v"]])
    add("mmcs_round_in_shuffled_height_order", [[(16, 3), (256, 2), (4, 2), (64, 1)]], [["ab", "v", "u", "u"]])
    add("mmcs_equally_tall_matrices_of_widths_3_then_5", [[(32, 3), (32, 5)]], [["u", "uv"]])
    add("mmcs_equally_tall_matrices_of_widths_5_then_3", [[(32, 5), (32, 3)]], [["uv", "u"]])
    add("mmcs_round_of_40_one_column_matrices", [[(32, 1)] * 40], [["u"] * 39 + ["ab"]])
    for mmcs in (KECCAK, POSEIDON):
        add("drop_bottom_layers_2^14_rows_blowup_4_injected_one_layer_up_%s" % MMCS_NAME[mmcs], [[(1 << 14, 2), (1 << 13, 3)]], [["u", "v"]], log_blowup=2, mmcs=mmcs)
        add("drop_bottom_layers_2^13_rows_blowup_8_injected_one_layer_up_%s" % MMCS_NAME[mmcs], [[(1 << 13, 2), (1 << 12, 3)]], [["u", "v"]], log_blowup=3, mmcs=mmcs)
    add("poseidon_rows_16_64_1024_widths_7_8_9_17", [[(rows, w) for w in (7, 8, 9, 17)] for rows in (16, 64, 1024)], [["u", "ab", "v", "uv"]] * 3, mmcs=POSEIDON)
    return out


DRAW_SEED = 0x9C5D
DRAW_WIDTHS = list(range(1, 10)) + [16, 17, 33, 103, 205]


def _draws():
    rng = np.random.default_rng(DRAW_SEED)
    names = sorted(POINTS)
    out = []
    while len(out) < 24:
        rounds = [[(1 << int(rng.integers(0, 12)), int(rng.choice(DRAW_WIDTHS))) for _ in range(int(rng.integers(1, 6)))] for _ in range(int(rng.integers(1, 4)))]
        points = [["".join(rng.choice(names, int(rng.integers(1, 6)))) for _ in rnd] for rnd in rounds]
        cfg = dict(log_blowup=int(rng.integers(1, 4)), mmcs=int(rng.choice([KECCAK, POSEIDON])), num_queries=int(rng.choice([1, 5, 9])), pow_bits=int(rng.choice([0, 3])))
        c = _case("draw_%02d" % len(out), rounds, points, prefix=int(rng.integers(0, 12)), seed=1000 + len(out), **cfg)
        if work(c) <= WORK_CAP:  # (a draw above the cap is drawn again: the sequence stays a function of DRAW_SEED alone)
            out.append(c)
    return out


def work(case):
    return sum(m[0] * m[1] * len(s) for rnd, pts in zip(case["rounds"], case["points"]) for m, s in zip(rnd, pts))


DESIGNED = _designed()
DRAWS = _draws()
CASES = DESIGNED + DRAWS
assert len({c["name"] for c in CASES}) == len(CASES) and all(work(c) <= WORK_CAP for c in CASES)


def case_id(case):
    return case["name"]


# ---- inputs and oracle half ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rc():
    return va.poseidon_round_constants()


def inputs(case):
    """(rounds of canonical matrices, points[r][i] = [Ext5], observed prefix)"""
    rng = np.random.default_rng([0x9C5, 2, case["seed"]])
    rounds = []
    for rnd in case["rounds"]:
        mats = []
        for m in rnd:
            uniform = rng.integers(0, P, (m[0], m[1]), dtype=np.uint32)  # drawn whether used or not: a kind does not shift the other matrices
            mats.append(ec.stage_matrices(m[0], m[1], seed=case["seed"])[m[2]] if len(m) > 2 else uniform)
        rounds.append(mats)
    points = [[[POINTS[nm] for nm in s] for s in rnd] for rnd in case["points"]]
    observed = [int(x) for x in rng.integers(0, P, case["prefix"])]
    return rounds, points, observed


@functools.lru_cache(maxsize=None)
def _oracle(name):
    case = BY_NAME[name]
    rounds, points, observed = inputs(case)
    with sc.oracle_mmcs(case["mmcs"], _rc()):
        return po.pcs_open(rounds, points, _rc(), observed=observed, log_blowup=case["log_blowup"], num_queries=case["num_queries"], pow_bits=case["pow_bits"])


BY_NAME = {c["name"]: c for c in CASES}


def oracle_open(case):
    """(roots, opened values flat, proof words) of the oracle; computed once per process and shared — do not modify"""
    return _oracle(case["name"])


def verify_kw(case):
    return dict(log_blowup=case["log_blowup"], num_queries=case["num_queries"], pow_bits=case["pow_bits"],
                hash_kind=va.HASH_POSEIDON16 if case["mmcs"] == POSEIDON else va.HASH_KECCAK256)


def shapes(case):
    return [[m[0] for m in rnd] for rnd in case["rounds"]], [[m[1] for m in rnd] for rnd in case["rounds"]]


# ---- where a word of the opened values / of the proof lies -------------------------------------------------------------------------------------------
def value_index(case, pos):
    """(round, matrix, point, column, limb) of word `pos` of the flat opened values"""
    for r, (rnd, pts) in enumerate(zip(case["rounds"], case["points"])):
        for i, (m, s) in enumerate(zip(rnd, pts)):
            for p in range(len(s)):
                if pos < 5 * m[1]:
                    return (r, i, p, pos // 5, pos % 5)
                pos -= 5 * m[1]
    raise IndexError(pos)


def log_max_lde(case):
    return max(m[0] for rnd in case["rounds"] for m in rnd).bit_length() - 1 + case["log_blowup"]


def proof_regions(case):
    """[(name, first word, end word)] of the TwoAdicFriPcsProof words: [n_layers][roots][n_queries][per query: n_layers, per layer: sibling value (5),
    path length, path] [final polynomial (5)] [witness] [n_queries][per query: n_rounds, per round: n_matrices, per matrix: width, row; path length, path]"""
    nl, nq, lm = log_max_lde(case) - case["log_blowup"], case["num_queries"], log_max_lde(case)
    per_query = 1 + sum(5 + 1 + 8 * (lm - 1 - l) for l in range(nl))
    per_query_in = 1 + sum(1 + sum(1 + m[1] for m in rnd) + 1 + 8 * (max(m[0] for m in rnd).bit_length() - 1 + case["log_blowup"]) for rnd in case["rounds"])
    edges = [("commit-phase roots", 1 + 8 * nl), ("commit-phase answers", 1 + nq * per_query), ("final polynomial", 5), ("proof-of-work witness", 1),
             ("input openings", 1 + nq * per_query_in)]
    out, at = [], 0
    for name, n in edges:
        out.append((name, at, at + n))
        at += n
    return out


def proof_region(case, pos):
    for name, a, b in proof_regions(case):
        if a <= pos < b:
            return name
    return "beyond the proof"


# ---- the signature ------------------------------------------------------------------------------------------------------------------------------------
def signature(case):
    """The set of dispatch edges `case` reaches (tuples of words and numbers)"""
    lb, hsh = case["log_blowup"], MMCS_NAME[case["mmcs"]]
    sig = set()
    groups = {}  # LDE height -> (distinct point names in first-seen order, [(set of slots of a matrix)])
    seen_at = {}
    for r, (rnd, pts) in enumerate(zip(case["rounds"], case["points"])):
        for i, (m, s) in enumerate(zip(rnd, pts)):
            n, w = m[0], m[1]
            kern = "mfma" if n >= MFMA_DOT_MIN_ROWS else "valu"
            sig.add(("dot", kern, "rows", n) if n in (1, 2, 128, 256, 512, 1024, 2048, 8192) else ("dot", kern))
            if kern == "valu" and n > DOT_TR:
                sig.add(("dot", "valu", "more than one tile"))
            if kern == "mfma":
                sig.add(("dot", "mfma", "width mod 16", w % 16) if w % 16 in (0, 1, 15) else ("dot", "mfma", "width mod 16", "other"))
            sig.add(("point list", kern, len(s)))
            if len(set(s)) < len(s):
                sig.add(("point repeated on one matrix",))
            for p0 in range(0, len(s), DOT_POINTS_PER_LAUNCH):
                np_ = min(DOT_POINTS_PER_LAUNCH, len(s) - p0)
                cap = col_dot_max_columns(np_)
                chunks = -(-w // cap)
                sig.add(("dot", kern, "points", np_, "chunked" if chunks > 1 else "whole"))
                if w % cap == 0:
                    sig.add(("dot", kern, "points", np_, "chunk ends on the limit"))
                if chunks > 1 and w % cap == 1:
                    sig.add(("dot", kern, "points", np_, "last chunk one column"))
                sig.add(("open_y segments", min(chunks, 3)))
            zs, mats = groups.setdefault(n << lb, ([], []))
            slots = set()
            for nm in s:
                if nm not in zs:
                    zs.append(nm)
                slots.add(zs.index(nm))
                if nm == "f":
                    sig.add(("point in the base field",))
                for (r2, n2) in seen_at.get(nm, ()):
                    if n2 != n:
                        sig.add(("point shared by two heights",))
                    if r2 != r:
                        sig.add(("point shared by two rounds",))
                seen_at.setdefault(nm, set()).add((r, n))
            mats.append((r, slots))
            if len(m) > 2:
                sig.add(("reduce", "rows" if (n << lb) >= REDUCE_ROWS_MIN_LDE else "row", "blowup", 1 << lb, "columns", m[2]))
    for L, (zs, mats) in groups.items():
        d = len(zs)
        sig.add(("distinct points on one height", "rows" if L >= REDUCE_ROWS_MIN_LDE else "row", d))
        if len({r for r, _ in mats}) > 1 and len(mats) == 3:
            sig.add(("three matrices of one height over two rounds",))
        rows_kernel = L >= REDUCE_ROWS_MIN_LDE
        for s0 in range(0, d, MAX_OPEN_POINTS_PER_LAUNCH):
            np_ = min(MAX_OPEN_POINTS_PER_LAUNCH, d - s0)
            acc = "accumulate" if s0 else "first"
            sig.add(("reduce", "rows", "NP", np_, "R", 4 if np_ <= 2 else 2, acc) if rows_kernel else ("reduce", "row", acc))
            if s0 and any(min(sl) >= s0 for _, sl in mats):
                sig.add(("reduce", "rows" if rows_kernel else "row", "matrix live only in a later chunk"))
        if rows_kernel and (L >> lb) < MFMA_DOT_MIN_ROWS:
            sig.add(("reduce", "rows", "values from the VALU dot kernel", "blowup", 1 << lb))
    heights = sorted({m[0] for rnd in case["rounds"] for m in rnd})
    if tuple(heights) == VALU_HEIGHTS:
        sig.add(("dot", "valu", "exactly the rows 1, 2, 128, 256 and 512 in one opening"))
    lm = log_max_lde(case)
    if lm == lb:
        sig.add(("fri", "no layer", "blowup", 1 << lb))
    if heights == [1, 2]:
        sig.add(("fri", "heights 1 and 2 only"))
    if len(heights) == 2 and heights[0] == 1 and heights[1] >= 1024:
        sig.add(("fri", "only the tallest height and height 1"))
    if heights == [1 << k for k in range(11)]:
        sig.add(("fri", "every height from 1 to 1024"))
    if (1 << lm) // 2 >= DROP_MIN_LEAVES:
        sig.add(("fri", "layer tree drops its bottom", hsh))
    if case["num_queries"] in (1, MAX_QUERIES):
        sig.add(("queries", case["num_queries"]))
    if case["pow_bits"] in (0, 10):
        sig.add(("pow_bits", case["pow_bits"]))
    if case["prefix"] in (0, 7, 8, 9):
        sig.add(("observed prefix", case["prefix"]))
    for rnd in case["rounds"]:
        hs = [m[0] for m in rnd]
        maxh = max(hs) << lb
        if hs == sorted(hs) and len(set(hs)) > 2:
            sig.add(("mmcs", "round in ascending height order"))
        if hs != sorted(hs) and hs != sorted(hs, reverse=True):
            sig.add(("mmcs", "round in shuffled height order"))
        for a, b in zip(rnd, rnd[1:]):
            if a[0] == b[0] and {a[1], b[1]} == {3, 5}:
                sig.add(("mmcs", "equally tall matrices of widths", a[1], b[1]))
        if len(rnd) >= 40 and len(set(hs)) == 1:
            sig.add(("mmcs", "40 one-column matrices of one height"))
        parents = maxh // 2
        if case["mmcs"] == KECCAK:
            sig.add(("mmcs", hsh, "parents <= TOP_FIRST_LEN" if parents <= TOP_FIRST_LEN else "parents > TOP_FIRST_LEN"))
        else:
            sig.add(("mmcs", hsh, "parents <= POSEIDON_ROW_MAX" if parents <= POSEIDON_ROW_MAX else "parents > POSEIDON_ROW_MAX"))
            for m in rnd:
                if m[0] in (16, 64, 1024) and m[1] in (7, 8, 9, 17):
                    sig.add(("mmcs", hsh, "rows", m[0], "width", m[1]))
        if maxh >= DROP_MIN_LEAVES:
            injected = any((m[0] << lb) * 2 == maxh for m in rnd)
            sig.add(("mmcs", hsh, "bottom layers dropped", "blowup", 1 << lb, "injection one layer up" if injected else "no injection there"))
    return sig


def _required():
    e = set()
    for n in (1, 2, 128, 256, 512):
        e.add(("dot", "valu", "rows", n))
    for n in (1024, 2048, 8192):
        e.add(("dot", "mfma", "rows", n))
    e.add(("dot", "valu", "more than one tile"))
    e.add(("dot", "valu", "exactly the rows 1, 2, 128, 256 and 512 in one opening"))
    for r in (0, 1, 15, "other"):
        e.add(("dot", "mfma", "width mod 16", r))
    for kern in ("valu", "mfma"):
        for np_ in (1, 2):
            for how in ("whole", "chunked", "chunk ends on the limit", "last chunk one column"):
                e.add(("dot", kern, "points", np_, how))
    for n in (1, 2, 3):
        e.add(("open_y segments", n))
    for n in (1, 2, 3, 5):
        e |= {("point list", "valu", n), ("point list", "mfma", n)}
    e |= {("point repeated on one matrix",), ("point in the base field",), ("point shared by two heights",), ("point shared by two rounds",),
          ("three matrices of one height over two rounds",)}
    for d in (1, 2, 3, 4, 5, 8, 9):
        e |= {("distinct points on one height", "row", d), ("distinct points on one height", "rows", d)}
    for acc in ("first", "accumulate"):
        e.add(("reduce", "row", acc))
        for np_ in (1, 2, 3, 4):
            e.add(("reduce", "rows", "NP", np_, "R", 4 if np_ <= 2 else 2, acc))
    for k in ("row", "rows"):
        e.add(("reduce", k, "matrix live only in a later chunk"))
    for b in (2, 4, 8):
        e |= {("reduce", "rows", "blowup", b, "columns", "edge_mix"), ("reduce", "row", "blowup", b, "columns", "const_%08x" % (P - 1))}
        e.add(("fri", "no layer", "blowup", b))
    for b in (4, 8):
        e.add(("reduce", "rows", "values from the VALU dot kernel", "blowup", b))
    e |= {("fri", "heights 1 and 2 only"), ("fri", "only the tallest height and height 1"), ("fri", "every height from 1 to 1024")}
    e |= {("queries", 1), ("queries", MAX_QUERIES), ("pow_bits", 0), ("pow_bits", 10)}
    for n in (0, 7, 8, 9):
        e.add(("observed prefix", n))
    e |= {("mmcs", "round in ascending height order"), ("mmcs", "round in shuffled height order"), ("mmcs", "equally tall matrices of widths", 3, 5),
          ("mmcs", "equally tall matrices of widths", 5, 3), ("mmcs", "40 one-column matrices of one height")}
    e |= {("mmcs", "keccak", "parents <= TOP_FIRST_LEN"), ("mmcs", "keccak", "parents > TOP_FIRST_LEN"),
          ("mmcs", "poseidon", "parents <= POSEIDON_ROW_MAX"), ("mmcs", "poseidon", "parents > POSEIDON_ROW_MAX")}
    for rows in (16, 64, 1024):
        for w in (7, 8, 9, 17):
            e.add(("mmcs", "poseidon", "rows", rows, "width", w))
    for hsh in ("keccak", "poseidon"):
        for b in (4, 8):
            e.add(("mmcs", hsh, "bottom layers dropped", "blowup", b, "injection one layer up"))
    return e


REQUIRED_EDGES = _required()
