"""The CPU half of tests/pcs_corpus.py: the constants the corpus' signature is computed from are the source's, the designed cases reach every edge
of the table, and every case goes through the oracle (which aborts on an inverse of zero: a case that passes here has none) and through the
product's HOST verifier, which must accept the oracle's opening and reject it with one opened value or one proof word changed."""
import os
import re

import numpy as np
import pytest

import pcs_corpus as pc
import valida_amd as va

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "valida_amd", "csrc")


def _src(rel):
    with open(os.path.join(CSRC, rel)) as f:
        return f.read()


def _int(text):
    m = re.fullmatch(r"\s*(\d+)(?:ull)?\s*(?:<<\s*(\d+))?\s*", text)
    assert m, text
    return int(m.group(1)) << int(m.group(2) or 0)


def _constant(rel, name):
    hits = re.findall(r"\b%s\s*=\s*([^,;]+)[,;]" % name, _src(rel))
    assert len(hits) == 1, "%s: %d definitions of %s (tests/pcs_corpus.py assumes one)" % (rel, len(hits), name)
    return _int(hits[0])


@pytest.mark.parametrize("rel,name", [("kernels/open.hip", "MFMA_DOT_MIN_ROWS"), ("kernels/open.hip", "DOT_TR"), ("kernels/open.hip", "DOT_MAX_PASSES"),
                                      ("kernels/open.hip", "DOT_THREADS"), ("kernels/launch.hpp", "MAX_OPEN_POINTS_PER_LAUNCH"), ("host/pcs.hpp", "DROP_MIN_LEAVES"),
                                      ("host/pcs.hpp", "TOP_FIRST_LEN"), ("kernels/poseidon_mmcs.hip", "POSEIDON_ROW_MAX")])
def test_the_corpus_assumes_the_sources_constants(rel, name):
    assert _constant(rel, name) == getattr(pc, name), "%s in %s moved: tests/pcs_corpus.py (signature, REQUIRED_EDGES and the designed cases) must follow" % (name, rel)


def test_the_corpus_assumes_the_sources_dispatch_conditions():
    where = "tests/pcs_corpus.py must follow"
    op, pr = _src("kernels/open.hip"), _src("host/prover.cpp")
    m = re.search(r"uint64_t col_dot_max_columns\(int np\) \{ return \(uint64_t\)DOT_MAX_PASSES \* DOT_THREADS / \(5 \* \(uint64_t\)np\); \}", op)
    assert m, "col_dot_max_columns changed: " + where
    m = re.search(r"const bool rows_kernel_ok = vec_ok && L >= (\d+) &&", op)
    assert m and int(m.group(1)) == pc.REDUCE_ROWS_MIN_LDE, "the height condition of launch_reduce_openings moved: " + where
    m = re.search(r"const int R = rows_env == 2 \|\| rows_env == 4 \? rows_env : \(np <= 2 \? 4 : 2\);", op)
    assert m, "the rows per thread of launch_reduce_openings changed: " + where
    m = re.search(r"if \(n >= MFMA_DOT_MIN_ROWS\) \{  // matrix cores", op)
    assert m, "the kernel choice of launch_col_dot changed: " + where
    m = re.search(r'if \(NQ > (\d+)\) throw std::invalid_argument\("open: at most (\d+) queries"\);', pr)
    assert m and int(m.group(1)) == int(m.group(2)) == pc.MAX_QUERIES, "the query limit of open_multi_batches moved: " + where
    m = re.search(r"for \(size_t p0 = 0; p0 < pts\.size\(\); p0 \+= (\d+)\) \{\s*const int np = \(int\)std::min<size_t>\((\d+), pts\.size\(\) - p0\);", pr)
    assert m and int(m.group(1)) == int(m.group(2)) == pc.DOT_POINTS_PER_LAUNCH, "the points per column-dot launch changed: " + where
    m = re.search(r"maxh >= DROP_MIN_LEAVES && layers\.size\(\) >= 4", _src("host/pcs.hpp"))
    assert m, "the condition of DeviceTree::drop_bottom changed: " + where
    # the LDE coset and the field of the base-field point's membership test
    assert va.P == pc.P == 2 ** 31 - 2 ** 27 + 1


def test_the_designed_cases_reach_every_edge_of_the_table():
    reached = set().union(*[pc.signature(c) for c in pc.DESIGNED])
    missing = pc.REQUIRED_EDGES - reached
    assert not missing, "edges no designed case reaches: %s" % sorted(map(str, missing))


@pytest.mark.parametrize("case", pc.DESIGNED, ids=pc.case_id)
def test_every_designed_case_is_the_only_one_to_reach_some_edge(case):
    """so that removing a designed case makes the coverage test above fail and name an edge: no case is there for nothing"""
    others = set().union(*[pc.signature(c) for c in pc.DESIGNED if c is not case])
    assert (pc.signature(case) & pc.REQUIRED_EDGES) - others, "every edge of %s is reached by another designed case as well" % case["name"]


def test_the_draws_are_what_the_issue_asks_for():
    assert len(pc.DRAWS) == 24
    for c in pc.DRAWS:
        assert 1 <= len(c["rounds"]) <= 3 and all(1 <= len(rnd) <= 5 for rnd in c["rounds"])
        assert all(m[0] in [1 << k for k in range(12)] and m[1] in pc.DRAW_WIDTHS for rnd in c["rounds"] for m in rnd)
        assert all(1 <= len(s) <= 5 for rnd in c["points"] for s in rnd)
        assert c["log_blowup"] in (1, 2, 3) and c["num_queries"] in (1, 5, 9) and c["pow_bits"] in (0, 3) and pc.work(c) <= pc.WORK_CAP
    assert {c["log_blowup"] for c in pc.DRAWS} == {1, 2, 3} and {c["mmcs"] for c in pc.DRAWS} == {pc.KECCAK, pc.POSEIDON}


def test_the_base_field_point_lies_on_no_committed_coset():
    z, heights = pc.POINTS["f"], {m[0] << c["log_blowup"] for c in pc.CASES for rnd in c["rounds"] for m in rnd}
    assert z[1:] == [0, 0, 0, 0]
    for L in sorted(heights):  # z in 31 H_L  <=>  (z / 31)^L = 1
        assert pow(z[0] * pow(31, pc.P - 2, pc.P) % pc.P, L, pc.P) != 1, L


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_oracle_opening_is_accepted_by_the_host_verifier_and_tampering_is_not(rc, case):
    roots, values, proof = pc.oracle_open(case)
    rounds, points, obs = pc.inputs(case)
    heights, widths = pc.shapes(case)
    assert roots.shape == (len(rounds), 8) and values.size == sum(5 * m[1] * len(s) for rnd, pts in zip(case["rounds"], case["points"]) for m, s in zip(rnd, pts))
    regions = pc.proof_regions(case)
    assert regions[-1][2] == proof.size, "pcs_corpus.proof_regions does not describe the proof's layout"
    assert proof[0] == pc.log_max_lde(case) - case["log_blowup"] and proof[regions[1][1]] == proof[regions[4][1]] == case["num_queries"]

    def verify(values, proof):
        ch = va.Challenger(rc)
        ch.observe(obs)
        return va.verify_multi_batches(list(roots), heights, widths, points, values, proof, ch, rc, **pc.verify_kw(case))

    assert verify(values, proof) is None
    rng = np.random.default_rng([0x9C5, 3, case["seed"]])
    pos = int(rng.integers(0, values.size))
    bad = values.copy()
    bad[pos] = (int(bad[pos]) + 1) % pc.P
    assert verify(bad, proof) is not None, "accepted with opened value %s changed" % (pc.value_index(case, pos),)
    # one proof word, anywhere but the proof-of-work witness: with few bits to grind a changed witness is as good as the prover's (and every
    # other word is bound: lengths by the parser, digests and rows by the Merkle paths, the final polynomial by the fold)
    wit = regions[3][1]
    pos = int(rng.integers(0, proof.size - 1))
    pos += pos >= wit
    bad = proof.copy()
    bad[pos] = (int(bad[pos]) + 1) % pc.P
    assert verify(values, bad) is not None, "accepted with proof word %d (%s) changed" % (pos, pc.proof_region(case, pos))


def test_the_corpus_holds_the_query_limit_and_nothing_above():
    """the limit itself is a case (queries_256_on_64_rows); 257 is refused (tests/test_pcs_shapes_gpu.py pins the message)"""
    assert max(c["num_queries"] for c in pc.CASES) == pc.MAX_QUERIES
