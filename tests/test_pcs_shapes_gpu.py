"""The GPU half of tests/pcs_corpus.py: vgpu_commit_batches + vgpu_open_multi_batches on every case of the corpus against the oracle's
pcs.commit_batches + open_multi_batches on the same matrices, points and transcript prefix (tests/test_pcs_shapes_cpu.py runs the oracle halves
without a GPU).  Exact equality everywhere; the assertions come in the order of the stages, so a failure names the first stage that differs."""
import hashlib
import json
import os

import numpy as np
import pytest

import pcs_corpus as pc
import valida_amd as va
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prover_for(machine, rc):
    """One prover context per (blowup, hash, queries, proof-of-work bits), shared by the module's cases"""
    made = {}

    def get(case):
        key = (case["log_blowup"], case["mmcs"], case["num_queries"], case["pow_bits"])
        if key not in made:
            made[key] = va.Prover(machine, rc, log_blowup=key[0], num_queries=key[2], pow_bits=key[3],
                                  hash_kind=va.HASH_POSEIDON16 if key[1] == pc.POSEIDON else va.HASH_KECCAK256)
        return made[key]
    yield get
    made.clear()


def _first(got, want):
    """None, or (position, got, want) of the first differing word; a differing length counts from the shorter one's end"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    n = min(got.size, want.size)
    d = np.nonzero(got[:n] != want[:n])[0]
    if d.size:
        return int(d[0]), int(got[d[0]]), int(want[d[0]])
    return None if got.size == want.size else (n, "%d words" % got.size, "%d words" % want.size)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_commit_and_open_match_the_oracle(prover_for, rc, case):
    p = prover_for(case)
    rounds, points, obs = pc.inputs(case)
    roots, values, proof = pc.oracle_open(case)
    # 1. the roots (and behind a wrong root: is it the LDE or the tree?)
    pds = [p.commit_batches([p.upload(m) for m in rnd]) for rnd in rounds]
    for r, pd in enumerate(pds):
        if _first(pd.root, roots[r]) is not None:
            for i, m in enumerate(rounds[r]):
                d = _first(pd.lde(i), po.committed_lde(m, case["log_blowup"], 31))
                assert d is None, "round %d: the LDE of matrix %d %s differs at word %d: %s vs %s" % ((r, i, m.shape) + d)
            pytest.fail("round %d: every LDE is the oracle's, the root is not: %s vs %s" % (r, list(pd.root), list(roots[r])))
    # 2. the opened values
    ch = va.Challenger(rc)
    ch.observe(obs)
    opened, words = p.open_multi_batches(pds, points, ch)
    got = np.concatenate([v.ravel() for rnd in opened for mat in rnd for v in mat])
    d = _first(got, values)
    assert d is None, "opened value (round, matrix, point, column, limb) = %s: %s vs %s" % (pc.value_index(case, min(d[0], values.size - 1)), d[1], d[2])
    # 3. the proof words
    d = _first(words, proof)
    assert d is None, "proof word %d (%s): %s vs %s" % (d[0], pc.proof_region(case, d[0]), d[1], d[2])
    # 4. the product's host verifier accepts the device's opening
    ch2 = va.Challenger(rc)
    ch2.observe(obs)
    heights, widths = pc.shapes(case)
    assert va.verify_multi_batches([pd.root for pd in pds], heights, widths, points, opened, words, ch2, rc, **pc.verify_kw(case)) is None
    # 5. opening and verifying left both transcripts in the same state
    assert np.array_equal(ch.sample(7), ch2.sample(7))


def test_257_queries_are_refused_and_the_device_proves_on(machine, rc, prover, fib25):
    case = pc.BY_NAME["queries_256_on_64_rows"]
    rounds, points, obs = pc.inputs(case)
    p = va.Prover(machine, rc, num_queries=pc.MAX_QUERIES + 1, pow_bits=case["pow_bits"])
    pds = [p.commit_batches([p.upload(m) for m in rnd]) for rnd in rounds]
    ch = va.Challenger(rc)
    ch.observe(obs)
    with pytest.raises(va.VgpuError, match="open: at most 256 queries"):
        p.open_multi_batches(pds, points, ch)
    # the refused prover still commits (a root does not depend on the number of queries) ...
    again = p.commit_batches([p.upload(m) for m in rounds[0]])
    assert _first(again.root, pc.oracle_open(case)[0][0]) is None
    del pds, again, p
    # ... and the device proves fib(25) to its golden bytes
    with open(os.path.join(os.path.dirname(__file__), "golden", "fib25_oracle.json")) as f:
        g = json.load(f)
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    proof = prover.prove([prover.upload(m) for m in mt], [(c, prover.upload(m)) for c, m in prep])
    assert hashlib.sha256(proof.bytes()).hexdigest() == g["proof_sha256"]
