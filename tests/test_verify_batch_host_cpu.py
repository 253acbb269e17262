"""The host half of the batched verifier: the plan builder (host/verifier.hpp plan_multi_batches, machine_verifier.hpp plan_machine_proof)
is now what vgpu_verify runs before its per-query checks.  A hostile-shape corpus is rejected with the reason the host verifier has always
given, at the query where it meets it, and the committed CBOR proof still verifies."""
import os

import numpy as np
import pytest

import valida_amd as va
import verify_corpus as vc
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fib25_q3(rc, fib25):
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    return po.prove_basic(mt, prep[0][1], prep[1][1], rc, num_queries=3).words, va.host_commit_root([m for _, m in prep], rc)


def test_hostile_shapes_are_rejected_with_their_reasons(machine, rc, fib25_q3):
    words, pc = fib25_q3
    got = {label: va.verify(machine, rc, w, pc, num_queries=3) for label, w in vc.hostile(words)}
    assert all(g is not None and g.startswith("verify: ") for g in got.values()), got
    for label, g in got.items():
        if label.startswith("length field"):
            assert g in ("verify: length field exceeds the proof", "verify: wrong number of chip proofs"), (label, g)
    for q in (0, 1):
        assert got["in_path q%d one digest short" % q] == "verify: an input-round Merkle opening does not match its commitment"
        assert got["in_path q%d one digest long" % q] == "verify: an input-round Merkle opening does not match its commitment"
    for q in (0, 2):
        assert got["step_path q%d one digest short" % q] == "verify: a commit-phase Merkle opening does not match its commitment"
    assert got["row one column short at query 1"] == "verify: opened row has the wrong width"
    # query 0's tampered row is met first: the host order is query-major
    assert got["query 0 row tampered, query 1 row short"] == "verify: an input-round Merkle opening does not match its commitment"
    assert got["log_degree 27"] == got["log_degree 40"] == "verify: bad log_degree"
    assert got["log_degree 26"] == got["log_degree 4294967295"] == "verify: a matrix is taller than the first FRI layer"
    assert got["trace_local one value short"] == "verify: wrong number of opened values"
    assert got["rounds of query 0 + 1"] is not None
    assert got["empty"] == got["one word"] == "verify: proof words end early"
    assert va.verify(machine, rc, words, pc, num_queries=4) == "verify: wrong number of queries"
    assert va.verify(machine, rc, words, pc, num_queries=3) is None


def test_the_committed_cbor_proof_still_verifies(machine, rc):
    blob = open(os.path.join(ROOT, "tests", "golden", "fib25_q4_proof.cbor"), "rb").read()
    words = va.proof_from_cbor(blob)
    prep = va.Workload.fib(25).preprocessed()
    pc = va.host_commit_root([m for _, m in prep], rc)
    assert va.verify(machine, rc, words, pc, num_queries=4) is None
    bad = vc.mutate(words, words.size - 100)
    assert va.verify(machine, rc, bad, pc, num_queries=4) is not None
    assert np.array_equal(va.proof_from_cbor(blob), words)
