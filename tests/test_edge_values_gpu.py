"""The extreme stored words of tests/edge_corpus.py THROUGH THE STAGES, against the oracle: LDE and commit roots, permutation traces, FRI folds,
whole proofs and openings on inputs chosen so that the device holds 0, 1, p - 1, 0x77FFFFFF and mixtures of the edge set E where every other
GPU test holds uniform words (tests/edge_stage_cases.py has the cases; tests/test_field_edges_cpu.py runs their oracle halves without a GPU).

Inputs cross the ABI as canonical values and are converted, so a chosen stored word w is uploaded as edge_corpus.from_words(w) = w R^-1 mod p.
A CONSTANT column's low-degree extension is constant: it is the one way to put a chosen word into EVERY row of the LDE that the quotient,
opening and leaf-hash kernels read — hence the constant-word matrices beside the alternating, impulse and edge-mix ones, whose LDE rows are
whatever the transform makes of them.
"""
import numpy as np
import pytest

import edge_corpus as ec
import edge_stage_cases as sc
import valida_amd as va
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
P = ec.P


@pytest.fixture(scope="module")
def prover_for(machine, rc):
    """One prover context per configuration, shared by the module's cases"""
    made = {}

    def get(mmcs=sc.KECCAK, log_blowup=1, interpret_air=False, num_queries=40, pow_bits=8):
        key = (mmcs, log_blowup, interpret_air, num_queries, pow_bits)
        if key not in made:
            made[key] = va.Prover(machine, rc, log_blowup=log_blowup, num_queries=num_queries, pow_bits=pow_bits, interpret_air=interpret_air,
                                  hash_kind=va.HASH_POSEIDON16 if mmcs == sc.POSEIDON else va.HASH_KECCAK256)
        return made[key]
    yield get
    made.clear()


@pytest.mark.parametrize("case", sc.LDE_CASES, ids=sc.case_id)
def test_lde_and_commit_roots_of_edge_matrices(prover_for, rc, case):
    p = prover_for(case["mmcs"], case["log_blowup"])
    want = sc.oracle_lde_commit(case, rc)
    for kind, mats in sc.lde_matrices(case["log_h"]).items():
        pd = p.commit_batches([p.upload(m) for m in mats])
        for i in range(len(mats)):
            assert first_mismatch(pd.lde(i), want[kind][0][i]) is None, (kind, "width %d" % mats[i].shape[1])
        assert first_mismatch(pd.root, want[kind][1]) is None, kind


@pytest.mark.parametrize("case", sc.PERM_CASES, ids=sc.case_id)
def test_permutation_trace_of_edge_mains_and_challenges(prover, case):
    main, ch = sc.perm_inputs(case)
    want = sc.oracle_perm_trace(case)
    got, cs = prover.generate_permutation_trace(case["chip"], prover.upload(main), ch)
    assert first_mismatch(got, want) is None
    assert first_mismatch(cs, want[-1, -5:]) is None


@pytest.mark.parametrize("case", sc.FOLD_CASES, ids=sc.case_id)
def test_fri_fold_of_edge_vectors(prover, case):
    f, beta = sc.fold_inputs(case)
    assert first_mismatch(prover.fri_fold(f, beta), sc.oracle_fri_fold(case)) is None


@pytest.mark.parametrize("interpret_air", [False, True], ids=["compiled", "interpreted"])
@pytest.mark.parametrize("case", sc.PROOF_CASES, ids=sc.case_id)
def test_whole_proof_of_edge_traces_gives_the_oracles_bytes(prover_for, rc, case, interpret_air):
    """The traces satisfy no constraint; both provers prove them anyway, and the quotient and permutation folders' four-product groups and the
    openings run on extreme LDE words."""
    p = prover_for(case["mmcs"], case["log_blowup"], interpret_air)
    mt, prep = sc.proof_inputs(case)
    ref = sc.oracle_proof(case, rc)
    proof = p.prove([p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep], debug=True)
    for chip in range(va.NUM_CHIPS):
        assert first_mismatch(proof.debug_perm_trace(chip), ref.perm_trace(chip)) is None, "perm trace of chip %d" % chip
    for chip in range(va.NUM_CHIPS):
        assert first_mismatch(proof.debug_quotient(chip), ref.quotient(chip)) is None, "quotient chunks of chip %d (%s)" % (chip, va.CHIP_NAMES[chip])
    assert first_mismatch(proof.words, ref.words) is None
    assert proof.bytes() == ref.bytes()


@pytest.mark.parametrize("case", sc.OPEN_CASES, ids=sc.case_id)
def test_openings_of_edge_columns_at_edge_points(prover_for, rc, case):
    p = prover_for(num_queries=sc.OPEN_QUERIES, pow_bits=sc.OPEN_POW_BITS)
    rounds, points, obs = sc.open_inputs(case)
    roots, values, proof = sc.oracle_open(case, rc)
    pds = [p.commit_batches([p.upload(m) for m in rnd]) for rnd in rounds]
    for k, pd in enumerate(pds):
        assert first_mismatch(pd.root, roots[k]) is None
    ch = va.Challenger(rc)
    ch.observe(obs)
    opened, words = p.open_multi_batches(pds, points, ch)
    got = np.concatenate([v.ravel() for rnd in opened for mat in rnd for v in mat])
    assert first_mismatch(got, values) is None
    assert first_mismatch(words, proof) is None
    ch2 = va.Challenger(rc)
    ch2.observe(obs)
    heights, widths = [[m.shape[0] for m in rnd] for rnd in rounds], [[m.shape[1] for m in rnd] for rnd in rounds]
    assert va.verify_multi_batches([pd.root for pd in pds], heights, widths, points, opened, words, ch2, rc, num_queries=sc.OPEN_QUERIES, pow_bits=sc.OPEN_POW_BITS) is None
    assert np.array_equal(ch.sample(7), ch2.sample(7))
