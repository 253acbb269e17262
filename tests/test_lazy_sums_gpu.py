"""The lazily folded field sums ON THE DEVICE.  (1) The lazy-sum probe (kernels/lazy_probe.hip: fold_hi, the Ext5 product, sums of every length the
kernels unroll) in its device forms — carry-out + v_cndmask inline assembly where the emulation of tests/test_lazy_sums_cpu.py compiles plain C++
— on the corpus of tests/lazy_corpus.py, word for word against the plain-integer reference.  (2) The stages whose sums are folded lazily, against
the oracle, at the smallest shapes that take the changed paths (tests/lazy_stage_cases.py): openings through both reduced-openings kernels,
and the permutation trace and the quotient of every chip, one stage call each.
"""
import numpy as np
import pytest

import lazy_corpus as lc
import lazy_stage_cases as ls
import valida_amd as va
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
P = lc.P


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_device_probe_matches_the_reference(prover, case):
    op, n = case
    operands = lc.corpus(op, n)
    assert not lc.missing_rows(operands, lc.boundary_vectors(op, n))
    want = lc.reference(op, n, operands)  # asserts every operand's domain
    got = va.lazy_probe(prover, op, n, operands)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]), operands[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.fixture(scope="module")
def open_prover(machine, rc):
    return va.Prover(machine, rc, num_queries=ls.OPEN_QUERIES, pow_bits=ls.OPEN_POW_BITS)


@pytest.mark.parametrize("case", ls.OPEN_CASES, ids=ls.case_id)
def test_openings_through_both_reduced_openings_kernels(open_prover, rc, case):
    p = open_prover
    rounds, points, obs = ls.open_inputs(case)
    roots, values, proof = ls.oracle_open(case)
    pds = [p.commit_batches([p.upload(m) for m in rnd]) for rnd in rounds]
    for k, pd in enumerate(pds):
        assert first_mismatch(pd.root, roots[k]) is None
    ch = va.Challenger(rc)
    ch.observe(obs)
    opened, words = p.open_multi_batches(pds, points, ch)
    got = np.concatenate([v.ravel() for rnd in opened for mat in rnd for v in mat])
    assert first_mismatch(got, values) is None
    assert first_mismatch(words, proof) is None


@pytest.fixture(scope="module")
def chip_stages(prover, rc):
    """case -> (permutation traces, quotient chunks) of all fourteen chips from one stage call each, driven as a host drives Machine::prove
    (basic/src/lib.rs:185-590); computed once per case, shared by the two tests below."""
    made = {}

    def get(case):
        key = ls.case_id(case)
        if key not in made:
            p = prover
            mt, prep = ls.chip_inputs(case)
            dmain = [p.upload(m) for m in mt]
            dprep = [(c, p.upload(m)) for c, m in prep]
            slot = {c: k for k, (c, _) in enumerate(dprep)}
            ch = va.Challenger(rc)
            prep_pd = p.commit_batches([t for _, t in dprep])
            ch.observe(prep_pd.root)
            main_pd = p.commit_batches(dmain)
            ch.observe(main_pd.root)
            rnd = ch.sample(15)
            perm, cums = [], []
            for i in range(va.NUM_CHIPS):
                t, cs = p.permutation_trace_device(i, dmain[i], rnd, dprep[slot[i]][1] if i in slot else None)
                perm.append(t)
                cums.append(cs)
            perm_pd = p.commit_batches(perm)
            ch.observe(perm_pd.root)
            alpha = ch.sample(5)
            quot = [p.quotient(i, main_pd, i, perm_pd, i, rnd, alpha, cums[i], prep_pd if i in slot else None, slot.get(i, 0)).download() for i in range(va.NUM_CHIPS)]
            made[key] = ([t.download() for t in perm], quot)
        return made[key]
    yield get
    made.clear()


@pytest.mark.parametrize("case", ls.CHIP_CASES, ids=ls.case_id)
def test_permutation_trace_of_every_chip(chip_stages, case):
    ref = ls.oracle_chips(case)
    perm, _ = chip_stages(case)
    for chip in range(va.NUM_CHIPS):
        assert first_mismatch(perm[chip], ref.perm_trace(chip).reshape(perm[chip].shape)) is None, "perm trace of chip %d (%s)" % (chip, va.CHIP_NAMES[chip])


@pytest.mark.parametrize("case", ls.CHIP_CASES, ids=ls.case_id)
def test_quotient_of_every_chip(chip_stages, case):
    ref = ls.oracle_chips(case)
    _, quot = chip_stages(case)
    for chip in range(va.NUM_CHIPS):
        q = quot[chip]
        assert first_mismatch(q[ls.bitrev_rows(q.shape[0])], ref.quotient(chip).reshape(q.shape)) is None, "quotient chunks of chip %d (%s)" % (chip, va.CHIP_NAMES[chip])
