"""The DEVICE forms of the field arithmetic at their extreme operands.  Under __HIP_DEVICE_COMPILE__ reduce_once / sub_mod are carry-out +
v_cndmask inline assembly and the S-box multiplies through __mulhi; the hipemu tests compile the plain C++ forms instead, and every other GPU
test draws canonical operands uniformly, so a correction that gives p instead of 0, a missing second subtraction or a wrong sign would need a
2^-31 event to show.  Here the field probe (valida_amd.field_probe: the real functions from the real headers, raw stored words in and out) runs
each primitive in ONE launch on the corpus of tests/edge_corpus.py — every named boundary vector asserted present — and is compared word for
word with the plain-integer reference tests/field_ref.py.  tests/test_field_edges_cpu.py runs the same corpus without a GPU.
"""
import numpy as np
import pytest

import edge_corpus as ec
import field_ref as fr
import valida_amd as va

pytestmark = pytest.mark.gpu
P = ec.P


@pytest.fixture(scope="module")
def want(rc):
    """op -> the reference's words, computed once per op"""
    cache = {}

    def get(op):
        if op not in cache:
            cache[op] = fr.apply(op, ec.corpus(op), permute=lambda st: va.poseidon16_permute(rc, st))
        return cache[op]
    return get


@pytest.mark.parametrize("op", list(va.FIELD_PROBE_OPS))
def test_device_primitive_matches_the_integer_reference_on_the_edge_corpus(prover, want, op):
    operands = ec.corpus(op)
    missing = ec.missing_rows(operands, ec.boundary_vectors(op))
    assert not missing, missing[:4]
    got = va.field_probe(prover, op, operands)  # one launch, no item skipped
    assert got.shape == want(op).shape
    assert ec.first_mismatch_item(op, operands, got, want(op)) is None
    if op.startswith("bfly"):
        assert (got < P).all(), "an unreduced value leaves the round"


def test_poseidon_mmcs_context_dispatches_the_same_permutation(machine, rc, want):
    p = va.Prover(machine, rc, hash_kind=va.HASH_POSEIDON16)
    for op in ("permute", "permute_plain"):
        assert ec.first_mismatch_item(op, ec.corpus(op), va.field_probe(p, op, ec.corpus(op)), want(op)) is None


def test_probe_refuses_items_that_would_read_past_the_twiddle_tables(prover):
    x = np.zeros((3, 18), dtype=np.uint32)
    for op, low, lowbits in (("bfly_dit", 0, 11), ("bfly_dif", 16, 4), ("bfly_dit_lb0", 0, 1), ("bfly_dif_lb0", 1, 0)):
        x[1, 16], x[1, 17] = low, lowbits
        with pytest.raises(va.VgpuError) as e:
            va.field_probe(prover, op, x)
        assert e.value.code == -1, op
