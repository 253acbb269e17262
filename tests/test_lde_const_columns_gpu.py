"""Constant trace columns in the fused LDE, on the GPU (kernels/layout.hip: k_ingest's flags; kernels/ntt.hip: k_lde_colmap, k_lde_fill_const, the
mapped three passes).  No proof word may depend on the switch: the pattern matrices of tests/test_lde_const_columns_cpu.py at 2^13 x 17, blowup 2,
through the main round's commitment (vgpu_commit_batches_flagged) with the switch on and off — roots and LDEs equal each other and the oracle's, the
flags equal numpy's — and whole proofs of fib(582) and alu(100) against the committed oracle fixtures with both settings, fib(582) also with the
pool-poison hook set."""
import hashlib
import json
import os

import numpy as np
import pytest

import test_lde_const_columns_cpu as cc
import valida_amd as va
from conftest import first_mismatch
from oracle import pyoracle as po  # checker only

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LOG_N, W, LOG_BLOWUP = 13, 17, 1

_REF = {}


def pattern(name):
    """(matrix, constant mask, oracle LDE, oracle root) of one pattern: computed once, shared by both settings."""
    if name not in _REF:
        rng = np.random.default_rng(1700 + sorted(cc.patterns(W)).index(name))
        m = np.ascontiguousarray(np.stack([cc.column(k, 1 << LOG_N, rng) for k in cc.patterns(W)[name]], axis=1), dtype=np.uint32)
        _REF[name] = (m, (m == m[0]).all(0), po.committed_lde(m, LOG_BLOWUP, cc.SHIFT), po.commit_root([m], log_blowup=LOG_BLOWUP))
    return _REF[name]


@pytest.fixture(scope="module")
def provers(machine, rc):
    on, off = va.Prover(machine, rc), va.Prover(machine, rc)
    off.set_const_columns(False)
    return {"on": on, "off": off}


@pytest.mark.parametrize("setting", ["on", "off"])
@pytest.mark.parametrize("name", sorted(cc.patterns(W)))
def test_pattern_matrices_commit_to_the_oracles_root_and_lde(provers, name, setting):
    m, const, want_lde, want_root = pattern(name)
    p = provers[setting]
    pd, flags = p.commit_batches_flagged([p.upload(m)])
    assert np.array_equal(flags[0] == 0, const), "flags differ from (m == m[0]).all(0): %s" % flags[0]
    assert first_mismatch(pd.root, want_root) is None
    assert first_mismatch(pd.lde(0), want_lde) is None
    plain = p.commit_batches([p.upload(m)])  # no map: as before
    assert first_mismatch(plain.root, want_root) is None
    assert first_mismatch(plain.lde(0), want_lde) is None


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        g = json.load(f)
    w = va.Workload.fib(g["n"]) if isinstance(g["n"], int) else va.Workload.alu(g["n"][1])
    mt, prep = w.main_traces(), w.preprocessed()
    assert hashlib.sha256(b"".join(m.tobytes() for m in mt)).hexdigest() == g["traces_sha256"]
    return g, mt, prep


def _assert_golden(p, g, mt, prep, what):
    proof = p.prove([p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep])
    assert proof.words.size == g["proof_words"], what
    assert [int(x) for x in proof.words[2:26]] == g["commitments"], what
    assert hashlib.sha256(proof.bytes()).hexdigest() == g["proof_sha256"], what


@pytest.mark.parametrize("setting", ["on", "off"])
@pytest.mark.parametrize("fixture", ["fib582_oracle.json", "alu100_oracle.json"])
def test_whole_proofs_are_the_oracles_with_both_settings(provers, fixture, setting):
    g, mt, prep = _golden(fixture)
    _assert_golden(provers[setting], g, mt, prep, "%s, constant columns %s" % (fixture, setting))


def test_fib582_really_has_constant_columns(provers):
    """The feature cannot be silently inactive: the device flags of fib(582)'s cpu trace name at least 10 constant columns, the mem trace (2^14 rows:
    the only trace of this proof tall enough for the three-pass LDE, so the one whose columns are filled) at least one, and both equal numpy's."""
    _, mt, _ = _golden("fib582_oracle.json")
    p = provers["on"]
    cpu, mem = mt[0], mt[2]
    assert mem.shape[0] == 1 << 14
    _, flags = p.commit_batches_flagged([p.upload(cpu), p.upload(mem)])
    for m, f in zip((cpu, mem), flags):
        assert np.array_equal(f == 0, (m == m[0]).all(0))
    assert int((flags[0] == 0).sum()) >= 10, flags[0]
    assert int((flags[1] == 0).sum()) >= 1, flags[1]


@pytest.mark.parametrize("word", [0x00000001, 0x5A5A5A5A, 0xFFFFFFFF])
def test_fib582_with_the_pool_poisoned(machine, rc, word):
    """The flags and the map come from the pool: written in full before they are read, whatever the block held (every block filled on alloc and on release)."""
    g, mt, prep = _golden("fib582_oracle.json")
    p = va.Prover(machine, rc)
    p.set_pool_poison(word)
    before = p.pool_poison_stats()
    _assert_golden(p, g, mt, prep, "first proof, pool word %08x" % word)
    _assert_golden(p, g, mt, prep, "second proof (recycled blocks), pool word %08x" % word)
    m, const, want_lde, want_root = pattern("mixed")
    pd, flags = p.commit_batches_flagged([p.upload(m)])
    assert np.array_equal(flags[0] == 0, const)
    assert first_mismatch(pd.root, want_root) is None
    assert first_mismatch(pd.lde(0), want_lde) is None
    assert all(a > b for a, b in zip(p.pool_poison_stats(), before)), "the pool filled nothing during this test"
