"""The field-edge corpus without a GPU.  (1) The field probe's own kernel source (valida_amd/csrc/kernels/field_probe.hip) runs under
tools/hipemu on the whole corpus of tests/edge_corpus.py and is compared word for word with the plain-integer reference tests/field_ref.py:
corpus and reference agree, every operand lies in its op's domain, every named boundary vector is in what the device will be sent.  Under
hipemu the plain C++ forms of the corrections are compiled, so this says nothing about the device's inline assembly and __mulhi forms — that is
tests/test_field_edges_gpu.py, on the same corpus.  (2) The reference itself against the oracle's extension-field and Poseidon code.  (3) The
ORACLE half of every stage case of tests/test_edge_values_gpu.py: the oracle aborts the process on an inverse of zero, so a seeded corpus that
passes here has none.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_corpus as ec
import edge_stage_cases as sc
import field_ref as fr
import valida_amd as va
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ec.P
c_u32p = ctypes.POINTER(ctypes.c_uint32)
OPS = list(va.FIELD_PROBE_OPS)


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "field_probe_emu.cpp")
    out = os.path.join(ROOT, "build", "libfieldprobeemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    k = os.path.join(ROOT, "valida_amd", "csrc", "kernels")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(ROOT, "valida_amd", "csrc", "field.hpp"),
            os.path.join(ROOT, "valida_amd", "csrc", "host", "poseidon_opt.hpp")] + [
        os.path.join(k, f) for f in ("field_probe.hip", "butterfly.hpp", "poseidon_perm.hpp", "launch.hpp", "device_common.hpp", "profiler.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    return ctypes.CDLL(out)


def emu_probe(emu, rc, op, operands):
    code, iw, ow = va.FIELD_PROBE_OPS[op]
    a = np.ascontiguousarray(np.asarray(operands, dtype=np.uint32).T)
    assert a.shape[0] == iw
    n = a.shape[1]
    out = np.zeros((ow, n), dtype=np.uint32)
    sparse = ctypes.c_int(0)
    r = np.ascontiguousarray(rc, dtype=np.uint32)
    assert emu.emu_field_probe(r.ctypes.data_as(c_u32p), ctypes.c_uint32(code), a.ctypes.data_as(c_u32p), ctypes.c_uint64(n), out.ctypes.data_as(c_u32p),
                               ctypes.byref(sparse)) == 0
    return np.ascontiguousarray(out.T), bool(sparse.value)


def has_row(corpus, vec):
    return not ec.missing_rows(corpus, [vec])


def reference(op, operands, rc):
    return fr.apply(op, operands, permute=lambda st: va.poseidon16_permute(rc, st))


@pytest.mark.parametrize("op", OPS)
def test_corpus_holds_every_named_boundary_vector(op):
    c = ec.corpus(op)
    assert c.dtype == np.uint32 and c.shape[1] == va.FIELD_PROBE_OPS[op][1]
    missing = ec.missing_rows(c, ec.boundary_vectors(op))
    assert not missing, missing[:4]


def test_the_bounds_the_table_names_are_the_bounds_of_the_constants():
    assert 4 * (P - 1) ** 2 >> 32 == 0xE1000000 and 0xE1000000 - P == 1761607679 and 0xE1000000 < 2 * P
    assert (2 * P - 1) * (P - 1) >> 32 == 0x70800000 < P and (2 * P - 1) * (P - 1) < P << 32
    assert 2 * P - 1 == 0xF0000001 < 2 ** 32
    assert P * P < P << 31  # the S-box's largest product, (-p)^2
    assert has_row(ec.corpus("monty_reduce_wide"), ((4 * (P - 1) ** 2) & 0xFFFFFFFF, 0xE1000000))
    assert has_row(ec.corpus("monty_reduce"), (((2 * P - 1) * (P - 1)) & 0xFFFFFFFF, 0x70800000))
    assert has_row(ec.corpus("mul"), (2 * P - 1, P - 1)) and has_row(ec.corpus("mul"), (P - 1, 2 * P - 1))
    assert has_row(ec.corpus("sbox_plus"), (0, 0)) and has_row(ec.corpus("monty_signed"), ((P * P) & 0xFFFFFFFF, (P * P) >> 32))


@pytest.mark.parametrize("op", OPS)
def test_probe_source_under_emulation_matches_the_reference(emu, rc, op):
    operands = ec.corpus(op)
    want = reference(op, operands, rc)  # asserts every operand's domain
    got, sparse = emu_probe(emu, rc, op, operands)
    assert sparse, "the sparse-round tables are valid for the project's round constants: `permute` must run the dispatched schedule"
    assert ec.first_mismatch_item(op, operands, got, want) is None
    if op.startswith("bfly"):
        assert (got < P).all(), "an unreduced value leaves the round"


def test_the_vectorised_wide_reduction_is_the_scalar_one():
    c = ec.corpus("monty_reduce_wide")
    rows = np.concatenate([c[:: max(1, len(c) // 4096)], np.asarray(ec.boundary_vectors("monty_reduce_wide"), dtype=np.uint32)])
    want = [fr.monty_reduce_wide(int(lo) | int(hi) << 32) for lo, hi in rows]
    assert fr.apply("monty_reduce_wide", rows).ravel().tolist() == want


def test_the_three_op_tables_agree(emu):
    """The op table exists three times: valida_amd.FIELD_PROBE_OPS, the enum vk::FieldProbeOp (kernels/launch.hpp) and field_probe_shape's
    array (field_probe.hip).  Names and order against the enum's text, shapes against the kernel source through the emulation library."""
    import re

    hdr = open(os.path.join(ROOT, "valida_amd", "csrc", "kernels", "launch.hpp")).read()
    body = re.search(r"enum FieldProbeOp \{(.*?)\}", hdr, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",")]
    assert names[-1] == "FIELD_PROBE_OPS" and all(n.startswith("FP_") for n in names[:-1])
    assert [n[3:].lower() for n in names[:-1]] == list(va.FIELD_PROBE_OPS)
    assert [code for code, _, _ in va.FIELD_PROBE_OPS.values()] == list(range(len(names) - 1))
    for name, (code, iw, ow) in va.FIELD_PROBE_OPS.items():
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        assert emu.emu_field_probe_shape(ctypes.c_uint32(code), ctypes.byref(a), ctypes.byref(b)) == 1, name
        assert (a.value, b.value) == (iw, ow), name
    assert emu.emu_field_probe_shape(ctypes.c_uint32(len(va.FIELD_PROBE_OPS)), ctypes.byref(a), ctypes.byref(b)) == 0


def test_emulated_probe_refuses_items_that_would_read_past_the_twiddle_tables(emu, rc):
    """The range check of low / lowbits is a host function the C entry point and the emulation harness both call before the launch."""
    x = np.zeros((18, 3), dtype=np.uint32)
    out = np.zeros((16, 3), dtype=np.uint32)
    r = np.ascontiguousarray(rc, dtype=np.uint32)
    for op, low, lowbits in (("bfly_dit", 0, 11), ("bfly_dif", 16, 4), ("bfly_dit_lb0", 0, 1), ("bfly_dif_lb0", 1, 0)):
        x[16, 1], x[17, 1] = low, lowbits
        assert emu.emu_field_probe(r.ctypes.data_as(c_u32p), ctypes.c_uint32(va.FIELD_PROBE_OPS[op][0]), x.ctypes.data_as(c_u32p), ctypes.c_uint64(3),
                                   out.ctypes.data_as(c_u32p), None) == 1, op


def test_rust_binding_has_no_bare_keyword_as_an_identifier():
    """No Rust toolchain here, so nothing compiles bindings/rust: a C parameter or field named like a Rust keyword (`in`, `type`, `ref`, ...) would
    be a syntax error in the generated crate.  The generator writes such names as raw identifiers; the committed file has none bare."""
    import re
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings as g

    assert g.rust_ident("in") == "r#in" and g.rust_ident("type") == "r#type" and g.rust_ident("operands") == "operands"
    with pytest.raises(ValueError):
        g.rust_ident("self")
    text = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    idents = re.findall(r"(?<![#\w])(\w+): ", text)
    assert len(idents) > 200
    bare = sorted({i for i in idents if i in g.RUST_KEYWORDS | {"self", "Self", "super", "crate"}})
    assert not bare, bare


def test_probe_wrapper_refuses_malformed_operands():
    with pytest.raises(ValueError):
        va.field_probe(None, "add", np.zeros((4, 3), dtype=np.uint32))
    with pytest.raises(KeyError):
        va.field_probe(None, "no_such_op", np.zeros((4, 2), dtype=np.uint32))


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------------------
def test_reference_extension_field_matches_the_oracle():
    rng = np.random.default_rng(41)
    ops = ec.corpus("ext_mul")
    for r in np.concatenate([ops[:196], ops[rng.integers(0, len(ops), 300)]]).tolist():
        a, b = r[:5], r[5:]
        want = po.ext5_mul([fr.from_words(v) for v in a], [fr.from_words(v) for v in b])
        assert [fr.from_words(v) for v in fr.ext_mul(a, b)] == want.tolist(), (a, b)
    ops = ec.corpus("ext_inv")
    for a in np.concatenate([ops[:79], ops[rng.integers(0, len(ops), 200)]]).tolist():
        if not any(a):
            continue  # the oracle aborts on the inverse of zero; the reference and the device give 0 (field.hpp: "0 -> 0")
        assert fr.ext_inv_plain([fr.from_words(v) for v in a]) == po.ext5_inv([fr.from_words(v) for v in a]).tolist(), a
        assert fr.ext_mul(a, fr.ext_inv(a)) == [fr.to_words(1), 0, 0, 0, 0]


def test_reference_permutation_matches_the_oracle(rc):
    for st in ec.corpus("permute").tolist():
        canon = [fr.from_words(v) for v in st]
        assert [fr.to_words(v) for v in canon] == st
        assert va.poseidon16_permute(rc, canon).tolist() == po.poseidon_permute(rc, canon).tolist()


def test_from_words_gives_the_values_whose_stored_form_is_the_word():
    w = np.array(ec.E, dtype=np.uint64)
    assert [fr.to_words(int(v)) for v in ec.from_words(w)] == ec.E
    for name, m in ec.stage_matrices(8, 3).items():
        assert m.shape == (8, 3) and m.dtype == np.uint32 and (m < P).all(), name
    assert fr.to_words(int(ec.constant_matrix(0x77FFFFFF, 2, 2)[1, 1])) == 0x77FFFFFF


def test_stage_cases_hold_the_vectors_the_bounds_table_names():
    """DESIGN.md "Arithmetic bounds": the stage vectors of its rows exist and hold the stored words they are named for."""
    stored = lambda m: (np.asarray(m, dtype=np.uint64) * np.uint64(fr.R) % np.uint64(P))
    for rows in (64, 512, 1024, 2048):
        for kind, word in (("const_78000000", P - 1), ("const_77ffffff", 0x77FFFFFF), ("const_6fffffff", 0x6FFFFFFF)):
            case = {"rows": rows, "columns": kind}
            assert case in sc.OPEN_CASES
            rounds, points, _ = sc.open_inputs(case)
            assert [m.shape for m in rounds[0]] == [(rows, 3), (rows, 17)] and all((stored(m) == word).all() for m in rounds[0])
            assert all((stored(pts[0]) == P - 1).all() and (stored(pts[1]) != 0).all() for pts in points[0])
        assert {"rows": rows, "columns": "edge_mix"} in sc.OPEN_CASES
    for mmcs in (sc.KECCAK, sc.POSEIDON):
        for b in (1, 2):
            case = {"traces": "const_78000000", "mmcs": mmcs, "log_blowup": b}
            assert case in sc.PROOF_CASES
            assert all((stored(m) == P - 1).all() for m in sc.proof_inputs(case)[0])
            assert {"traces": "edge_mix", "mmcs": mmcs, "log_blowup": b} in sc.PROOF_CASES
            for k in (0, 4, 12, 13):
                assert {"log_h": k, "mmcs": mmcs, "log_blowup": b} in sc.LDE_CASES
    for k in (0, 4, 12, 13):
        mats = sc.lde_matrices(k)
        assert (stored(mats["const_78000000"][2]) == P - 1).all() and set(np.unique(stored(mats["alternating"][0])).tolist()) <= {0, P - 1}
        assert set(np.unique(stored(mats["edge_mix"][2])).tolist()) <= set(ec.E)
    main, ch = sc.perm_inputs({"chip": 2, "rows": 1 << 13, "main": "edge_mix", "challenges": "all_pm1"})
    assert main.shape == (1 << 13, 14) and (stored(ch) == P - 1).all()


# ---- the oracle half of every stage case (tests/test_edge_values_gpu.py runs the device half against the same calls) ----------------------------
@pytest.mark.parametrize("case", sc.LDE_CASES, ids=sc.case_id)
def test_oracle_half_lde_and_commit(case, rc):
    sc.oracle_lde_commit(case, rc)


@pytest.mark.parametrize("case", sc.PERM_CASES, ids=sc.case_id)
def test_oracle_half_perm_trace(case):
    assert sc.oracle_perm_trace(case).shape[0] == case["rows"]


@pytest.mark.parametrize("case", sc.FOLD_CASES, ids=sc.case_id)
def test_oracle_half_fri_fold(case):
    assert sc.oracle_fri_fold(case).shape == (1 << case["log_n"] >> 1, 5)


@pytest.mark.parametrize("case", sc.PROOF_CASES, ids=sc.case_id)
def test_oracle_half_whole_proofs(case, rc):
    assert len(sc.oracle_proof(case, rc).bytes()) > 0


@pytest.mark.parametrize("case", sc.OPEN_CASES, ids=sc.case_id)
def test_oracle_half_openings(case, rc):
    sc.oracle_open(case, rc)
