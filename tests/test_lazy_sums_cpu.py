"""The lazily folded field sums without a GPU.  (1) The lazy-sum probe's own kernel source (valida_amd/csrc/kernels/lazy_probe.hip) under
tools/hipemu on the corpus of tests/lazy_corpus.py, word for word against the plain-integer reference there (the device forms: the same corpus in
tests/test_lazy_sums_gpu.py).  (2) field.hpp's bound-checking build (VG_LAZY_CHECK) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer — a subprocess; nothing sanitized is loaded here — over the same corpus and over every length 1 .. 64: no 64-bit sum
wraps, no high word reaches 2p where it is folded or reduced, and the checker does fire on a sum outside its domain.  (3) The bounds as numbers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lazy_corpus as lc
import lazy_stage_cases as ls
import valida_amd as va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lc.P
c_u32p = ctypes.POINTER(ctypes.c_uint32)
CODE = {name: v[0] for name, v in va.LAZY_PROBE_OPS.items()}


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "lazy_probe_emu.cpp")
    out = os.path.join(ROOT, "build", "liblazyprobeemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    k = os.path.join(ROOT, "valida_amd", "csrc", "kernels")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(ROOT, "valida_amd", "csrc", "field.hpp")] + [
        os.path.join(k, f) for f in ("lazy_probe.hip", "launch.hpp", "device_common.hpp", "profiler.hpp")]
    if _stale(out, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def bounds_program():
    src = os.path.join(ROOT, "tests", "emu", "lazy_bounds_host.cpp")
    out = os.path.join(ROOT, "build", "lazy_bounds_host")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if _stale(out, [src, os.path.join(ROOT, "valida_amd", "csrc", "field.hpp")]):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", out], check=True)
    return out


def run_bounds(program, tmp_path, records):
    """records: [(op, terms, operands)] -> (the completed process, the results per record)."""
    fin, fout = str(tmp_path / "operands.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        for op, terms, operands in records:
            a = np.ascontiguousarray(operands, dtype=np.uint32)
            f.write(np.array([CODE[op], terms, a.shape[0]], dtype=np.uint32).tobytes())
            f.write(a.tobytes())
    r = subprocess.run([program, fin, fout], capture_output=True, text=True)
    res = []
    if r.returncode == 0:
        flat = np.fromfile(fout, dtype=np.uint32)
        at = 0
        for op, terms, operands in records:
            ow = 2 if op == "fold_hi" else 5
            n = len(operands)
            res.append(flat[at:at + n * ow].reshape(n, ow))
            at += n * ow
        assert at == flat.size
    return r, res


def emu_probe(emu, op, terms, operands):
    a = np.ascontiguousarray(np.asarray(operands, dtype=np.uint32).T)
    ow = va.LAZY_PROBE_OPS[op][2]
    out = np.zeros((ow, a.shape[1]), dtype=np.uint32)
    assert emu.emu_lazy_probe(ctypes.c_uint32(CODE[op]), ctypes.c_uint32(terms), a.ctypes.data_as(c_u32p), ctypes.c_uint64(a.shape[1]), out.ctypes.data_as(c_u32p)) == 0
    return np.ascontiguousarray(out.T)


def first_mismatch(operands, got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if bad.size == 0 else (int(bad[0]), operands[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


def test_the_bounds_of_the_fold_schedule_are_the_bounds_of_the_constants():
    """field.hpp, LazyAcc: four products from empty, two after a fold, and no third."""
    pm1 = P - 1
    assert 4 * pm1 ** 2 < 2 ** 64 and 4 * pm1 ** 2 >> 32 < 2 * P and 5 * pm1 ** 2 >= 2 ** 64
    folded = (P << 32) - 1  # the largest value a fold leaves
    assert folded + 2 * pm1 ** 2 < 2 ** 64 and (folded + 2 * pm1 ** 2) >> 32 < 2 * P
    assert (P << 32) + 3 * P * P > 2 ** 64
    assert (folded + 2 * pm1 ** 2) >> 32 == 0xE8800000 and 0xE8800000 * 16 < 31 * P  # 1.9375 p
    # a product with one operand below 2p counts as two
    assert (2 * P - 1) * pm1 <= 2 * P * P and folded + (2 * P - 1) * pm1 < 2 ** 64


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_corpus_holds_every_named_boundary_vector(case):
    op, n = case
    c = lc.corpus(op, n)
    assert c.dtype == np.uint32 and c.shape[1] == lc.in_words(op, n) == va.LAZY_PROBE_OPS[op][1](n)
    assert c.shape[0] >= (lc.N_LOOP if op == "lin_dot_loop" else 1 << 16)
    assert not lc.missing_rows(c, lc.boundary_vectors(op, n))
    pm1 = P - 1
    if op == "fold_hi":
        assert not lc.missing_rows(c, [(lo, hi) for hi in (pm1, P, P + 1, 2 * P - 1) for lo in (0, 1, 2 ** 32 - 1, 2 ** 32 - P)])
    else:
        w = c.shape[1]
        named = [(pm1,) * w]
        if n:  # alternating terms and a one-hot pair
            t = w // n
            named += [tuple(pm1 if (i // t) % 2 == ph else 0 for i in range(w)) for ph in (0, 1)]
            named.append(tuple(pm1 if i in (0, 5) else 0 for i in range(w)))
        assert not lc.missing_rows(c, named)


def test_the_lists_of_lengths_are_the_ones_the_probe_is_built_for(emu):
    assert [c for c in lc.CASES if c[0] == "lin_dot"] == [("lin_dot", n) for n in list(range(1, 18)) + [34]]
    assert [c for c in lc.CASES if c[0] == "ext_dot"] == [("ext_dot", n) for n in range(1, 9)]
    assert list(va.LAZY_PROBE_OPS) == ["fold_hi", "ext_mul", "lin_dot", "ext_dot", "lin_dot_loop"]
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    for name, (code, iw, ow, lengths) in va.LAZY_PROBE_OPS.items():
        for n in range(0, 70):
            ok = emu.emu_lazy_probe_shape(ctypes.c_uint32(code), ctypes.c_uint32(n), ctypes.byref(a), ctypes.byref(b)) == 1
            assert ok == (n in lengths), (name, n)
            if ok:
                assert (a.value, b.value) == (iw(n), ow), (name, n)
    assert emu.emu_lazy_probe_shape(ctypes.c_uint32(len(va.LAZY_PROBE_OPS)), ctypes.c_uint32(0), ctypes.byref(a), ctypes.byref(b)) == 0


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_reference_is_the_big_integer_one(case):
    op, n = case
    c = lc.corpus(op, n)
    rows = np.concatenate([c[:: max(1, len(c) // 64)], c[-len(lc.boundary_vectors(op, n)):]])
    want = lc.reference(op, n, rows)
    assert want.tolist() == [lc.reference_bigint(op, n, r) for r in rows]


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_probe_source_under_emulation_matches_the_reference(emu, case):
    op, n = case
    operands = lc.corpus(op, n)
    want = lc.reference(op, n, operands)  # asserts every operand's domain
    got = emu_probe(emu, op, n, operands)
    assert first_mismatch(operands, got, want) is None
    if op != "fold_hi":
        assert (got < P).all()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_sums_stay_within_their_bounds_on_the_corpus(bounds_program, tmp_path, case):
    op, n = case
    operands = lc.corpus(op, n)
    r, res = run_bounds(bounds_program, tmp_path, [(op, n, operands)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert first_mismatch(operands, res[0], lc.reference(op, n, operands)) is None


def test_sums_stay_within_their_bounds_at_every_length_up_to_64(bounds_program, tmp_path):
    pm1 = P - 1
    rng = np.random.default_rng(64)
    records = []
    for n in range(1, 65):
        w = 6 * n
        rows = [np.full(w, pm1), np.array([pm1 if (i // 6) % 2 == 0 else 0 for i in range(w)]), np.array([pm1 if (i // 6) % 2 == 1 else 0 for i in range(w)])]
        records.append(("lin_dot_loop", n, np.concatenate([np.array(rows, dtype=np.uint64), rng.integers(0, P, (256, w), dtype=np.uint64)]).astype(np.uint32)))
    for n in range(1, 17):  # Ext5 x Ext5 terms: 5 products per limb and term
        w = 10 * n
        records.append(("ext_dot", n, np.concatenate([np.full((1, w), pm1, dtype=np.uint64), rng.integers(0, P, (64, w), dtype=np.uint64)]).astype(np.uint32)))
    r, res = run_bounds(bounds_program, tmp_path, records)
    assert r.returncode == 0, r.stderr[-2000:]
    for (op, n, operands), got in zip(records, res):
        assert first_mismatch(operands, got, lc.reference(op, n, operands)) is None, (op, n)


def test_the_checking_build_fires_outside_the_domain(bounds_program, tmp_path):
    """Words of 2^32 - 1 are no field elements: four such products overflow 64 bits, and a high word of 2p is one too many for a fold."""
    r, _ = run_bounds(bounds_program, tmp_path, [("lin_dot_loop", 5, np.full((1, 30), 0xFFFFFFFF, dtype=np.uint32))])
    assert r.returncode != 0 and "lazy bound broken" in r.stderr
    r, _ = run_bounds(bounds_program, tmp_path, [("fold_hi", 0, np.array([[0, 2 * P]], dtype=np.uint32))])
    assert r.returncode != 0 and "high word >= 2p at a fold" in r.stderr
    r, res = run_bounds(bounds_program, tmp_path, [("fold_hi", 0, np.array([[7, 2 * P - 1]], dtype=np.uint32))])
    assert r.returncode == 0 and res[0].tolist() == [[7, P - 1]]


# ---- the oracle half of every stage case (tests/test_lazy_sums_gpu.py runs the device half against the same calls) ------------------------------
def test_open_layouts_cover_the_widths_and_point_counts():
    widths = {w for lay in ls.OPEN_LAYOUTS.values() for rows, group in lay if rows >= 512 for w, _ in group}
    assert widths == {1, 3, 4, 5, 6, 7, 8, 9, 13, 17, 23}  # through the rows kernel (LDE heights 1024 and 2048)
    per_height = {(name, rows): len({c for _, names in group for c in names}) for name, lay in ls.OPEN_LAYOUTS.items() for rows, group in lay}
    assert {per_height[k] for k in per_height if k[1] >= 512} == {1, 2, 3, 4} and {per_height[k] for k in per_height if k[1] == 256} >= {2, 3, 4}
    assert all(1 <= len(group) <= 3 for lay in ls.OPEN_LAYOUTS.values() for _, group in lay)
    stored = lambda m: np.asarray(m, dtype=np.uint64) * np.uint64(lc.R) % np.uint64(P)
    for kind, word in (("const_%08x" % (P - 1), P - 1), ("const_77ffffff", 0x77FFFFFF)):
        rounds, points, _ = ls.open_inputs({"layout": "np4_np1_row2", "columns": kind})
        assert all((stored(m) == word).all() for m in rounds[0])
        assert (stored(points[0][0][0]) == P - 1).all()


@pytest.mark.parametrize("case", ls.OPEN_CASES, ids=ls.case_id)
def test_oracle_half_openings(case):
    roots, values, proof = ls.oracle_open(case)
    assert roots.shape == (1, 8) and values.size and proof.size


@pytest.mark.parametrize("case", ls.CHIP_CASES, ids=ls.case_id)
def test_oracle_half_chip_stages(case):
    ref = ls.oracle_chips(case)
    mt, _ = ls.chip_inputs(case)
    assert [m.shape[0] for m in mt] == [32 if c == 1 else 256 if c == 12 else case["rows"] for c in range(va.NUM_CHIPS)]
    for chip in range(va.NUM_CHIPS):
        assert ref.quotient(chip).size == mt[chip].shape[0] * 10 and ref.perm_trace(chip).size % (5 * mt[chip].shape[0]) == 0


def test_probe_wrapper_refuses_malformed_operands():
    with pytest.raises(ValueError):
        va.lazy_probe(None, "lin_dot", 3, np.zeros((4, 17), dtype=np.uint32))
    with pytest.raises(ValueError):
        va.lazy_probe(None, "lin_dot", 18, np.zeros((4, 108), dtype=np.uint32))
    with pytest.raises(KeyError):
        va.lazy_probe(None, "no_such_op", 0, np.zeros((4, 2), dtype=np.uint32))
