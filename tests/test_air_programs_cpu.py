"""Captured AIRs, host half: generated programs through the capture (vgpu_air_*), the fold rules and the lowering of air/symbolic.hpp, and
the device interpreters' own source (kernels/quotient.hip) under tools/hipemu.

What a captured program should compute is said by two things that share no code with vair::compile: the oracle's scripted chip (oracle/chips.hpp,
a postfix walk evaluated directly on each of its builders) and eval_py / degree_py of tests/air_script.py (plain integers).  Nothing here needs a
device; the refusals in particular are proven on the host, and nothing refused ever reaches one.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import air_script as A
import valida_amd as va
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
CASES = A.all_cases()
ACCEPTED = [n for n in CASES if n not in A.REFUSED]
FRI = dict(num_queries=5, pow_bits=4)
INVALID_ARG, UNSUPPORTED = -1, -4


def test_every_named_case_is_in_the_corpus():
    assert [n for n in A.NAMED if n not in A.CORPUS] == [] and len(A.NAMED) == len(set(A.NAMED)) == len(A.CORPUS)
    assert sum(n.startswith("generated_") for n in CASES) == 40
    gen = [A.generated(s) for s in range(A.N_GENERATED)]
    assert all(s.width <= 8 and s.prep_width <= 3 and A.degree_py(s)[0] <= 9 for s in gen)
    assert {A.degree_py(s)[1] for s in gen} == {1, 2, 3} and any(s.prep_width for s in gen)  # the draws reach every quotient degree, and preprocessed columns


# ---- the oracle alone, before anything of the product runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCEPTED)
def test_oracle_alone_proves_every_case(rc, name):
    """No case aborts the oracle (it inverts, takes logarithms of heights, indexes rows): its proof of the unsatisfied seeded trace exists, at
    the smallest heights the device tests use, with the quotient matrix they compare against."""
    s = CASES[name]
    chip, lqd = A.set_oracle(s), A.degree_py(s)[1]
    assert po.script_degree(0)[0] == lqd
    for h in (1, 4):
        pre = A.trace(7, h, s.prep_width) if s.prep_width else None
        res = po.prove_machine([chip], [A.trace(3, h, s.width)], rc, log_blowup=lqd, prep=[pre], **FRI)
        assert res.words.size > 0 and res.quotient(0).size == h * (5 << lqd)


# ---- 1. three-way evaluation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCEPTED)
def test_three_way_evaluation(name):
    """vgpu_machine_eval_constraints (the compiled register program) == oracle_eval_constraints (the scripted chip) == eval_py, on 21 rows:
    every 0 / 1 selector combination, rows of 0, 1 and p - 1, words of the edge corpus with selectors anywhere in the field."""
    s = CASES[name]
    mach, chip = A.to_ffi(s), A.set_oracle(s)
    rows = A.eval_rows(1, s.width, s.prep_width)
    assert len(rows) >= 16
    for l, n, pl, pn, f, la, tr in rows:
        want = A.eval_py(s, [int(v) for v in l], [int(v) for v in n], [int(v) for v in pl], [int(v) for v in pn], f, la, tr)
        pa = (pl, pn) if s.prep_width else (None, None)
        assert mach.eval_constraints(0, l, n, *pa, is_first=f, is_last=la, is_transition=tr).tolist() == want
        assert po.eval_constraints(chip, l, n, *pa, is_first=f, is_last=la, is_transition=tr).tolist() == want


# ---- 2. degrees (defect 1) and program shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ACCEPTED)
def test_degree_is_the_references(name):
    s = CASES[name]
    info = A.to_ffi(s).chip_info(0)
    A.set_oracle(s)
    dmax, lqd = A.degree_py(s)
    assert (info["log_quotient_degree"], info["max_degree"], info["constraints"]) == (lqd, dmax, len(s.constraints)) == po.script_degree(0)
    assert (info["width"], info["preprocessed_width"]) == (s.width, s.prep_width)


def test_folded_expressions_keep_the_unsimplified_degree():
    """Defect 1: 0 * x^4 and x^5 - x^5 fold to the constant 0 in the DAG; the reference's SymbolicExpression does not fold, and the same chip
    captured in-tree (DegreeBuilder) gets degree 4 / 5: log_quotient_degree 2, not 1."""
    for name, deg in (("fold_zero_times_x4", 4), ("fold_x5_minus_x5", 5)):
        info = A.to_ffi(CASES[name]).chip_info(0)
        assert (info["max_degree"], info["log_quotient_degree"]) == (deg, 2) == A.degree_py(CASES[name])
    assert [A.degree_py(CASES["degree_%d" % d])[1] for d in (3, 4, 5, 8, 9)] == [1, 2, 2, 3, 3]


def test_degree_10_is_refused():
    codes = []
    A.to_ffi(CASES["degree_10"], codes)
    assert codes[0][0] == UNSUPPORTED and "degree_10" in codes[0][1]


@pytest.mark.parametrize("regs,lqd", A.REGISTER_CASES)
def test_register_counts_reach_every_boundary(regs, lqd):
    """The achieved register count, not the intended one: 1, 31 | 32 | 33 (one VGPR bank, two), 63 | 64 | 65 (two banks, the LDS file), 200, and
    the largest file each LDS kernel holds; the satisfiable variants keep the count."""
    name = "regs_%d_lqd%d" % (regs, lqd)
    info = A.to_ffi(CASES[name]).chip_info(0)
    assert (info["registers"], info["log_quotient_degree"]) == (regs, lqd)
    assert A.to_ffi(A.satisfiable_case(name).script).chip_info(0)["registers"] == regs
    assert (A.MAX_REGS_PAIR, A.MAX_REGS_GENERAL) == (592, 640)


def test_padding_to_whole_quads():
    """Unpadded lengths 4, 5, 6, 7 -> 4, 8, 8, 8 instructions (the VGPR interpreters fetch four at a time); an AIR without constraints has an
    empty program and still evaluates (to nothing)."""
    assert [A.to_ffi(CASES["pad_len%d" % n]).chip_info(0)["instructions"] for n in (4, 5, 6, 7)] == [4, 8, 8, 8]
    m = A.to_ffi(CASES["no_constraints"])
    assert (m.chip_info(0)["instructions"], m.chip_info(0)["registers"], m.chip_info(0)["constraints"]) == (0, 0, 0)
    assert m.eval_constraints(0, np.zeros(3, np.uint32), np.zeros(3, np.uint32)).size == 0


# ---- 3. verdicts ---------------------------------------------------------------------------------------------------------------------------
def _verdicts(mach, chip, words, pre, lqd, rc):
    pc = va.host_commit_root([pre], rc, log_blowup=lqd) if pre is not None else None
    return va.verify(mach, rc, words, pc, log_blowup=lqd, **FRI), po.verify_machine([chip], words, rc, log_blowup=lqd, prep=[pre], **FRI)


@pytest.mark.parametrize("name", ACCEPTED)
def test_verdicts_on_satisfiable_and_broken_traces(rc, name):
    """The oracle's proof of the satisfiable variant is accepted by the product's Machine::verify and by the oracle's; one changed cell gives a
    proof both reject.  A proof opens no preprocessed columns (basic/src/lib.rs:612-613): an AIR whose constraints read one is rejected by both
    verifiers even when honest -- the verdicts still agree."""
    s, fill, free_width, break_col = A.satisfiable_case(name)
    if not s.constraints:
        return
    mach, chip, lqd = A.to_ffi(s), A.set_oracle(s), A.degree_py(s)[1]
    h = 4
    pre = A.trace(7, h, s.prep_width) if s.prep_width else None
    good = fill(A.trace(3, h, free_width), pre, domain=True)
    a, b = _verdicts(mach, chip, po.prove_machine([chip], [good], rc, log_blowup=lqd, prep=[pre], **FRI).words, pre, lqd, rc)
    reads_prep = any(e[0] == "prep" for e in A._postorder(s.constraints))
    if reads_prep:  # (a read that the capture folds away -- 0 * prep -- is no read: then both accept)
        assert (a is None) == (b is None) and (a is None or "preprocessed column" in a)
    else:
        assert a is None and b is None
    bad = good.copy()
    bad[1, break_col] = (int(bad[1, break_col]) + 1) % P  # one cell of a column every row's constraints bind
    a, b = _verdicts(mach, chip, po.prove_machine([chip], [bad], rc, log_blowup=lqd, prep=[pre], **FRI).words, pre, lqd, rc)
    assert a is not None and b is not None


# ---- 4. refusals (defects 2 and 3): on the host, at the call or at vgpu_machine_push_air --------------------------------------------------------
def _push(build, name="refused", width=4, prep_width=0):
    L, u = va.lib(), ctypes.c_uint32
    m, air = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0 and L.vgpu_air_new(name.encode(), u(width), u(prep_width), ctypes.byref(air)) == 0
    try:
        build(L, air, u)
        code = L.vgpu_machine_push_air(m, air)
        return code, L.vgpu_last_error().decode(), int(L.vgpu_machine_num_chips(m))
    finally:
        L.vgpu_air_free(air)
        L.vgpu_machine_free(m)


@pytest.mark.parametrize("is_prep,width,prep_width,column", [(0, 4, 0, 4), (0, 4, 0, 4000), (0, 4, 0, 65535), (0, 4, 0, 65536), (1, 4, 3, 3), (1, 4, 3, 65535), (1, 4, 3, 65536),
                                                             (1, 4, 0, 0), (0, 1, 0, 1)])
def test_column_out_of_range_is_refused(is_prep, width, prep_width, column):
    """Defect 2: a variable outside the AIR (column == width, 65535, 65536 -- which the program's 16-bit column field would wrap to 0 --, any
    preprocessed column of an AIR without preprocessed columns) would be loaded out of bounds by the interpreter."""
    def build(L, air, u):
        L.vgpu_air_assert_zero(air, u(L.vgpu_air_variable(air, u(is_prep), u(column), u(0))))
    code, msg, n = _push(build, "cols", width, prep_width)
    assert code == INVALID_ARG and "'cols'" in msg and "column" in msg and n == 0
    # the last column itself is fine
    ok = _push(lambda L, air, u: L.vgpu_air_assert_zero(air, u(L.vgpu_air_variable(air, u(0), u(width - 1), u(1)))), "cols", width, prep_width)
    assert ok[0] == 0 and ok[2] == 1


@pytest.mark.parametrize("op", ["add_left", "add_right", "sub_left", "sub_right", "mul_left", "mul_right", "neg", "assert_zero"])
def test_node_that_does_not_exist_is_refused(op):
    def build(L, air, u):
        x = L.vgpu_air_variable(air, u(0), u(0), u(0))
        ghost = x + 1  # the next handle: it does not exist yet
        if op == "neg":
            r = L.vgpu_air_neg(air, u(ghost))
        elif op == "assert_zero":
            r = x
            L.vgpu_air_assert_zero(air, u(ghost))
        else:
            f = getattr(L, "vgpu_air_" + op.split("_")[0])
            r = f(air, u(x), u(ghost)) if op.endswith("right") else f(air, u(ghost), u(x))
        L.vgpu_air_assert_zero(air, u(r))  # the bad result is itself no node
    code, msg, n = _push(build, "ghost")
    assert code == INVALID_ARG and "'ghost'" in msg and "does not exist" in msg and ("vgpu_air_" + op.split("_left")[0].split("_right")[0]) in msg and n == 0


@pytest.mark.parametrize("lqd,limit", [(1, A.MAX_REGS_PAIR), (2, A.MAX_REGS_GENERAL), (3, A.MAX_REGS_GENERAL)])
def test_register_file_that_does_not_fit_is_refused(lqd, limit):
    """Defect 3: one register above what the LDS interpreter of this quotient degree holds is refused when the AIR is pushed (the quotient launch
    would ask for more dynamic LDS than the kernel may have); exactly the limit is accepted."""
    assert A.to_ffi(A.held_products(limit - 1, lqd)).chip_info(0)["registers"] == limit
    codes = []
    A.to_ffi(A.held_products(limit, lqd), codes)
    assert codes[0][0] == INVALID_ARG and "registers" in codes[0][1] and str(limit + 1) in codes[0][1] and ("regs_%d_lqd%d" % (limit + 1, lqd)) in codes[0][1]
    codes = []
    A.to_ffi(A.held_products(700, lqd), codes)  # the 701 registers of the probe
    assert codes[0][0] == INVALID_ARG


# ---- 5. the interpreters' own source under emulation ------------------------------------------------------------------------------------------
def _rocm_clang():
    """ROCm's clang++ (the compiler hipcc drives), found beside hipcc."""
    hipcc = shutil.which("hipcc")
    roots = [os.environ.get("ROCM_PATH")] + ([os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))] if hipcc else []) + ["/opt/rocm"]
    for r in roots:
        if r and os.path.exists(os.path.join(r, "llvm", "bin", "clang++")):
            return os.path.join(r, "llvm", "bin", "clang++")
    raise RuntimeError("no ROCm clang++ found beside hipcc: the harness's ext_vector_type register banks need clang")


@pytest.fixture(scope="module")
def emu():
    """tests/emu/quotient_emu.cpp includes kernels/quotient.hip.  The VGPR register files are ext_vector_type vectors: the harness is compiled by
    ROCm's clang++ as a plain host compiler (no offload)."""
    src = os.path.join(ROOT, "tests", "emu", "quotient_emu.cpp")
    out = os.path.join(ROOT, "build", "libquotientemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h"), os.path.join(csrc, "field.hpp"), os.path.join(csrc, "chips", "basic_machine.hpp"),
            os.path.join(csrc, "air", "symbolic.hpp"), os.path.join(csrc, "host", "machine.hpp")] + [
        os.path.join(csrc, "kernels", f) for f in ("quotient.hip", "launch.hpp", "device_common.hpp", "interactions.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run([_rocm_clang(), "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIPCC__", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emu_quotient.restype = ctypes.c_int64
    L.emu_check.restype = ctypes.c_int64
    return L


def _capture_into(emu_lib, s):
    """The script handed to the harness's own AIR (the harness links the capture's source, not libvgpu.so)."""
    u = ctypes.c_uint32
    emu_lib.emu_air_new.restype = ctypes.c_void_p
    air = ctypes.c_void_p(emu_lib.emu_air_new(u(s.width), u(s.prep_width)))

    class Shim:  # air_script.capture speaks vgpu_air_*
        def __getattr__(self, fn):
            return getattr(emu_lib, fn.replace("vgpu_air_", "emu_air_"))
    A.capture(Shim(), air, s)
    return air


def _oracle_stage(s, h, rc, satisfied=False):
    """The oracle's proof of the case at height h: its LDEs in committed (bit-reversed) order, transcript values and quotient matrix."""
    chip, lqd = A.set_oracle(s), A.degree_py(s)[1]
    pre = A.trace(7, h, s.prep_width) if s.prep_width else None
    tr = A.trace(3, h, s.width)
    res = po.prove_machine([chip], [tr], rc, log_blowup=lqd, prep=[pre], **FRI)
    t = res.transcript
    perm = res.perm_trace(0).reshape(h, 5)
    shift = 31
    return dict(lqd=lqd, main=po.committed_lde(tr, lqd, shift), prep=po.committed_lde(pre, lqd, shift) if pre is not None else None, perm=po.committed_lde(perm, lqd, shift),
                rnd=t[8:23], alpha=t[23:28], cum=perm[h - 1], quotient=res.quotient(0).reshape(h, 5 << lqd), trace=tr, pre=pre)


def _emu_quotient(emu_lib, s, st, h, natural):
    """-> (chunk matrix, kernel name, threads, dynamic LDS bytes, registers)"""
    air = _capture_into(emu_lib, s)
    try:
        out = np.zeros((h, 5 << st["lqd"]), np.uint32)
        info, kernel = np.zeros(4, np.uint32), ctypes.create_string_buffer(96)
        pp = st["prep"].ctypes.data_as(po.c_u32p) if st["prep"] is not None else None
        got = emu_lib.emu_quotient(air, ctypes.c_uint32(h.bit_length() - 1), ctypes.c_uint32(st["lqd"]), st["main"].ctypes.data_as(po.c_u32p), pp,
                                   st["perm"].ctypes.data_as(po.c_u32p), st["alpha"].ctypes.data_as(po.c_u32p), np.ascontiguousarray(st["cum"]).ctypes.data_as(po.c_u32p),
                                   ctypes.c_int(natural), out.ctypes.data_as(po.c_u32p), info.ctypes.data_as(po.c_u32p), kernel, ctypes.c_uint64(96))
        assert got == 0
        return out, kernel.value.decode(), int(info[0]), int(info[1]), int(info[2])
    finally:
        emu_lib.emu_air_free(air)


def _bitrev(h):
    k = h.bit_length() - 1
    return np.array([int(format(r, "0%db" % k)[::-1], 2) if k else 0 for r in range(h)])


EMU_SMALL = [n for n in ACCEPTED if not n.startswith("regs_") and n != "constraints_300"]


@pytest.mark.parametrize("name", EMU_SMALL)
def test_quotient_kernels_under_emulation(emu, rc, name):
    """k_quotient / k_quotient_general, interpreting the captured program over the oracle's LDEs: the chunk matrix is the oracle's, word for word
    (bit-reversed row positions, and natural ones for log_quotient_degree 1)."""
    s = CASES[name]
    for h in (1, 2, 4, 64):
        st = _oracle_stage(s, h, rc)
        for natural in ([0, 1] if st["lqd"] == 1 else [0]):
            q, kernel, _, _, _ = _emu_quotient(emu, s, st, h, natural)
            want = st["quotient"] if natural else st["quotient"][_bitrev(h)]
            assert np.array_equal(q, want), (h, natural, kernel)


@pytest.mark.parametrize("regs,lqd", A.REGISTER_CASES)
def test_every_interpreter_instantiation_under_emulation(emu, rc, regs, lqd):
    """The register-file boundaries: which kernel ran is asserted from the launch (one bank up to 32 registers, two up to 64, the LDS file above,
    at 128 and 64 threads), at heights that give the LDS kernels more than one workgroup."""
    s = CASES["regs_%d_lqd%d" % (regs, lqd)]
    want_kernel = "k_quotient%s<%d>" % ("" if lqd == 1 else "_general", 1 if regs <= 32 else 2 if regs <= 64 else 0)
    for h in ((4, 512) if regs in (33, 65, 200) else (128,) if regs >= 592 else (64,)):
        st = _oracle_stage(s, h, rc)
        q, kernel, threads, lds, got_regs = _emu_quotient(emu, s, st, h, 0)
        assert (kernel, got_regs) == (want_kernel, regs)
        assert (threads, lds) == ((256, 0) if regs <= 64 else (128, regs * 128 * 4) if regs <= 128 else (64, regs * 64 * 4))
        assert lds <= (148 if lqd == 1 else 160) * 1024  # the dynamic LDS the kernel may have (launch.hpp)
        assert np.array_equal(q, st["quotient"][_bitrev(h)]), h


def test_emulation_reached_all_six_kernels():
    reached = {("" if q == 1 else "_general", 1 if r <= 32 else 2 if r <= 64 else 0) for r, q in A.REGISTER_CASES}
    assert reached == {(g, k) for g in ("", "_general") for k in (0, 1, 2)}


@pytest.mark.parametrize("name", ["regs_33_lqd1", "regs_65_lqd1", "regs_200_lqd2", "regs_592_lqd1", "regs_640_lqd2", "constraints_300", "load_prep_w7", "every_opcode",
                                  "selectors", "generated_6", "assert_forms"])
def test_check_constraints_kernel_under_emulation(emu, name):
    """k_check_constraints<INTERPRET> (the LDS register file at every size, its launch sizing included) on a satisfied witness and on one with one
    changed cell: the first failing (row, code) is the one eval_py gives."""
    s, fill, free_width, break_col = A.satisfiable_case(name)
    for h in (4, 512) if not name.startswith("regs_") or name == "regs_33_lqd1" else (128,):
        pre = A.trace(7, h, s.prep_width) if s.prep_width else None
        good = fill(A.trace(3, h, free_width), pre)
        assert A.first_failing_row(s, good, pre) is None
        bad = good.copy()
        r = (2 * h) // 3
        bad[r, break_col] = (int(bad[r, break_col]) + 1) % P
        assert A.first_failing_row(s, bad, pre) == r
        air = _capture_into(emu, s)
        try:
            for tr, want in ((good, -1), (bad, (r << 16) | 0xFFFD)):
                pp = pre.ctypes.data_as(po.c_u32p) if pre is not None else None
                info, kernel = np.zeros(4, np.uint32), ctypes.create_string_buffer(96)
                got = emu.emu_check(air, ctypes.c_uint32(h.bit_length() - 1), np.ascontiguousarray(tr).ctypes.data_as(po.c_u32p), pp, info.ctypes.data_as(po.c_u32p), kernel,
                                    ctypes.c_uint64(96))
                assert got == want and "k_check_constraints<QuotientArgs::INTERPRET>" in kernel.value.decode()
                regs = int(info[2])
                assert (int(info[0]), int(info[1])) == ((256, regs * 1024) if regs <= 64 else (128, regs * 512) if regs <= 128 else (64, regs * 256)) and info[1] <= 160 * 1024
        finally:
            emu.emu_air_free(air)
