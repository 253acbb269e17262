"""The batched verifier (vgpu_verify_batch) on the CPU: the kernels of valida_amd/csrc/kernels/verify.hip — the very source — run under
tools/hipemu behind the product's host half (host/verify_batch.hpp), over oracle proofs, honest and tampered, with both MMCS hashes and
captured AIRs of log_quotient_degree 2 and 3.  Every verdict and message must be vgpu_verify's (va.verify) on the same proof."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import valida_amd as va
import verify_corpus as vc
from conftest import pow_machine, pow_trace
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_u32p = ctypes.POINTER(ctypes.c_uint32)
MSG_CAP = 512


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "verify_emu.cpp")
    out = os.path.join(ROOT, "build", "libverifyemu.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    csrc = os.path.join(ROOT, "valida_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tools", "hipemu", "hip", "hip_runtime.h")]
    for base, _, files in os.walk(csrc):
        deps += [os.path.join(base, f) for f in files if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-DVK_ALIGNBIT_NOP=0", "-x", "c++", "-I", os.path.join(ROOT, "tools", "hipemu"), src,
                        "-o", out, "-lpthread"], check=True)
    return ctypes.CDLL(out)


def emu_batch(emu, machine, rc, proofs, commits, chunk_words=0, log_blowup=1, num_queries=40, pow_bits=8, hash_kind=va.HASH_KECCAK256):
    """vgpu_verify_batch through the emulated kernels: one entry per proof, None or the rejection message."""
    n = len(proofs)
    keep = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
    ptrs = (c_u32p * n)(*[k.ctypes.data_as(c_u32p) for k in keep])
    nw = (ctypes.c_uint64 * n)(*[k.size for k in keep])
    pc = None
    if commits is not None:
        flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in commits]))
        pc = flat.ctypes.data_as(c_u32p)
    r = np.ascontiguousarray(rc, dtype=np.uint32)
    status = (ctypes.c_int32 * n)()
    msgs = ctypes.create_string_buffer(n * MSG_CAP)
    code = emu.emu_verify_batch(ctypes.c_void_p(machine._h.value), ctypes.c_uint32(log_blowup), ctypes.c_uint32(num_queries), ctypes.c_uint32(pow_bits),
                                ctypes.c_uint32(int(hash_kind)), ctypes.c_uint32(0), r.ctypes.data_as(c_u32p), ptrs, nw, pc, ctypes.c_uint32(n),
                                ctypes.c_uint64(chunk_words), status, msgs, ctypes.c_uint64(MSG_CAP))
    assert code == 0, msgs.raw[:MSG_CAP].split(b"\0")[0].decode()
    return [None if status[i] == 0 else msgs.raw[i * MSG_CAP:(i + 1) * MSG_CAP].split(b"\0")[0].decode() for i in range(n)]


def _fib_proof(rc, n, num_queries, hash_kind=va.HASH_KECCAK256):
    w = va.Workload.fib(n)
    mt, prep = w.main_traces(), w.preprocessed()
    po.set_mmcs_hash(1 if hash_kind == va.HASH_POSEIDON16 else 0, rc)
    try:
        words = po.prove_basic(mt, prep[0][1], prep[1][1], rc, num_queries=num_queries).words
    finally:
        po.set_mmcs_hash(0)
    return words, va.host_commit_root([m for _, m in prep], rc, hash_kind=hash_kind)


@pytest.mark.parametrize("hash_kind", [va.HASH_KECCAK256, va.HASH_POSEIDON16], ids=["keccak", "poseidon"])
def test_batch_matches_host_verify_on_honest_and_tampered_proofs(emu, machine, rc, hash_kind):
    words, pc = _fib_proof(rc, 25, 3, hash_kind)
    kw = dict(num_queries=3, hash_kind=hash_kind)
    assert va.verify(machine, rc, words, pc, **kw) is None
    bad = vc.mutations(words, 160, seed=9)
    proofs = [words] + bad + [words[:-1].copy(), np.concatenate([words, [0]]).astype(np.uint32), words]
    got = emu_batch(emu, machine, rc, proofs, [pc] * len(proofs), **kw)
    want = [va.verify(machine, rc, p, pc, **kw) for p in proofs]
    assert got == want
    assert got[0] is None and got[-1] is None and all(g is not None for g in got[1:-1])
    assert any("input-round Merkle" in g for g in got[1:-1]) and any("commit-phase Merkle" in g for g in got[1:-1])


def test_mixed_programs_heights_and_chunks(emu, machine, rc):
    """fib proofs of different lengths (different chip heights), each with its own preprocessed commitment, honest and tampered, in one batch;
    the same batch cut into chunks of one proof each gives the same answers."""
    proofs, commits = [], []
    for n, seed in ((25, 1), (40, 2), (90, 3)):
        words, pc = _fib_proof(rc, n, 2)
        proofs += [words] + vc.mutations(words, 12, seed=seed, stride=97)
        commits += [pc] * (len(proofs) - len(commits))
    kw = dict(num_queries=2)
    want = [va.verify(machine, rc, p, c, **kw) for p, c in zip(proofs, commits)]
    assert sum(w is None for w in want) == 3
    assert emu_batch(emu, machine, rc, proofs, commits, **kw) == want
    assert emu_batch(emu, machine, rc, proofs, commits, chunk_words=1, **kw) == want
    # another program's commitment for one proof: rejected by the transcript, the others unaffected
    swapped = list(commits)
    swapped[0] = commits[-1]
    assert emu_batch(emu, machine, rc, proofs, swapped, **kw) == [va.verify(machine, rc, p, c, **kw) for p, c in zip(proofs, swapped)]


def test_captured_airs_of_higher_quotient_degree(emu, rc):
    mach, codes = pow_machine([("pow9", 9, True), ("pow5", 5, False)])
    assert codes == [0, 0]
    traces = [pow_trace(8, 9, 3), pow_trace(32, 5, 3)]
    words = po.prove_machine([po.TEST_POW9, po.TEST_POW5], traces, rc, log_blowup=3, num_queries=5, pow_bits=4).words
    kw = dict(log_blowup=3, num_queries=5, pow_bits=4)
    proofs = [words] + vc.mutations(words, 40, seed=5, stride=3, n_chips=2)
    want = [va.verify(mach, rc, p, None, **kw) for p in proofs]
    assert want[0] is None and all(w is not None for w in want[1:])
    assert emu_batch(emu, mach, rc, proofs, None, **kw) == want


def test_hostile_shapes_are_rejected_with_the_host_messages(emu, machine, rc):
    words, pc = _fib_proof(rc, 25, 3)
    corpus = vc.hostile(words)
    proofs = [w for _, w in corpus] + [words]
    kw = dict(num_queries=3)
    want = [va.verify(machine, rc, p, pc, **kw) for p in proofs]
    assert want[-1] is None and all(w is not None for w in want[:-1]), [(l, w) for (l, _), w in zip(corpus, want)]
    assert emu_batch(emu, machine, rc, proofs, [pc] * len(proofs), **kw) == want
    # the wrong query count is a property of the configuration
    assert emu_batch(emu, machine, rc, [words], [pc], num_queries=4) == [va.verify(machine, rc, words, pc, num_queries=4)]
