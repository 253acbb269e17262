"""The batched verifier on the MI355X (vgpu_verify_batch, valida_amd.Verifier): GPU proofs of every configuration accepted, and on
tampered, hostile and mixed batches every verdict and message equal to the host verifier's (vgpu_verify) on the same proof."""
import os
import subprocess
import sys

import pytest

import valida_amd as va
import verify_corpus as vc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prove(machine, rc, w, **kw):
    p = va.Prover(machine, rc, **kw)
    mt, prep = w.main_traces(), w.preprocessed()
    words = p.prove([p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]).words
    pc = va.host_commit_root([m for _, m in prep], rc, log_blowup=kw.get("log_blowup", 1), hash_kind=kw.get("hash_kind", va.HASH_KECCAK256))
    return words, pc


CONFIGS = {
    "c1": (lambda: va.Workload.fib(25), {}),
    "c2": (lambda: va.Workload.fib(149794), {}),
    "c3_blowup4": (lambda: va.Workload.fib(599183), {"log_blowup": 2}),
    "c4": (lambda: va.Workload.alu(116507), {}),
    "c2_poseidon": (lambda: va.Workload.fib(149794), {"hash_kind": va.HASH_POSEIDON16}),
    "c4_poseidon": (lambda: va.Workload.alu(116507), {"hash_kind": va.HASH_POSEIDON16}),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_honest_proofs_of_every_configuration_are_accepted(machine, rc, name):
    make, kw = CONFIGS[name]
    words, pc = _prove(machine, rc, make(), **kw)
    v = va.Verifier(machine, rc, **kw)
    assert v.verify_batch([words], [pc]) == [None]
    assert va.verify(machine, rc, words, pc, **kw) is None
    host_ms, device_ms = v.timing()
    assert host_ms > 0 and device_ms > 0


def test_named_programs_in_one_batch(machine, rc):
    names = ["left_imm_ops", "signed_inequality", "loadfp", "static_data"]
    proofs, commits = [], []
    for n in names + ["mixed_ops:40"]:
        words, pc = _prove(machine, rc, va.Workload.named(n))
        proofs.append(words)
        commits.append(pc)
    # mixed_ops runs the reference's stub chips (mul / div / shift / com): its proof is well-formed but no verifier accepts it
    want = [None] * len(names) + [va.verify(machine, rc, proofs[-1], commits[-1])]
    assert want[-1] is not None and "out-of-domain constraint mismatch" in want[-1]
    assert va.Verifier(machine, rc).verify_batch(proofs, commits) == want
    # every proof against another program's commitment: the transcript differs, rejected as the host rejects it
    rolled = commits[1:] + commits[:1]
    want = [va.verify(machine, rc, p, c) for p, c in zip(proofs, rolled)]
    assert all(w is not None for w in want)
    assert va.Verifier(machine, rc).verify_batch(proofs, rolled) == want


@pytest.fixture(scope="module")
def fib_proofs(machine, rc):
    return {n: _prove(machine, rc, va.Workload.fib(n)) for n in (25, 40, 90, 582)}


def test_mutations_mixed_with_honest_proofs_match_the_host_verifier(machine, rc, fib_proofs):
    words, pc = fib_proofs[25]
    c2, c2pc = _prove(machine, rc, va.Workload.fib(149794))
    bad25 = vc.mutations(words, 1000, seed=11, stride=2)
    bad_c2 = vc.mutations(c2, 120, seed=12, stride=23)
    assert len(bad25) >= 1000 and len(bad_c2) >= 200
    proofs, commits = [], []
    for i, b in enumerate(bad25):
        proofs.append(b)
        commits.append(pc)
        if i % 50 == 0:  # honest proofs of other lengths in between
            n = (40, 90, 582)[(i // 50) % 3]
            proofs.append(fib_proofs[n][0])
            commits.append(fib_proofs[n][1])
    proofs += bad_c2 + [c2, words]
    commits += [c2pc] * (len(bad_c2) + 1) + [pc]
    got = va.Verifier(machine, rc).verify_batch(proofs, commits)
    want = [va.verify(machine, rc, p, c) for p, c in zip(proofs, commits)]
    assert got == want
    assert got[-1] is None and got[-2] is None
    assert sum(g is None for g in got) == 2 + (len(bad25) + 49) // 50
    # the oracle's verifier rejects every mutated proof too
    w25 = va.Workload.fib(25).preprocessed()
    wc2 = va.Workload.fib(149794).preprocessed()
    for b in bad25:
        assert po.verify_basic(w25[0][1], w25[1][1], b, rc) is not None
    for b in bad_c2:
        assert po.verify_basic(wc2[0][1], wc2[1][1], b, rc) is not None


def test_hostile_shapes_are_rejected_without_a_device_error(machine, rc, fib_proofs):
    words, pc = fib_proofs[25]
    corpus = vc.hostile(words)
    proofs = [w for _, w in corpus] + [words]
    want = [va.verify(machine, rc, p, pc) for p in proofs]
    assert want[-1] is None and all(w is not None for w in want[:-1])
    assert va.Verifier(machine, rc).verify_batch(proofs, [pc] * len(proofs)) == want
    assert va.Verifier(machine, rc, num_queries=39).verify_batch([words], [pc]) == [va.verify(machine, rc, words, pc, num_queries=39)]


def test_a_batch_larger_than_one_chunk(machine, rc, fib_proofs):
    proofs, commits = [], []
    for n, (words, pc) in sorted(fib_proofs.items()):
        proofs += [words] + vc.mutations(words, 20, seed=n, stride=211)
        commits += [pc] * (len(proofs) - len(commits))
    v = va.Verifier(machine, rc)
    whole = v.verify_batch(proofs, commits)
    v.set_chunk_words(max(p.size for p in proofs))  # one proof per chunk
    assert v.verify_batch(proofs, commits) == whole
    v.set_chunk_words(3 * max(p.size for p in proofs))
    assert v.verify_batch(proofs, commits) == whole
    assert whole == [va.verify(machine, rc, p, c) for p, c in zip(proofs, commits)]
    assert v.verify_batch([], []) == []


def test_command_line_on_the_device(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "fib25_q4_proof.cbor")
    base = [sys.executable, "-m", "valida_amd.verify_cli", "--program", "fib", "--n", "25", "--queries", "4", "--device", "0"]
    r = subprocess.run(base + [golden], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "accepted", r.stdout + r.stderr
    words = va.proof_from_cbor(open(golden, "rb").read())
    bad = tmp_path / "bad.bin"
    bad.write_bytes(vc.mutate(words, words.size - 20).astype("<u4").tobytes())
    r = subprocess.run(base + [str(bad)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("REJECTED: verify:"), r.stdout + r.stderr
    r = subprocess.run(base + [golden, str(bad)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.splitlines()[0].endswith(": accepted") and "REJECTED" in r.stdout.splitlines()[1]
