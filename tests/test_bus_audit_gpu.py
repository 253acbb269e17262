"""The bus audit on the MI355X (vgpu_bus_audit; kernels/bus_audit.hip) against the independent numpy restatement of tests/bus_audit_ref.py: every
input of the issue's table under both machine kinds, from uploaded traces and from traces generated on the device; the collision path forced with
8- and 16-bit keys; truncation; full size (C2); an audit between two proofs; the `check` action of the command line on device 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bus_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_bus_audit_cpu import ADD, BALANCED, C2_FAULTS, CPU, GENERAL, MEM, MEMORY, RANGE, RANGE_CHIP, exe, witness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def audit_all(provers, w, faults=(), generated=True, **kw):
    """The reference's report and the device's: uploaded traces under both machine kinds and (unfaulted witnesses) traces generated on the device,
    which the interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = witness(w, faults)
    r = ref.audit(provers["basic"].machine, mt, prep)
    reps = [p.bus_audit(*upload(p, mt, prep), **kw) for p in provers.values()]
    if generated and not faults:
        main, pre = generate(provers["basic"], w)
        reps += [p.bus_audit(main, pre, **kw) for p in provers.values()]
    for rep in reps:
        ref.assert_report_equals(rep, r, kw.get("max_tuples", 64), kw.get("max_records_per_tuple", 4))
        assert np.array_equal(rep.words, reps[0].words) and rep.device_ms > 0
    return r, reps[0]


@pytest.mark.parametrize("name", list(BALANCED))
def test_balanced_witnesses(provers, name):
    r, rep = audit_all(provers, BALANCED[name]())
    assert rep.balanced and rep.total_unbalanced == 0 and rep.tuples == [] and [b["width"] for b in rep.buses] == [14, 8, 1]


def test_faults_in_fib25(provers, fib25):
    r, rep = audit_all(provers, fib25, [(RANGE_CHIP, 7, 0)], max_records_per_tuple=1000)
    (t,) = rep.tuples
    assert t["bus"] == RANGE and t["fields"] == [7] and t["net_signed"] == -1 and t["records"][-1][:4] == (RANGE_CHIP, 7, 0, 0)
    assert all(rec[0] == ADD and rec[3] == 1 for rec in t["records"][:-1])
    r, rep = audit_all(provers, fib25, [(ADD, 5, 11)])
    assert rep.total_unbalanced == 4 and sorted(t["bus"] for t in rep.tuples) == [GENERAL, GENERAL, RANGE, RANGE]


def test_store_byte_and_echo(provers):
    r, rep = audit_all(provers, exe(vp.store_byte_program()))
    assert rep.total_unbalanced == 5 and [t["bus"] for t in rep.tuples] == [MEMORY] * 5 and [t["net_signed"] for t in rep.tuples] == [-1] * 5
    assert [t["records"] for t in rep.tuples] == [[(MEM, row, 0, 0, 1)] for row in range(15, 20)] and [t["fields"][1] for t in rep.tuples] == [4, 6, 8, 10, 13]
    r, rep = audit_all(provers, exe(vp.echo_program(3), b"abc"))
    assert rep.total_unbalanced == 6 and [t["net_signed"] for t in rep.tuples] == [1, 1, 1, -1, -1, -1]
    assert [t["fields"][4] for t in rep.tuples] == [97, 98, 99] * 2 and [t["fields"][13] for t in rep.tuples] == [0, 0, 0, 1, 3, 5]


@pytest.mark.parametrize("name,total,general,range_", [("mixed_ops:40", 640, 406, 234), ("mixed_ops:700", 6917, 6661, 256)])
def test_mixed_ops(provers, name, total, general, range_):
    r, rep = audit_all(provers, va.Workload.named(name), max_tuples=10000)
    assert rep.total_unbalanced == total == rep.reported and {b["bus"]: b["unbalanced"] for b in rep.buses} == {GENERAL: general, MEMORY: 0, RANGE: range_}


@pytest.mark.parametrize("name", ["mixed_ops:700", "store_byte", "fib9359"])
def test_key_collisions_do_not_change_the_report(provers, name):
    """hash_bits 8 and 16: mixed_ops:700 and fib(9359) have far more than 2^8 distinct tuples, so at 8 bits their keys collide whatever the mix is
    (and with 115 070 / 505 724 live records over 2^16 keys at 16 bits too); store_byte (50 tuples) is here for its verdict."""
    w = {"mixed_ops:700": lambda: va.Workload.named("mixed_ops:700"), "store_byte": lambda: exe(vp.store_byte_program()), "fib9359": lambda: va.Workload.fib(9359)}[name]()
    mt, prep = witness(w)
    r = ref.audit(provers["basic"].machine, mt, prep)
    if name != "store_byte":
        assert r["live"] > 1 << 16
    for kind, p in provers.items():
        main, pre = upload(p, mt, prep)
        full = p.bus_audit(main, pre, max_tuples=10000)
        ref.assert_report_equals(full, r, 10000, 4)
        for bits in (8, 16):
            cut = p.bus_audit(main, pre, max_tuples=10000, hash_bits=bits)
            assert np.array_equal(cut.words, full.words), (kind, bits)


@pytest.mark.parametrize("max_tuples", [1, 64, 10000])
@pytest.mark.parametrize("max_records", [1, 4])
def test_truncation(provers, max_tuples, max_records):
    mt, prep = witness(va.Workload.named("mixed_ops:700"))
    r = ref.audit(provers["basic"].machine, mt, prep)
    p = provers["basic"]
    rep = p.bus_audit(*upload(p, mt, prep), max_tuples=max_tuples, max_records_per_tuple=max_records)
    ref.assert_report_equals(rep, r, max_tuples, max_records)
    assert rep.total_unbalanced == 6917 and rep.reported == min(max_tuples, 6917) and rep.truncated == (max_tuples < 6917)


def test_full_size_c2(provers):
    """C2 (fib(149794): 2^20 cpu rows, 2^22 memory rows) balanced, from generated and from uploaded traces; then the two faults of the issue against the
    reference (computed once: about 20 s and 3 GB on one host core)."""
    w = va.Workload.fib(149794)
    assert w.cpu_height == 1 << 20
    p = provers["basic"]
    main, pre = generate(p, w)
    rep = p.bus_audit(main, pre)
    assert rep.balanced and {b["bus"]: b["live"] for b in rep.buses} == {GENERAL: 1198362, MEMORY: 4493872, RANGE: 2396980}
    print("C2 balanced, generated traces: device %.3f ms, call %.3f ms" % (rep.device_ms, rep.host_ms))
    assert provers["ffi"].bus_audit(main, pre).balanced
    del main, pre
    mt, prep = witness(w, C2_FAULTS)
    r = ref.audit(p.machine, mt, prep)
    assert r["pairs"] == 13632781 and r["live"] == 8089214 and r["total_unbalanced"] == 3
    for q in provers.values():
        rep = q.bus_audit(*upload(q, mt, prep))
        ref.assert_report_equals(rep, r)
    print("C2 faulted, uploaded traces: device %.3f ms, call %.3f ms" % (rep.device_ms, rep.host_ms))
    a, b, c = rep.tuples
    assert (a["bus"], a["fields"], a["net_signed"], a["records"]) == (MEMORY, [1, 43217, 4048, 0, 215, 242, 210, 40], 1, [(CPU, 43217, 0, 1, 1)])
    assert (b["bus"], b["fields"], b["net_signed"], b["records"]) == (MEMORY, [1, 43217, 4048, 0, 215, 242, 210, 41], -1, [(MEM, 12345, 0, 0, 1)])
    assert (c["bus"], c["fields"], c["net_signed"]) == (RANGE, [7], -1) and [rec[:2] for rec in c["records"]] == [(ADD, 29), (ADD, 110), (ADD, 112), (ADD, 115)]


def test_audit_between_two_proofs(prover):
    """A context runs one thing at a time; an audit leaves nothing behind: the next proof is its golden one and the pool's live bytes are what they were."""
    with open(os.path.join(ROOT, "tests", "golden", "fib582_oracle.json")) as f:
        g = json.load(f)
    w = va.Workload.fib(g["n"])
    mt, prep = witness(w)
    main, pre = upload(prover, mt, prep)
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]
    live_before = prover.memory()[0]
    rep = prover.bus_audit(main, pre)
    assert rep.balanced and prover.memory()[0] == live_before
    bad = prover.upload(np.where(np.arange(mt[ADD].size).reshape(mt[ADD].shape) == 11, (mt[ADD].astype(np.uint64) + 1) % P, mt[ADD]).astype(np.uint32))
    assert not prover.bus_audit(main[:ADD] + [bad] + main[ADD + 1:], pre, hash_bits=8).balanced
    del bad
    assert prover.memory()[0] == live_before
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]


def test_device_argument_validation(prover, fib25):
    mt, prep = witness(fib25)
    main, pre = upload(prover, mt, prep)
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])),
                      ("has no preprocessed columns", dict(pre=pre + [(ADD, main[ADD])])), ("hash_bits", dict(hash_bits=65)), ("hash_bits", dict(hash_bits=0))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.bus_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_on_the_device(tmp_path):
    sb, loop, adv, out = tmp_path / "store_byte.bin", tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json"
    sb.write_bytes(vp.machine_code(vp.store_byte_program()))
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", sb, out, "--device", 0)
    assert r.returncode == 1, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 6 and lines[-1].startswith("unbalanced: 5 tuples")
    for line, clk in zip(lines, (4, 6, 8, 10, 13)):
        assert line.startswith("memory bus [1, %d, " % clk) and line.endswith("cycle %d: pc %d STOREU8" % (clk, clk))
    j = json.loads(out.read_text())
    assert j["total_unbalanced"] == 5 and j["device_ms"] > 0
    r = _cli("check", loop, out, adv)
    assert r.returncode == 0 and r.stdout.startswith("balanced: "), r.stderr[-3000:]
