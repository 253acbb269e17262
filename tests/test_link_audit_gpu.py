"""The link audit on the MI355X (vgpu_link_audit; kernels/link_audit.hip) against the host audit (vgpu_link_audit_host, itself held to the
reference by tests/test_link_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from uploaded
traces and from traces generated on the device; fib(1) (the height-1 chips), fib(25) (a tuple over two join workgroups), alu(50), mixed_ops
(unanswered and unbalanced tuples), fib(582) (many mask workgroups with halo and wrap, a tuple over seven join workgroups); the analytic machine
with its closed forms; cut grouping keys; determinism; the context still proves the oracle's proof afterwards; argument validation;
`check --links` on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_link_audit_cpu import CPU, DIV, MEM, MEMORY, analytic_machine, analytic_traces, bus_of, check_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def audit_all(provers, w, **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device, which the
    interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.link_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].link_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].link_audit(*upload(provers["ffi"], mt, prep), **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].link_audit(main, pre, **kw), provers["ffi"].link_audit(main, pre, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([b for b in zip(rep.buses, host.buses) if b[0] != b[1]], [c for c in zip(rep.chips, host.chips) if c[0] != c[1]],
                                                       [t for t in zip(rep.tuples, host.tuples) if t[0] != t[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations > 0
    return host, reps[0]


@pytest.fixture(scope="module")
def analytic(rc):
    machine = analytic_machine()
    return machine, va.Prover(machine, rc, interpret_air=True)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_machine(analytic, n):
    machine, p = analytic
    mt = analytic_traces(n)
    rep = p.link_audit([p.upload(m) for m in mt], [], max_tuples=1 << 10, max_records_per_tuple=16)
    check_analytic(rep, n)
    assert np.array_equal(rep.words, va.link_audit_host(machine, mt, [], max_tuples=1 << 10, max_records_per_tuple=16).words)


def test_fib1_height_one_chips(provers):
    w = va.Workload.fib(1)
    assert sum(1 for m in w.main_traces() if m.shape[0] == 1) >= 8
    audit_all(provers, w)


def test_fib25(provers):
    host, rep = audit_all(provers, va.Workload.fib(25), max_tuples=1 << 20, max_records_per_tuple=300)
    assert not rep.truncated and rep.open_tuples == rep.reported == 398
    assert max(t["n_send"] + t["n_recv"] for t in rep.tuples) == 267  # the largest tuple spans two join workgroups
    assert all(rep.open(CPU)[(3, j)] == (105, 0) for j in range(13)) and rep.open(MEM)[(0, 2)] == (401, 401)  # tests/test_link_audit_cpu.py pins them against the reference


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50))
    assert rep.open_tuples > 64 and rep.truncated and rep.reported == 64


def test_mixed_ops(provers):
    w = va.Workload.named("mixed_ops:3")
    host, rep = audit_all(provers, w, max_tuples=1 << 20)
    assert rep.open(DIV) == {(0, j): (12, 12) for j in range(13)}
    bus = provers["basic"].bus_audit(*upload(provers["basic"], w.main_traces(), w.preprocessed()))
    assert not bus.balanced  # the audit ignores net: it runs on unbalanced witnesses alike


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: many mask workgroups, the halo rows between them and the wrap between row 0 and row n - 1; 31 766 live
    records, the largest tuple over seven join workgroups."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_tuples=1 << 20, max_records_per_tuple=2)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f dual row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert sum(b["live"] for b in rep.buses) == 31766
    assert any(t["n_send"] + t["n_recv"] > 256 for t in rep.tuples) and max(t["n_send"] + t["n_recv"] for t in rep.tuples) == 1660
    firsts = [t["records"][0][:3] for t in rep.tuples]
    assert firsts == sorted(firsts) and bus_of(rep, MEMORY)["open_tuples"] == bus_of(rep, MEMORY)["tuples"]


def test_hash_bits_do_not_change_the_report(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    main, pre = upload(p, mt, prep)
    want = p.link_audit(main, pre).words
    assert np.array_equal(want, va.link_audit_host(p.machine, mt, prep).words)
    for bits in (8, 16):
        assert np.array_equal(p.link_audit(main, pre, hash_bits=bits).words, want)


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.link_audit(main, pre, max_tuples=256) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.link_audit(main, pre)
    assert rep.open_tuples > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_tuples", dict(max_tuples=0)),
                      ("hash_bits", dict(hash_bits=65))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.link_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1 and "link_audit" in str(e.value)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_links_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--links")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--links")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(line.startswith("mem: interaction 0 (receives on the memory bus): fields") and " open on " in line for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["links"], json.loads(out_host.read_text())["links"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
