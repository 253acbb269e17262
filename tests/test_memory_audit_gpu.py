"""The memory audit on the MI355X (vgpu_memory_audit; kernels/memory_audit.hip) against the host audit (vgpu_memory_audit_host, itself held to
the numpy reference by tests/test_memory_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from
uploaded traces and from traces generated on the device; the VM's witnesses, fib(582); fib(25) tampered; every edge trace, planted stale read,
static and extreme trace of tests/memory_audit_cases.py; synthetic traces at the heights where the max-scan and the sort's digit table get a
second block; the limits; determinism; the pool's live bytes; refusals that leave the prover usable; `check --memory` on device 0; the fourteen
audits back to back on one context."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import memory_audit_cases as cases
import valida_amd as va
import valida_programs as vp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product", "domain", "memory"]


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


@pytest.fixture(scope="module")
def ram(rc):
    machine = cases.ram_machine()
    return machine, va.Prover(machine, rc, interpret_air=True)


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def same(rep, host):
    assert np.array_equal(rep.words, host.words), (rep.counters, host.counters, rep.findings[:3], host.findings[:3])
    assert rep.device_ms > 0 and rep.evaluations == host.evaluations


def audit_uploaded(provers, mt, prep, **kw):
    host = va.memory_audit_host(provers["basic"].machine, mt, prep, **kw)
    for p in provers.values():
        same(p.memory_audit(*upload(p, mt, prep), **kw), host)
    return host


def on_ram(ram, t, **kw):
    machine, p = ram
    host = va.memory_audit_host(machine, [t], [], **kw)
    same(p.memory_audit([p.upload(t)], [], **kw), host)
    return host


@pytest.mark.parametrize("name", ["fib25", "alu50", "left_imm_ops", "signed_inequality", "loadfp", "mixed_ops20", "static_data", "byte_loads", "store_byte"])
def test_vm_witnesses_uploaded(provers, name):
    host = audit_uploaded(provers, *cases.witness(name))
    assert host.total_findings == 0


@pytest.mark.parametrize("name,workload", [("fib25", lambda: va.Workload.fib(25)), ("fib582", lambda: va.Workload.fib(582))])
def test_traces_generated_on_the_device(provers, name, workload):
    """No ingest copy: the audit reads the generated traces where they lie.  fib(582): mem at 16384 rows, 8756 live: 64 key workgroups, five scan
    blocks, three sort blocks."""
    w = workload()
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.memory_audit_host(provers["basic"].machine, mt, prep)
    basic = provers["basic"]
    log = basic.upload_oplog(w.oplog())
    main, pre = [basic.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, basic.upload(m)) for c, m in prep]
    for p in provers.values():
        same(p.memory_audit(main, pre), host)
    same(provers["basic"].memory_audit(*upload(provers["basic"], mt, prep)), host)
    assert host.total_findings == 0 and host.counters["live"] == (401 if name == "fib25" else 8756)


@pytest.mark.parametrize("kind", ["read", "write", "uninit"])
def test_tampered_fib25(provers, kind):
    mt, prep, row = cases.tampered(kind)
    host = audit_uploaded(provers, mt, prep)
    assert host.total_findings >= 1 and (host.findings[0]["row"] == row) == (kind != "write")


def test_edge_static_and_extreme_traces(ram):
    for name, t in cases.edge_traces() + cases.static_traces() + cases.extreme_traces() + [("same_cycle_%d" % k, cases.same_cycle(bool(k))) for k in (0, 1)]:
        on_ram(ram, t)


def test_planted_stale_reads(ram):
    for position in cases.PLANT_POSITIONS:
        host = on_ram(ram, cases.planted(position))
        assert [(f["kind"], f["row"]) for f in host.findings] == [("stale_read", position)]


def test_a_run_of_3000_reads_and_a_row_permutation(ram):
    t, row = cases.long_run()
    assert [(f["kind"], f["row"]) for f in on_ram(ram, t).findings] == [("stale_read", row)]
    on_ram(ram, cases.permuted(t)[0])


def test_two_receives_of_one_row(rc):
    machine = cases.ram2_machine()
    p = va.Prover(machine, rc, interpret_air=True)
    t = cases.two_receive_trace()
    same(p.memory_audit([p.upload(t)], []), va.memory_audit_host(machine, [t], []))


@pytest.mark.parametrize("n", [4096, 8192, 32768, 1 << 20])
def test_block_boundaries(ram, n):
    """Every row live.  4096 records are the first height with a second block of the max-scan's first level (MM_SCAN_BLOCK = 2048 records), 8192
    the first with a second block of the radix sort (4096 pairs), 32768 the first at which a thread of the sort's digit-table scan takes a second
    entry (256 digits x 8 blocks over 1024 threads), 2^20 the first at which a thread of the max-scan's second level takes a second block maximum
    (512 blocks over 256 threads).  A tampered read of an address nobody has written yet is an uninitialised read."""
    host = on_ram(ram, cases.synthetic(n), max_findings=300)
    assert host.counters["live"] == n and host.total_findings == host.counters["stale_read"] + host.counters["uninit_read"] and host.counters["stale_read"] > 0 and host.counters["layout_descents"] > 0


def test_limits_and_determinism(ram):
    t = cases.many_findings()
    for k in (0, 1, 64, 300, 1 << 20):
        host = on_ram(ram, t, max_findings=k)
        assert host.total_findings == 300 and len(host.findings) == min(k, 300)
    machine, p = ram
    main = [p.upload(cases.synthetic(8192))]
    reps = [p.memory_audit(main, [], max_findings=1000) for _ in range(2)]
    assert np.array_equal(reps[0].words, reps[1].words) and reps[0].total_findings > 0


def test_context_stays_usable_after_a_pass_and_after_refusals(prover, rc, fib25):
    """An audit leaves nothing behind: the pool's live bytes are what they were; a refusal returns its status and message; the next fib(25)
    proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    mt, prep = fib25.main_traces(), fib25.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.memory_audit(main, pre)
    assert rep.counters["live"] == 401 and prover.memory()[0] == live_before
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_findings is at most 2\\^20", dict(max_findings=(1 << 20) + 1)),
                      ("no chip receives on global bus 7", dict(bus=7)), ("no chip receives on local bus 2", dict(bus=(False, 2)))):
        with pytest.raises(va.VgpuError, match="memory_audit: .*" + match) as e:
            prover.memory_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1
    t = cases.same_cycle(True)
    for machine, match in ((cases.ram_machine(fields=7), "receives 7 fields on global bus 2"), (cases.no_receive_machine(), "no chip receives on global bus 2")):
        p = va.Prover(machine, rc, interpret_air=True)
        with pytest.raises(va.VgpuError, match="memory_audit: .*" + match) as e:
            p.memory_audit([p.upload(t)], [])
        assert e.value.code == -1
    assert prover.memory()[0] == live_before and prover.memory_audit(main, pre).counters == rep.counters
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_memory_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--memory")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--memory")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and [line for line in r.stdout.split("\n") if line.startswith("mem: ")][-1].endswith("no finding")
    dev, host = json.loads(out.read_text())["memory"], json.loads(out_host.read_text())["memory"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}


def test_fourteen_audits_back_to_back_on_one_context(prover, machine, fib25):
    """From traces generated on the device and again from the same matrices uploaded, every report word for word the host audit's; the pool's
    live bytes afterwards are what they were and the next proof is byte for byte the proof made before them."""
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    host = {name: getattr(va, name + "_audit_host")(machine, mt, prep) for name in AUDITS}
    pre = [(c, prover.upload(m)) for c, m in prep]
    proof_before = prover.prove([prover.upload(m) for m in mt], pre).bytes()
    log = prover.upload_oplog(fib25.oplog())
    generated = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
    uploaded = [prover.upload(t.download()) for t in generated]
    live_before = prover.memory()[0]
    for main in (generated, uploaded):
        for name in AUDITS + ["memory", "bus"]:  # and the memory audit twice in a row, then the audit whose sort it shares
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
