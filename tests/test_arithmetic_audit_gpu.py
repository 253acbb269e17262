"""The arithmetic audit on the MI355X (vgpu_arithmetic_audit; kernels/arithmetic_audit.hip) against the host twin (vgpu_arithmetic_audit_host,
itself held to the numpy reference by tests/test_arithmetic_audit_cpu.py) word for word: the basic prover and the interpreting prover over the
captured chips, from uploaded traces and from traces generated on the device; the planted quotient and one case per kind; the edge corpus at
every height; synthetic traces at the heights where the passes get a second workgroup and the scan a second entry per thread; the limits;
determinism; the pool's live bytes; a poisoned pool; refusals that leave the prover usable; `check --arithmetic` on device 0; the sixteen
audits back to back on one context."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import arithmetic_audit_cases as cases
import valida_amd as va
import valida_programs as vp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product", "domain", "memory", "program", "arithmetic"]


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


@pytest.fixture(scope="module")
def alus(rc):
    """The captured machines of tests/arithmetic_audit_cases.py, each with its interpreting prover."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = (cases.machine(kind), va.Prover(cases.machine(kind), rc, interpret_air=True))
        return made[kind]

    return get


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def same(rep, host):
    assert np.array_equal(rep.words, host.words), (rep.counters, host.counters, rep.hard[:3], host.hard[:3], rep.soft[:3], host.soft[:3])
    assert rep.device_ms > 0 and rep.evaluations == host.evaluations == host.counters["live"]


def audit_uploaded(provers, mt, prep, **kw):
    host = va.arithmetic_audit_host(provers["basic"].machine, mt, prep, **kw)
    for p in provers.values():
        same(p.arithmetic_audit(*upload(p, mt, prep), **kw), host)
    return host


def on_alu(alus, trace, kind="alu", **kw):
    machine, p = alus(kind)
    traces = [trace] * (2 if kind == "alu_pair" else 1)
    host = va.arithmetic_audit_host(machine, traces, [], **kw)
    same(p.arithmetic_audit([p.upload(t) for t in traces], [], **kw), host)
    return host


@pytest.mark.parametrize("name", ["fib25", "fib582", "alu100"])
def test_vm_witnesses_uploaded_and_generated_on_the_device(provers, name):
    """Uploaded traces go through an ingest copy; traces generated from the operation logs are read where they lie.  Both provers, receives and both
    sides; no hard finding."""
    w = cases.workload(name)
    mt, prep = cases.witness(name)
    basic = provers["basic"]
    log = basic.upload_oplog(w.oplog())
    main, pre = [basic.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, basic.upload(m)) for c, m in prep]
    for sides in ("receives", "both"):
        host = audit_uploaded(provers, mt, prep, sides=sides)
        assert host.total_hard == 0 and host.counters["live"] > 0
        for p in provers.values():
            same(p.arithmetic_audit(main, pre, sides=sides), host)


def test_the_planted_quotient_and_the_witnesses_with_findings(provers):
    m = provers["basic"].machine
    main, prep, cpu_row = cases.planted_quotient()
    host = audit_uploaded(provers, main, prep)
    f = host.hard[0]
    assert host.total_hard == 1 and (f["kind"], f["chip"], f["row"], f["mask"], f["expected"]) == ("wrong_result", cases.DIV, 0, 0b1000, 14)
    assert audit_uploaded(provers, main, prep, sides="both").total_hard == 2
    clean, prep, _ = cases.completed_div()
    assert audit_uploaded(provers, clean, prep, sides="both").total_hard == 0
    for name, hard, soft, sign in (("div_100_7", 1, 0, 0), ("mulhs", 0, 0, 1), ("sra", 1, 1, 0), ("mixed_ops8", 40, 8, 8)):
        host = audit_uploaded(provers, *cases.witness(name))
        assert (host.total_hard, host.total_soft, host.counters["mulhs_sign_matters"]) == (hard, soft, sign), name
    assert audit_uploaded(provers, *cases.witness("mixed_ops8"), sides="both", max_findings=5).truncated == (True, True)


def test_one_record_of_each_kind_and_reason(alus):
    rows = [cases.record(100, 0xFFFFFFFF, 1, 1), cases.record(103, 9, 0, 0), cases.record(110, 0x80000000, 0xFFFFFFFF, 0x80000000), cases.record(105, 1, 32, 0),
            cases.record(110, 0xFFFFFFF5, 2, 0xFFFFFFFA), cases.record(106, 0x80000000, 31, 0xFFFFFFFF), cases.record(114, 0xFFFFFFFE, 3, 2), cases.record(300, 1, 2, 9)]
    bad = cases.record(100, 1, 2, 3)
    bad[12], bad[1] = 256, va.P - 1
    host = on_alu(alus, cases.padded(rows + [bad]))
    assert [f["kind"] for f in host.hard] == ["wrong_result", "undefined", "undefined", "undefined", "malformed"] and [f["mask"] for f in host.hard[1:4]] == [1, 2, 3]
    assert [f["kind"] for f in host.soft] == ["shift_quotient", "arithmetic_shr"] and host.counters["mulhs_sign_matters"] == 1 and host.counters["other"] == 1


@pytest.mark.parametrize("h", cases.HEIGHTS)
def test_edge_corpus_at_height(alus, h):
    on_alu(alus, cases.edge_trace(h), max_findings=1 << 20)


def test_the_whole_corpus_on_one_and_on_two_entries(alus):
    t = cases.full_corpus_trace()
    host = on_alu(alus, t, max_findings=1 << 20)
    assert all(host.counters[k] > 0 for k in va.ARITHMETIC_KINDS + va.ARITHMETIC_REASONS)
    pair = on_alu(alus, t, "alu_pair", sides="both", max_findings=1 << 20)
    assert pair.total_hard == 2 * host.total_hard and [f["chip"] for f in pair.soft] == [0] * host.total_soft + [1] * host.total_soft
    on_alu(alus, t, "alu_pair", sides="sends")
    on_alu(alus, t, "clk")


@pytest.mark.parametrize("n", [512, 1 << 17, 1 << 20])
def test_block_boundaries(alus, n):
    """A workgroup judges 256 rows and writes one entry of each table; the scan is one workgroup of 256 threads, each taking ceil(entries / 256)
    consecutive entries, and has no further chunking.  512 is the first height with a second workgroup; up to 65536 rows a scan thread takes at
    most one entry, so 2^17 is the first power-of-two height at which every scan thread takes more than one (two); 2^20 rows once: 4096
    entries, sixteen per thread.  A wrong result is planted on the first and the last row of every workgroup; with both sides of `alu_pair` the
    second entry's workgroups follow the first's in the tables."""
    t = cases.synthetic(n)
    host = on_alu(alus, t, max_findings=300)
    assert host.counters["live"] == n and host.total_hard == host.counters["wrong_result"] == 2 * n // 256 and len(host.hard) == min(300, 2 * n // 256)
    assert [f["row"] for f in host.hard[:4]] == [0, 255, 256, 511]
    if n <= 1 << 17:
        pair = on_alu(alus, t, "alu_pair", sides="both", max_findings=1 << 20)
        assert pair.total_hard == 4 * n // 256 and pair.hard[-1]["row"] == n - 1 and pair.hard[-1]["chip"] == 1 and pair.hard[2 * n // 256]["row"] == 0


def test_limits_and_determinism(alus):
    t = cases.many_findings()
    for k in (0, 1, 299, 300, 301, 1 << 20):
        host = on_alu(alus, t, max_findings=k)
        assert (host.total_hard, host.total_soft) == (300, 300) and len(host.hard) == len(host.soft) == min(k, 300)
    machine, p = alus("alu")
    up = [p.upload(cases.synthetic(8192))]
    reps = [p.arithmetic_audit(up, [], max_findings=1000) for _ in range(2)]
    assert np.array_equal(reps[0].words, reps[1].words) and reps[0].total_hard == 64


def test_a_poisoned_pool_gives_the_hosts_words(alus, rc):
    """Every block the pool hands out and takes back is filled with a non-zero word: no pass reads scratch it has not written."""
    machine = cases.machine("alu_pair")
    p = va.Prover(machine, rc, interpret_air=True)
    p.set_pool_poison(0xA5A5A5A5)
    t = cases.full_corpus_trace()
    for kw in (dict(sides="both", max_findings=1 << 20), dict(max_findings=3), dict(sides="sends", max_findings=0)):
        same(p.arithmetic_audit([p.upload(t), p.upload(t)], [], **kw), va.arithmetic_audit_host(machine, [t, t], [], **kw))
    assert p.pool_poison_stats()[0] > 0
    p.set_pool_poison(None)


def test_context_stays_usable_after_a_pass_and_after_refusals(prover, rc, fib25, alus):
    """An audit leaves nothing behind: the pool's live bytes are what they were; a refusal returns its status and message; the next fib(25)
    proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    mt, prep = fib25.main_traces(), fib25.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.arithmetic_audit(main, pre)
    assert rep.opcodes["ADD32"] == 105 and prover.memory()[0] == live_before
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_findings is at most 2\\^20", dict(max_findings=(1 << 20) + 1)),
                      ("sides is 1 \\(receives\\), 2 \\(sends\\) or 3 \\(both\\), got 4", dict(sides=4)), ("interaction 0 of chip mem has 8 fields on global bus 2", dict(bus=2)),
                      ("no chip receives on global bus 9", dict(bus=9)), ("no chip sends or receives on local bus 5", dict(bus=(False, 5), sides="both"))):
        with pytest.raises(va.VgpuError, match="arithmetic_audit: .*" + match) as e:
            prover.arithmetic_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1
    for kind, match in (("short", "has 12 fields on global bus 0; an ALU record has at least 13"), ("tx_only", "no chip receives on global bus 0")):
        machine, p = alus(kind)
        with pytest.raises(va.VgpuError, match="arithmetic_audit: .*" + match):
            p.arithmetic_audit([p.upload(cases.edge_trace(64))], [])
    assert prover.memory()[0] == live_before and np.array_equal(prover.arithmetic_audit(main, pre).words, rep.words)
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_arithmetic_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--arithmetic", "--sides", "both")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--arithmetic", "--sides", "both")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and [line for line in r.stdout.split("\n") if line.startswith("alu: ")][-1].endswith("no finding")
    dev, host = json.loads(out.read_text())["arithmetic"], json.loads(out_host.read_text())["arithmetic"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}


def test_sixteen_audits_back_to_back_on_one_context(prover, machine, fib25):
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
        for name in AUDITS + ["arithmetic", "memory"]:  # and the arithmetic audit twice in a row, then the audit whose scan it shares
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
