"""The domain audit on the MI355X (vgpu_domain_audit; kernels/domain_audit.hip) against the host audit (vgpu_domain_audit_host, itself held to
the reference by tests/test_domain_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from
uploaded traces and from traces generated on the device; fib(25), alu(50), fib(582); the needle with and without the break; every edge trace
and all 65536 narrow values; the heights around the first second slice and around the cap of 2048 slices; limits, chip mask, explicit lookup
buses; determinism; the pool's live bytes; refusals that leave the prover usable; `check --domains` on device 0; the thirteen audits back to
back on one context."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import domain_audit_cases as cases
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, MEM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product", "domain"]


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
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device (no ingest copy).
    All must say the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.domain_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].domain_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].domain_audit(*upload(provers["ffi"], mt, prep), **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].domain_audit(main, pre, **kw), provers["ffi"].domain_audit(main, pre, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4],
                                                       [(c, k) for c in range(va.NUM_CHIPS) for k in zip(rep.columns(c), host.columns(c)) if k[0] != k[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations == host.evaluations > 0
    return host, reps[0]


def test_fib25(provers):
    host, rep = audit_all(provers, va.Workload.fib(25), max_entries=1 << 20)
    assert rep.lookup_buses() == [(True, 2), (True, 3)] and rep.unguarded(ADD) == [2, 3, 6, 7]  # tests/test_domain_audit_cpu.py pins these against the reference
    assert [k["guarded_rows"] for k in rep.columns(ADD)[11:15]] == [105] * 4


def test_alu50(provers):
    audit_all(provers, va.Workload.alu(50), max_rows_per_entry=7)


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: 16 and 64 slices per virtual column merging through the bitmaps, as many guard workgroups; lists of 300 rows
    run over several workgroups and over the waves of a workgroup."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f cells)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert any(len(e["rows"]) == 300 and e["rows"][-1][0] - e["rows"][0][0] >= 299 for e in rep.entries)
    for e in rep.entries:
        rows = [r for r, _ in e["rows"]]
        assert rows == sorted(set(rows)) and len(rows) == min(e["unguarded_nonzero_rows"], 300)


def test_needle(rc):
    machine = cases.needle_machine()
    p = va.Prover(machine, rc, interpret_air=True)
    for broken in (False, True):
        t = cases.needle_traces(broken)
        for chips in (None, [0]):
            rep = p.domain_audit([p.upload(m) for m in t], [], chips=chips)
            assert np.array_equal(rep.words, va.domain_audit_host(machine, t, [], chips=chips).words), (broken, chips)
        assert rep.total_entries == (1 if broken else 0) and [e["rows"] for e in rep.entries] == ([[(511, 1 + 511 % 255)]] if broken else [])


@pytest.fixture(scope="module")
def edge(rc):
    machine = cases.edge_machine()
    return machine, va.Prover(machine, rc, interpret_air=True)


def test_edge_shapes(edge):
    machine, p = edge
    for name, t in cases.edge_traces():
        rep = p.domain_audit([p.upload(t)], [], max_rows_per_entry=7)
        assert np.array_equal(rep.words, va.domain_audit_host(machine, [t], [], max_rows_per_entry=7).words), name


def test_all_narrow_values(edge):
    machine, p = edge
    t = cases.all_narrow_values()
    rep = p.domain_audit([p.upload(t)], [])
    assert np.array_equal(rep.words, va.domain_audit_host(machine, [t], []).words)
    k = rep.columns(0)[0]
    assert (k["distinct_narrow"], k["dense"], k["cls"]) == (65536, True, "half")


@pytest.mark.parametrize("n", [256, 512, 1024, 1 << 19, 1 << 20])
def test_slice_boundaries(edge, n):
    """A virtual column gets a second slice at 512 rows (two tiles of 256); 256 is one tile below, and the next heights a machine admits are
    powers of two: 1024.  2^19 rows are the last height with one tile per slice (2048 slices), 2^20 the first with two."""
    machine, p = edge
    r = np.arange(n, dtype=np.uint64)
    t = np.stack([(r * 2654435761 >> 7) % 70000, (r % 5 != 0).astype(np.uint64), r], axis=1).astype(np.uint32)
    t[n - 1, 0] = 65535
    rep = p.domain_audit([p.upload(t)], [], max_rows_per_entry=3)
    assert np.array_equal(rep.words, va.domain_audit_host(machine, [t], [], max_rows_per_entry=3).words)
    assert rep.columns(0)[0]["wide_rows"] > 0 and 0 not in rep.unguarded(0)  # a wide column is no entry


def test_limits_chip_mask_and_lookup_buses(provers):
    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    main, pre = upload(p, mt, prep)
    for kw in (dict(max_entries=0), dict(max_entries=3, max_rows_per_entry=1), dict(max_rows_per_entry=0), dict(chips=[ADD, MEM]), dict(max_bits=8), dict(lookup_buses=[3]),
               dict(lookup_buses=[])):
        rep = p.domain_audit(main, pre, **kw)
        assert np.array_equal(rep.words, va.domain_audit_host(p.machine, mt, prep, **kw).words), kw
    assert p.domain_audit(main, pre, max_entries=0).total_entries > 0


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.domain_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable_after_a_pass_and_after_refusals(prover, rc, fib25):
    """An audit leaves nothing behind: the pool's live bytes are what they were; a refusal returns its status and message; the next fib(25)
    proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    mt, prep = fib25.main_traces(), fib25.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.domain_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_bits is at most 16", dict(max_bits=17)),
                      ("chip_mask names a chip", dict(chips=[20])), ("max_entries is at most 2\\^24", dict(max_entries=(1 << 24) + 1))):
        with pytest.raises(va.VgpuError, match="domain_audit: .*" + match) as e:
            prover.domain_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1
    wide = cases.needle_machine(bus=64)
    pw = va.Prover(wide, rc, interpret_air=True)
    t = cases.needle_traces(True)
    with pytest.raises(va.VgpuError, match="domain_audit: bus index 64 of chip user does not fit the 64-bit lookup masks") as e:
        pw.domain_audit([pw.upload(m) for m in t], [], lookup_buses=[3])
    assert e.value.code == -1 and pw.domain_audit([pw.upload(m) for m in t], [], chips=[0]).total_entries == 1
    assert prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_domains_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--domains")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--domains")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(" narrow column" in line and line.startswith("cpu: ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["domains"], json.loads(out_host.read_text())["domains"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}


def test_thirteen_audits_back_to_back_on_one_context(prover, machine, fib25):
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
        for name in AUDITS + ["domain", "rank"]:  # and the domain audit twice in a row, then the audit whose scan kernel it shares
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
    from oracle import pyoracle as po  # checker only

    assert proof_before == po.prove_basic(mt, prep[0][1], prep[1][1], va.poseidon_round_constants()).bytes()  # the oracle's proof of fib(25)
