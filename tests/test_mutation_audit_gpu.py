"""The mutation audit on the MI355X (vgpu_mutation_audit; kernels/mutation_audit.hip) against the host audit (vgpu_mutation_audit_host, itself
held to the brute-force reference by tests/test_mutation_audit_cpu.py) word for word: the inputs of the CPU suite under both machine kinds, from
uploaded traces and from traces generated on the device; delta sets and limits; 16 and 64 workgroups with the wrap between row 0 and row n - 1;
full size (C2) native against interpreted; the context still usable afterwards; determinism; `check --mutations` on device 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_mutation_audit_cpu import CPU, INPUTS, MUL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
FIB25_UNBOUND = [[14, 15, 17], [0], [9, 10, 11, 12, 13], [], [], list(range(8)), list(range(12)), [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11], [21, 27], [9], [72, 73, 74, 75],
                 [0, 1, 3, 4, 5, 6], [], [0, 1, 2, 3, 4]]  # tests/test_mutation_audit_cpu.py pins it against the reference


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
    host = va.mutation_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [p.mutation_audit(*upload(p, mt, prep), **kw) for p in provers.values()]
    main, pre = generate(provers["basic"], w)
    reps += [p.mutation_audit(main, pre, **kw) for p in provers.values()]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations >= host.evaluations  # (the device repeats the baselines in every column slice)
    return host, reps[0]


@pytest.mark.parametrize("name", list(INPUTS))
def test_device_equals_host(provers, name):
    """Chips of height 1 ride along in every witness; mixed_ops:40 is a failing witness (newly failing, not non-zero)."""
    host, rep = audit_all(provers, INPUTS[name]())
    assert not rep.truncated and rep.total_entries == rep.reported > 0
    if name != "mixed_ops:40":  # (whose multiplications bind mul's columns on some rows)
        assert rep.unbound_columns(MUL) == list(range(8))
    if name == "fib25":
        assert [rep.unbound_columns(c) for c in range(14)] == FIB25_UNBOUND and rep.chips[CPU]["free"] == [3131, 3047]


@pytest.mark.parametrize("kw", [dict(deltas=(1,)), dict(deltas=(2, 1, P - 1, 12345)), dict(max_entries=3), dict(max_rows_per_entry=1), dict(max_rows_per_entry=1000)],
                         ids=["+1", "four deltas", "3 entries", "1 row", "1000 rows"])
def test_deltas_and_limits(provers, kw):
    host, rep = audit_all(provers, va.Workload.alu(50), **kw)
    assert rep.truncated == ("max_entries" in kw)
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["free"], kw.get("max_rows_per_entry", 4))


def test_fib582_sixteen_workgroups(provers):
    """cpu height 4096: 16 workgroups of 256 rows, the halo rows between them and the wrap between row 0 and row n - 1."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)  # lists that run over more than one workgroup
    assert [rep.unbound_columns(c) for c in range(14)] == FIB25_UNBOUND


def test_largest_fib_of_cpu_height_2_14(provers):
    w = va.Workload.fib(2338)
    assert w.cpu_height == 1 << 14 and va.Workload.fib(2339).cpu_height == 1 << 15
    host, rep = audit_all(provers, w)
    print("fib(2338): device %.3f ms (%.0f row evaluations), host audit %.1f ms" % (rep.device_ms, rep.evaluations, host.host_ms))


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.mutation_audit(main, pre, max_rows_per_entry=64) for _ in range(5)]
        for rep in reps[1:]:
            assert np.array_equal(rep.words, reps[0].words)


def test_context_stays_usable(prover):
    """An audit leaves nothing behind: the pool's live bytes are what they were, the bus audit says what it said, the next proof is the golden one."""
    with open(os.path.join(ROOT, "tests", "golden", "fib582_oracle.json")) as f:
        g = json.load(f)
    w = va.Workload.fib(g["n"])
    main, pre = upload(prover, w.main_traces(), w.preprocessed())
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]
    live_before = prover.memory()[0]
    rep = prover.mutation_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    assert prover.bus_audit(main, pre).balanced
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]


def test_full_size_c2(provers):
    """C2 (fib(149794): 2^20 cpu rows), traces generated on the device: the native and the interpreted provers agree word for word, the unbound
    columns are fib(25)'s, every entry is consistent.  No host audit runs at this size (it would take minutes)."""
    w = va.Workload.fib(149794)
    assert w.cpu_height == 1 << 20
    main, pre = generate(provers["basic"], w)
    rep = provers["basic"].mutation_audit(main, pre)
    print("C2, generated traces: device %.3f ms, call %.3f ms, %.0f row evaluations" % (rep.device_ms, rep.host_ms, rep.evaluations))
    ffi = provers["ffi"].mutation_audit(main, pre)
    print("C2, interpreted: device %.3f ms, call %.3f ms" % (ffi.device_ms, ffi.host_ms))
    assert np.array_equal(ffi.words, rep.words)
    assert not rep.truncated and [rep.unbound_columns(c) for c in range(14)] == FIB25_UNBOUND
    for e in rep.entries:
        n = rep.chips[e["chip"]]["height"]
        assert 0 < e["free"] <= n and e["air"] + e["bus"] + e["free"] >= n and e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(4, e["free"])


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("the deltas must be distinct", dict(deltas=(3, 3))), ("a delta must be a canonical value", dict(deltas=(0,)))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.mutation_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_mutations_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--mutations")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--mutations")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(line.startswith("mul: unbound columns 0-7; ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["mutations"], json.loads(out_host.read_text())["mutations"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")  # (the device repeats the baselines in every column slice)
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
