"""The constraint audit on the MI355X (vgpu_constraint_audit; kernels/constraint_audit.hip) against the host audit (vgpu_constraint_audit_host,
itself held to the independent reference by tests/test_constraint_audit_cpu.py) word for word: every input of the issue's tables under both
machine kinds, from uploaded traces and from traces generated on the device; truncation; full size (C2) clean and with faults, with the Python
reference on row windows; the context still usable afterwards (bus audit, golden proof); determinism; `check --constraints` on device 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_audit_ref as ref
import valida_amd as va
import valida_programs as vp
from test_constraint_audit_cpu import ADD, CLEAN, CPU, FAILING, FAULTS, LT, N_CONSTRAINTS, every_50th, exe, witness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
GENERAL, MEMORY, RANGE = (1, 0), (1, 2), (1, 3)
C2_FAULTS = ((CPU, 777777, 1), (ADD, 12345, 11), (LT, 0, 0))


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def audit_all(provers, w, faults=(), **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and (unfaulted witnesses) traces generated on the device,
    which the interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = witness(w, faults)
    host = va.constraint_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [p.constraint_audit(*upload(p, mt, prep), **kw) for p in provers.values()]
    if not faults:
        main, pre = generate(provers["basic"], w)
        reps += [p.constraint_audit(main, pre, **kw) for p in provers.values()]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), (rep.constraints, host.constraints)
        assert rep.device_ms > 0
    return host, reps[0]


@pytest.mark.parametrize("name", list(CLEAN))
def test_clean_witnesses(provers, name):
    host, rep = audit_all(provers, CLEAN[name]())
    assert rep.satisfied and rep.total_failing == 0 and rep.constraints == [] and [c["constraints"] for c in rep.chips] == N_CONSTRAINTS


@pytest.mark.parametrize("name", list(FAILING))
def test_failing_witnesses(provers, name):
    host, rep = audit_all(provers, FAILING[name]())
    assert rep.total_failing == {"mixed_ops:40": 13, "echo3": 7}[name] and not rep.satisfied
    if name == "mixed_ops:40":
        assert [(e["chip"], e["constraint"], e["failing_rows"]) for e in rep.constraints][:5] == [(CPU, 32, 41), (CPU, 33, 41), (CPU, 35, 41), (CPU, 42, 41), (5, 0, 235)]
        assert rep.constraints[0]["rows"][:2] == [(21, 2013261825), (41, 2013261825)]
        print("mixed_ops:40 device %.3f ms, call %.3f ms" % (rep.device_ms, rep.host_ms))


@pytest.mark.parametrize("fault,failures", FAULTS)
def test_single_cell_faults(provers, fib25, fault, failures):
    host, rep = audit_all(provers, fib25, [fault])
    assert [(e["chip"], e["constraint"], e["rows"]) for e in rep.constraints] == failures


def test_truncation(provers):
    w = FAILING["mixed_ops:40"]()
    host, rep = audit_all(provers, w, max_constraints=3)
    assert rep.truncated and rep.total_failing == 13 and rep.reported == 3
    host, one = audit_all(provers, w, max_rows_per_constraint=1)
    host, every = audit_all(provers, w, max_rows_per_constraint=1000)
    for a, b in zip(one.constraints, every.constraints):
        assert a["failing_rows"] == b["failing_rows"] == len(b["rows"]) and a["rows"] == b["rows"][:1] and [r for r, _ in b["rows"]] == sorted(r for r, _ in b["rows"])
    big = va.Workload.named("mixed_ops:700")  # thousands of failing rows
    host, rep = audit_all(provers, big, max_rows_per_constraint=100)
    assert sum(c["failing_rows"] for c in rep.chips) > 2000
    print("mixed_ops:700 (%d failing rows) device %.3f ms, call %.3f ms" % (sum(c["failing_rows"] for c in rep.chips), rep.device_ms, rep.host_ms))


def test_full_size_c2(provers):
    """C2 (fib(149794): 2^20 cpu rows) clean, from generated traces under both machine kinds; then the three faults of the issue in uploaded matrices:
    device == host audit word for word, and the Python reference agrees row by row on the rows within 2 of each fault and on 4096 random rows.  The
    bus audit on the same prover afterwards still gives its known answer."""
    w = va.Workload.fib(149794)
    assert w.cpu_height == 1 << 20
    p = provers["basic"]
    main, pre = generate(p, w)
    rep = p.constraint_audit(main, pre)
    assert rep.satisfied and [c["constraints"] for c in rep.chips] == N_CONSTRAINTS and rep.chips[CPU]["height"] == 1 << 20
    print("C2 clean, generated traces: device %.3f ms, call %.3f ms" % (rep.device_ms, rep.host_ms))
    ffi = provers["ffi"].constraint_audit(main, pre)
    assert np.array_equal(ffi.words, rep.words)
    print("C2 clean, interpreted: device %.3f ms, call %.3f ms" % (ffi.device_ms, ffi.host_ms))
    bus = p.bus_audit(main, pre)
    assert bus.balanced and {b["bus"]: b["live"] for b in bus.buses} == {GENERAL: 1198362, MEMORY: 4493872, RANGE: 2396980}
    del main, pre
    mt, prep = witness(w)
    clean_host = va.constraint_audit_host(p.machine, mt, prep)
    assert np.array_equal(clean_host.words, rep.words)
    print("C2 clean, host audit: %.1f ms" % clean_host.host_ms)
    for chip, row, col in C2_FAULTS:
        mt[chip][row, col] = (int(mt[chip][row, col]) + 1) % P
    host = va.constraint_audit_host(p.machine, mt, prep, max_rows_per_constraint=1000)
    assert not host.satisfied and {e["chip"] for e in host.constraints} == {CPU, ADD, LT}
    for q in provers.values():
        dev = q.constraint_audit(*upload(q, mt, prep), max_rows_per_constraint=1000)
        assert np.array_equal(dev.words, host.words), (dev.constraints, host.constraints)
    print("C2 faulted, uploaded traces: device %.3f ms, call %.3f ms" % (dev.device_ms, dev.host_ms))
    # the reference, row by row: every failing row is listed (1000 > the few rows that fail), so a sampled row's listed values are all its failures
    listed = {}
    for e in dev.constraints:
        assert e["failing_rows"] == len(e["rows"])
        for row, value in e["rows"]:
            listed.setdefault((e["chip"], row), {})[e["constraint"]] = value
    rng = np.random.default_rng(20261017)
    sample = {chip: set() for chip in (CPU, ADD, LT)}
    for chip, row, _ in C2_FAULTS:
        sample[chip] |= {(row + d) % mt[chip].shape[0] for d in (-2, -1, 0, 1, 2)}
    for chip, count in ((CPU, 2048), (ADD, 1024), (LT, 1024)):
        sample[chip] |= set(int(r) for r in rng.integers(0, mt[chip].shape[0], count))
    prep_of = dict(prep)
    seen_failing = 0
    for chip, rows in sample.items():
        for r, v in ref.chip_rows(chip, mt[chip], prep_of.get(chip), sorted(rows)).items():
            bad = {int(k): int(v[k]) for k in np.nonzero(v)[0]}
            assert bad == listed.get((chip, r), {}), (chip, r)
            seen_failing += bool(bad)
    assert seen_failing >= 3


def test_context_stays_usable(prover):
    """An audit leaves nothing behind: the pool's live bytes are what they were, the bus audit says what it said, the next proof is the golden one."""
    with open(os.path.join(ROOT, "tests", "golden", "fib582_oracle.json")) as f:
        g = json.load(f)
    w = va.Workload.fib(g["n"])
    mt, prep = witness(w)
    main, pre = upload(prover, mt, prep)
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]
    live_before = prover.memory()[0]
    assert prover.constraint_audit(main, pre).satisfied and prover.memory()[0] == live_before
    bad = prover.upload(np.where(np.arange(mt[ADD].size).reshape(mt[ADD].shape) == 11, (mt[ADD].astype(np.uint64) + 1) % P, mt[ADD]).astype(np.uint32))
    rep = prover.constraint_audit(main[:ADD] + [bad] + main[ADD + 1:], pre)
    assert not rep.satisfied and {e["chip"] for e in rep.constraints} == {ADD}
    del bad
    assert prover.memory()[0] == live_before
    assert prover.bus_audit(main, pre).balanced
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]


def test_determinism(provers):
    """pc corrupted on every 50th row of a 2^18-row cpu trace (thousands of failing rows spread over all 1024 workgroups), audited five times:
    identical word images, listed rows ascending, equal to the host audit's."""
    mt, prep = every_50th(va.Workload.fib(37446), 1 << 18)
    host = va.constraint_audit_host(provers["basic"].machine, mt, prep, max_rows_per_constraint=64)
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.constraint_audit(main, pre, max_rows_per_constraint=64) for _ in range(5)]
        for rep in reps:
            assert np.array_equal(rep.words, host.words)
            for e in rep.constraints:
                assert [r for r, _ in e["rows"]] == sorted(set(r for r, _ in e["rows"])) and len(e["rows"]) == min(64, e["failing_rows"])
        assert max(e["failing_rows"] for e in reps[0].constraints) > 1000


def test_device_argument_validation(prover, fib25):
    mt, prep = witness(fib25)
    main, pre = upload(prover, mt, prep)
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])),
                      ("has no preprocessed columns", dict(pre=pre + [(ADD, main[ADD])])), ("max_constraints", dict(max_constraints=0))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.constraint_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_constraints_on_the_device(tmp_path):
    echo, loop, adv3, adv, out = tmp_path / "echo.bin", tmp_path / "loop.bin", tmp_path / "abc", tmp_path / "advice", tmp_path / "report.json"
    echo.write_bytes(vp.machine_code(vp.echo_program(3)))
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv3.write_bytes(b"abc")
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", echo, out, adv3, "--device", 0, "--constraints")
    assert r.returncode == 1, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 15 and lines[6].startswith("unbalanced: 6 tuples") and lines[7].startswith("cpu constraint 32 fails on 3 rows: row 1 = ")
    assert lines[11] == "output constraint 0 fails on 1 rows: row 2 = 5" and lines[14].startswith("violated: 7 constraints of 2 chips")
    j = json.loads(out.read_text())
    assert j["constraints"]["total_failing"] == 7 and j["constraints"]["device_ms"] > 0 and j["device_ms"] > 0
    r = _cli("check", loop, out, adv, "--constraints")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("balanced: ") and lines[1].startswith("satisfied: ") and json.loads(out.read_text())["constraints"]["satisfied"]
