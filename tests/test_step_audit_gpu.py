"""The step audit on the MI355X (vgpu_step_audit; kernels/step_audit.hip) against the host audit (vgpu_step_audit_host, itself held to the
reference by tests/test_step_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from uploaded
traces and from traces generated on the device; the analytic AIRs with their closed forms (WIDE: more than 64 items, columns beyond lane 63);
fib(1) (the height-1 chips), fib(25) with the pinned columns, alu(50), fib(582) (NW = 2 / 4, halo, wrap, lists over several workgroups); one
step and four steps; limits and chip mask; a captured AIR that does not fit the LDS is refused with the arithmetic; determinism; the context
still proves the oracle's proof afterwards; argument validation; `check --steps` on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, CPU, MEM, WIDE, analytic_machine, analytic_traces
from test_rank_audit_gpu import too_wide_machine
from test_step_audit_cpu import FIB25_CONFIRMED, FIB25_REFUTED, check_step_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
FFI_CHIPS = list(range(va.NUM_CHIPS))  # every BasicMachine chip fits the LDS under the interpreting prover too


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
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device.  All must say
    the same words; the device's bus word is 0 and so is the host's count (the theorem of the contract)."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.step_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].step_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].step_audit(*upload(provers["ffi"], mt, prep), chips=FFI_CHIPS, **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].step_audit(main, pre, **kw), provers["ffi"].step_audit(main, pre, chips=FFI_CHIPS, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations > 0
    assert all(c["bus"] == 0 for c in host.chips)
    return host, reps[0]


@pytest.fixture(scope="module")
def analytic(rc):
    machine = analytic_machine()
    return machine, va.Prover(machine, rc, interpret_air=True)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(analytic, n):
    machine, p = analytic
    mt = analytic_traces(n)
    rep = p.step_audit([p.upload(m) for m in mt], [], max_rows_per_entry=8)
    check_step_analytic(rep, n)
    assert rep.confirmed_columns(WIDE) == [0, 35, 69] and all(c["line_exact"] for c in rep.chips)
    assert np.array_equal(rep.words, va.step_audit_host(machine, mt, [], max_rows_per_entry=8).words)


def test_fib1_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(1))
    assert sum(1 for c in rep.chips if c["height"] == 1) >= 8 and all(c["audited"] for c in rep.chips)


def test_fib25(provers):
    host, rep = audit_all(provers, va.Workload.fib(25), max_entries=1 << 20)
    assert not rep.truncated and rep.total_entries == rep.reported > 0
    for chip in range(va.NUM_CHIPS):  # tests/test_step_audit_cpu.py pins them against the reference
        assert rep.confirmed_columns(chip) == FIB25_CONFIRMED[chip] and rep.refuted_columns(chip) == FIB25_REFUTED.get(chip, [])
    assert rep.chips[CPU]["height"] == 256


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50))
    assert rep.chips[CPU]["height"] == 512 and len(rep.confirmed_columns(ADD)) == 12


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: several waves per workgroup, many workgroups, the halo rows between them and the wrap between row 0 and
    row n - 1; lists of up to 300 rows run over several workgroups."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert any(len(e["rows"]) == 300 and e["rows"][-1]["row"] - e["rows"][0]["row"] >= 299 for e in rep.entries if e["chip"] in (MEM, ADD, CPU))
    for e in rep.entries:
        rows = [r["row"] for r in e["rows"]]
        assert rows == sorted(set(rows)) and len(rows) == min(e["coupled_exact"] + e["curved"], 300)


def test_one_step_and_four_steps(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, steps=[1])
    assert rep.steps == [1] and not rep.chips[ADD]["line_exact"] and rep.chips[MEM]["line_exact"]
    host, rep = audit_all(provers, w, steps=[1, P - 1, 2, P - 2])
    assert rep.steps == [1, P - 1, 2, P - 2] and rep.chips[ADD]["line_exact"]


def test_limits_and_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=3, max_rows_per_entry=2)
    assert rep.truncated and rep.reported == 3
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    rep = p.step_audit(*upload(p, mt, prep), chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["loose_cells"] == 0
    assert np.array_equal(rep.words, va.step_audit_host(p.machine, mt, prep, chips=[ADD, MEM]).words)


def test_a_chip_that_does_not_fit_the_lds_is_refused(rc):
    machine = too_wide_machine()
    mt = [np.arange(2 * 200, dtype=np.uint32).reshape(2, 200)]
    p = va.Prover(machine, rc, interpret_air=True)
    with pytest.raises(va.VgpuError, match="step_audit: .*does not fit a workgroup's LDS") as e:
        p.step_audit([p.upload(m) for m in mt], [])
    assert e.value.code == -1 and "too_wide" in str(e.value) and "163840" in str(e.value)  # VGPU_ERR_INVALID_ARG, with the arithmetic
    host = va.step_audit_host(machine, mt, [])  # the host audit has no limit
    assert host.confirmed_columns(0) == [0, 199] and host.chips[0]["exact_cells"] == 2 * 200


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.step_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.step_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("chip_mask names a chip", dict(chips=[20])), ("distinct", dict(steps=[2, 2])), ("1..p-1", dict(steps=[0]))):
        with pytest.raises(va.VgpuError, match="step_audit: .*" + match) as e:
            prover.step_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_steps_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--steps")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--steps")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(line.startswith("add: confirmed columns 0-7, 11-14 on") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["steps"], json.loads(out_host.read_text())["steps"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
