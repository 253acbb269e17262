"""The transition audit on the MI355X (vgpu_transition_audit; kernels/transition_audit.hip) against the host audit
(vgpu_transition_audit_host, itself held to the reference by tests/test_transition_audit_cpu.py) word for word: the basic prover and the
interpreting prover over the captured chips, from uploaded traces and from traces generated on the device; fib(1) (the height-1 chips have no
windows), fib(25) and alu(50); fib(582) (mem: many elimination slices and three levels of the merge tree, several waves per enforcement
workgroup, lists of 300 windows); the captured step AIR at the lane-word boundaries and at the widest window the device takes; the needle
traces; limits and chip mask; the w = 92 refusal with the arithmetic; determinism; argument validation; the context still proves the oracle's
proof afterwards; `check --transitions` on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import transition_audit_cases as cases
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, CPU, MEM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
FFI_CHIPS = list(range(va.NUM_CHIPS))


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def differences(rep, host):
    return ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]][:2], [g for g in zip(rep.gates, host.gates) if g[0] != g[1]][:2],
            [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:2])


def audit_all(provers, w, **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device.  All must say
    the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.transition_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].transition_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].transition_audit(*upload(provers["ffi"], mt, prep), chips=FFI_CHIPS, **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].transition_audit(main, pre, **kw), provers["ffi"].transition_audit(main, pre, chips=FFI_CHIPS, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), differences(rep, host)
        assert rep.device_ms > 0 and rep.evaluations == host.evaluations
    return host, reps[0]


def test_fib1_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(1))
    assert sum(1 for c in rep.chips if c["height"] == 1) >= 8 and all(c["audited"] for c in rep.chips)
    assert all(c["n_gates"] == 0 and c["rank"] == 0 for c in rep.chips if c["height"] == 1) and rep.reported > 0


def test_fib25(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=1 << 20, max_terms=64)
    assert not rep.truncated and rep.total_entries == rep.reported > 0 and rep.holds(w.main_traces()) == []
    # tests/test_transition_audit_cpu.py pins these against the reference
    assert (rep.chips[MEM]["transitions"], rep.chips[MEM]["gated"], rep.chips[CPU]["transitions"]) == (1, 21, 14)


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50), max_rows_per_entry=7, max_terms=32)
    assert rep.truncated and rep.reported == 1024 and rep.total_entries == 11580 and rep.chips[CPU]["height"] == 512


def test_fib582_many_slices(provers):
    """cpu height 4096, mem 16384: mem's 16383 windows are 512 elimination slices per gate (three levels of the fan-16 tree: 512 -> 32 -> 2 ->
    1), gates over the grid's y; several waves per workgroup in the enforcement pass, the halo rows between workgroups and the wrap; the count
    and list passes walk many workgroups of windows; lists of 300 windows."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert rep.chips[MEM]["height"] == 16384 and any(len(e["rows"]) == 300 and e["rows"][-1] - e["rows"][0] >= 299 for e in rep.entries if e["chip"] in (MEM, ADD, CPU))
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["free_windows"], 300)


@pytest.mark.parametrize("width", [5, 31, 32, 64, 91])
def test_step_airs(rc, width):
    """2 w + 1 = 63, 65, 129: the lane-word boundaries; 183: the widest window the device takes.  Width 5 at 8 rows: the layout."""
    n = 8 if width == 5 else cases.step_height(width)
    kw = dict(min_gate_windows=2) if width == 5 else {}
    machine, t = cases.step_machine(width), cases.step_trace(n, width)
    p = va.Prover(machine, rc, interpret_air=True)
    rep = p.transition_audit([p.upload(t)], [], max_terms=16, **kw)
    host = va.transition_audit_host(machine, [t], [], max_terms=16, **kw)
    assert np.array_equal(rep.words, host.words), differences(rep, host)
    step = [e for e in rep.entries if e["gate"] is None and e["column"] == 1 + width]
    assert [(e["l0"], e["terms"], e["free_windows"], e["held_windows"]) for e in step] == [(P - 1, [(1, P - 1), (1 + width, 1)], 0, n - 1)]


def test_a_window_too_wide_is_refused_and_the_host_answers(rc):
    width = 92
    machine, t = cases.step_machine(width), cases.step_trace(cases.step_height(width), width)
    p = va.Prover(machine, rc, interpret_air=True)
    with pytest.raises(va.VgpuError, match="transition_audit: .*2 w \\+ 1 = 185 columns, at most 184") as e:
        p.transition_audit([p.upload(t)], [])
    assert e.value.code == -1 and "chip step" in str(e.value) and "163840" in str(e.value)  # VGPU_ERR_INVALID_ARG, with the arithmetic
    host = va.transition_audit_host(machine, [t], [])  # the host audit has no limit
    assert host.chips[0]["rank"] == 184 and host.chips[0]["transitions"] == 1


@pytest.mark.parametrize("kind", ["none", "first", "last", "straddle"])
def test_needle_traces(rc, kind):
    machine = cases.free_machine(cases.NEEDLE_W)
    p = va.Prover(machine, rc, interpret_air=True)
    t = cases.needle(kind)
    rep = p.transition_audit([p.upload(t)], [])
    host = va.transition_audit_host(machine, [t], [])
    assert np.array_equal(rep.words, host.words), differences(rep, host)
    found = [e["terms"] for e in rep.entries if e["gate"] is None and e["column"] == cases.NEEDLE_F]
    assert found == ([cases.NEEDLE_TERMS] if kind == "none" else [])
    assert [(g["windows"], g["audited"]) for g in rep.gates if g["value"] == 1 and g["column"] in (5, 7)] == [(63, False), (64, True)]


def test_limits_and_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=9, max_rows_per_entry=2, max_terms=2, max_gates=7, min_gate_windows=100)
    assert rep.truncated and rep.reported == 9 and rep.total_entries > 9 and rep.chips[CPU]["gates_listed"] == 7 and rep.chips[CPU]["n_gates"] == 61
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    rep = p.transition_audit(*upload(p, mt, prep), chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["n_gates"] == 0
    assert np.array_equal(rep.words, va.transition_audit_host(p.machine, mt, prep, chips=[ADD, MEM]).words)


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.transition_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.transition_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("chip_mask names a chip", dict(chips=[20])), ("max_terms is at most 4096", dict(max_terms=5000)), ("max_gates is at most 4096", dict(max_gates=5000)),
                      ("min_gate_windows", dict(min_gate_windows=0))):
        with pytest.raises(va.VgpuError, match="transition_audit: .*" + match) as e:
            prover.transition_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_transitions_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--transitions")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--transitions")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(" transition" in line and line.startswith("cpu: ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["transitions"], json.loads(out_host.read_text())["transitions"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
