"""The field audit on the MI355X (vgpu_field_audit; kernels/field_audit.hip) against the host audit (vgpu_field_audit_host, itself held to the
interpolating reference by tests/test_field_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips,
from uploaded traces and from traces generated on the device; fib(1) (the height-1 chips), fib(25), alu(50), mixed_ops (div, shift, mul rows),
fib(582) (many workgroups, halo, wrap, lists that run over several workgroups); the analytic AIRs with their closed forms, WIDEF beyond lanes
63 and 128; a captured AIR that does not fit the LDS is refused with a message; determinism; the context still proves the oracle's proof
afterwards; `check --fields` on device 0."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_field_audit_cpu import ADD, CPU, DIV, MEM, WIDEF, analytic_machine, analytic_traces, check_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device, which the
    interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.field_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].field_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].field_audit(*upload(provers["ffi"], mt, prep), chips=FFI_CHIPS, **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].field_audit(main, pre, **kw), provers["ffi"].field_audit(main, pre, chips=FFI_CHIPS, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations > 0
    return host, reps[0]


@pytest.fixture(scope="module")
def analytic(rc):
    machine = analytic_machine()
    return machine, va.Prover(machine, rc, interpret_air=True)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_analytic_airs(analytic, n):
    machine, p = analytic
    mt = analytic_traces(n)
    rep = p.field_audit([p.upload(m) for m in mt], [], max_rows_per_entry=8)
    check_analytic(rep, n)
    assert rep.floating(WIDEF) == {(0, 3): n}  # columns beyond lanes 63 and 128
    assert np.array_equal(rep.words, va.field_audit_host(machine, mt, [], max_rows_per_entry=8).words)


def test_fib1_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(1))
    assert sum(1 for c in rep.chips if c["height"] == 1) >= 8 and all(c["audited"] for c in rep.chips)


def test_fib25(provers):
    host, rep = audit_all(provers, va.Workload.fib(25), max_entries=1 << 20)
    assert not rep.truncated and rep.total_entries == rep.reported > 0 and rep.chips[CPU]["height"] == 256
    assert rep.floating(MEM) == {(0, j): 401 for j in range(8)}  # fib(25) has 401 memory operations


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50))
    assert rep.chips[CPU]["height"] == 512 and rep.floating(CPU) and not any(m == 4 for m, _ in rep.floating(ADD))


def test_mixed_ops(provers):
    host, rep = audit_all(provers, va.Workload.named("mixed_ops:3"), max_entries=1 << 20)
    assert rep.floating(DIV) == {(0, j): 12 for j in range(13)}  # tests/test_field_audit_cpu.py pins it against the reference


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: many workgroups, the halo rows between them and the wrap between row 0 and row n - 1; lists of up to 300
    rows run over several workgroups."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f dual row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert rep.chips[MEM]["height"] == 16384
    assert any(len(e["rows"]) == 300 and e["rows"][-1]["row"] - e["rows"][0]["row"] >= 299 for e in rep.entries if e["chip"] in (MEM, CPU))
    for e in rep.entries:
        rows = [r["row"] for r in e["rows"]]
        assert rows == sorted(set(rows)) and len(rows) == min(e["floating"], 300)


def test_limits_and_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=3, max_rows_per_entry=2)
    assert rep.truncated and rep.reported == 3
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    rep = p.field_audit(*upload(p, mt, prep), chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["live_records"] == 0
    assert np.array_equal(rep.words, va.field_audit_host(p.machine, mt, prep, chips=[ADD, MEM]).words)


def too_wide_machine():
    """One captured AIR of 200 columns (x_0 + x_199, one receive of x_0): more than the device pass's 192 columns (and its basis alone would
    not fit the LDS)."""
    from test_pair_audit_cpu import Interaction, Vcol, VcolTerm

    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    air = ctypes.c_void_p()
    assert L.vgpu_air_new(b"too_wide", u(200), u(0), ctypes.byref(air)) == 0
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_add(air, u(L.vgpu_air_variable(air, u(0), u(0), u(0))), u(L.vgpu_air_variable(air, u(0), u(199), u(0))))))
    field = (Vcol * 1)(Vcol((VcolTerm * 1)(VcolTerm(0, 0, 1)), 1, 0))
    it = Interaction(field, 1, Vcol((VcolTerm * 1)(), 0, 1), 1, 0, 0)
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
    assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
    L.vgpu_air_free(air)
    return va.Machine(m)


def test_a_chip_that_does_not_fit_the_lds_is_refused(rc):
    machine = too_wide_machine()
    mt = [np.arange(2 * 200, dtype=np.uint32).reshape(2, 200)]
    p = va.Prover(machine, rc, interpret_air=True)
    with pytest.raises(va.VgpuError, match="does not fit a workgroup's LDS") as e:
        p.field_audit([p.upload(m) for m in mt], [])
    assert e.value.code == -1 and "too_wide" in str(e.value) and "163840" in str(e.value) and "field_audit" in str(e.value)  # VGPU_ERR_INVALID_ARG, with the arithmetic
    host = va.field_audit_host(machine, mt, [])  # the host audit has no limit: x_0 is free to move with x_199
    assert host.floating(0) == {(0, 0): 2}


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.field_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.field_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("chip_mask names a chip", dict(chips=[20]))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.field_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1 and "field_audit" in str(e.value)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_fields_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--fields")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--fields")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(line.startswith("mem: interaction 0 (receives on the memory bus): fields 0-7 float on") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["fields"], json.loads(out_host.read_text())["fields"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
