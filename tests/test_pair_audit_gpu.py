"""The pair audit on the MI355X (vgpu_pair_audit; kernels/pair_audit.hip) against the host audit (vgpu_pair_audit_host, itself held to the
brute-force reference by tests/test_pair_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from
uploaded traces and from traces generated on the device; the analytic AIRs; one workgroup with the height-1 chips sliced (fib(25)), alu(50), 16
workgroups with halo, wrap and lists that run over several workgroups (fib(582)); delta sets and limits; determinism; the context still usable
afterwards; `check --pairs` on device 0; a captured AIR of 33 interactions (the interaction walk in place of the masks)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_pair_audit_cpu import ADD, COM, CPU, FIB25_SLACK, LT, MUL, SUB, Interaction, Vcol, VcolTerm, analytic_machine, analytic_traces, check_analytic

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


def audit_all(provers, w, **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device, which the
    interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.pair_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [p.pair_audit(*upload(p, mt, prep), **kw) for p in provers.values()]
    main, pre = generate(provers["basic"], w)
    reps += [p.pair_audit(main, pre, **kw) for p in provers.values()]
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
    rep = p.pair_audit([p.upload(m) for m in mt], [])
    check_analytic(rep, n)
    assert np.array_equal(rep.words, va.pair_audit_host(machine, mt, []).words)


def test_fib25_one_workgroup_and_sliced_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(25), max_entries=1 << 20)
    assert not rep.truncated and rep.total_entries == rep.reported > 0
    for chip, pairs in FIB25_SLACK.items():  # tests/test_pair_audit_cpu.py pins them against the reference
        assert rep.slack_pairs(chip) == pairs
    assert rep.chips[CPU]["height"] == 256 and rep.chips[CPU]["audited"] and rep.chips[CPU]["slack"] > 0


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50))
    assert rep.chips[CPU]["height"] == 512 and rep.chips[ADD]["slack"] == 12


def test_fib582_sixteen_workgroups(provers):
    """cpu height 4096: 16 workgroups of 256 rows, the halo rows between them and the wrap between row 0 and row n - 1; lists of up to 300
    rows run over several workgroups."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms (%.0f row evaluations), host audit %.1f ms (%.0f)" % (rep.device_ms, rep.evaluations, host.host_ms, host.evaluations))
    assert any(len(e["rows"]) == 300 and e["rows"][-1] >= 512 for e in rep.entries if e["chip"] == CPU)
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["compensated"], 300)


@pytest.mark.parametrize("kw", [dict(deltas=(1,)), dict(deltas=(2, 1, P - 1, 12345)), dict(max_entries=3)], ids=["+1", "four deltas", "3 entries"])
def test_deltas_and_limits(provers, kw):
    host, rep = audit_all(provers, va.Workload.fib(25), **kw)
    assert rep.truncated == ("max_entries" in kw)
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["compensated"], 4)


def test_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, chips=[ADD, SUB, LT, COM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [ADD, SUB, LT, COM] and not any(rep.chips[MUL]["free"])


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.pair_audit(main, pre, max_rows_per_entry=64) for _ in range(5)]
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
    rep = prover.pair_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    assert prover.bus_audit(main, pre).balanced
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("the deltas must be distinct", dict(deltas=(3, 3))), ("chip_mask names a chip", dict(chips=[20]))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.pair_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_pairs_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--pairs")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--pairs")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(line.startswith("add: 12 slack pairs of ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["pairs"], json.loads(out_host.read_text())["pairs"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}


WIDE_BUS = 33  # interactions: one more than the per-row interaction mask holds, so the device walks every interaction with both cells changed


def wide_bus_machine():
    """One captured AIR (a, b, c, m) with a + b - c = 0 and 33 interactions of count (k + 1) m: the even ones send (a + b), the odd ones
    (a, k b + c), the last one (a - b)."""
    L, u = va.lib(), ctypes.c_uint32
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    air = ctypes.c_void_p()
    assert L.vgpu_air_new(b"wide_bus", u(4), u(0), ctypes.byref(air)) == 0
    a, b, c = (L.vgpu_air_variable(air, u(0), u(k), u(0)) for k in range(3))
    L.vgpu_air_assert_zero(air, u(L.vgpu_air_sub(air, u(L.vgpu_air_add(air, u(a), u(b))), u(c))))
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for k in range(WIDE_BUS):
        count = (VcolTerm * 1)(VcolTerm(0, 3, k + 1))
        if k == WIDE_BUS - 1:
            cols = [(VcolTerm * 2)(VcolTerm(0, 0, 1), VcolTerm(0, 1, P - 1))]
        elif k % 2 == 0:
            cols = [(VcolTerm * 2)(VcolTerm(0, 0, 1), VcolTerm(0, 1, 1))]
        else:
            cols = [(VcolTerm * 1)(VcolTerm(0, 0, 1)), (VcolTerm * 2)(VcolTerm(0, 1, k), VcolTerm(0, 2, 1))]
        fields = (Vcol * len(cols))(*[Vcol(t, len(t), 0) for t in cols])
        it = Interaction(fields, len(cols), Vcol(count, 1, 0), 0, 0, 1)
        assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
    assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
    L.vgpu_air_free(air)
    return va.Machine(m)


@pytest.mark.parametrize("n", [1, 512])
def test_more_than_32_interactions_walk_the_bus(rc, n):
    """A chip of more than 32 interactions takes the device's interaction walk (pa_bus_detected) in place of the host's masks.  (a, b) at
    (+1, -1) keeps a + b, so only the records that carry a alone notice it: it is compensated exactly on the rows without records (m = 0)."""
    machine = wide_bus_machine()
    r = np.arange(n, dtype=np.uint32)
    mt = [np.stack([r + 1, 2 * r + 3, 3 * r + 4, r % 3], axis=1).astype(np.uint32)]
    host = va.pair_audit_host(machine, mt, [], max_entries=1 << 20)
    p = va.Prover(machine, rc, interpret_air=True)
    rep = p.pair_audit([p.upload(m) for m in mt], [], max_entries=1 << 20)
    assert np.array_equal(rep.words, host.words)
    assert rep.chips[0]["interactions"] == WIDE_BUS
    by = {(e["c1"], e["c2"], e["q"]): e for e in rep.entries}
    assert by[(0, 1, 1)]["compensated"] == by[(0, 1, 2)]["compensated"] == len([x for x in range(n) if x % 3 == 0])
