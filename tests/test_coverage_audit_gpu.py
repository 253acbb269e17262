"""The coverage audit on the MI355X (vgpu_coverage_audit; kernels/coverage_audit.hip) against the host audit (vgpu_coverage_audit_host, itself
held to the brute-force reference by tests/test_coverage_audit_cpu.py) word for word: the inputs of the CPU suite under both machine kinds, from
uploaded traces and from traces generated on the device; delta sets and the max_cells cut; 16 row tiles walked by 16, 1, 3 and 5 workgroups; 64
row tiles in the default launch shape; determinism; the context still usable afterwards; `check --coverage` on device 0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valida_amd as va
import valida_programs as vp
from test_coverage_audit_cpu import BITWISE, CPU, INPUTS, LT, OUTPUT, STATIC_DATA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = va.P
FIB_DEAD = {LT: [21, 29, 30, 32, 34], BITWISE: [2, 3, 4, 23, 24, 25, 44, 45, 46, 65, 66, 67], OUTPUT: [0, 1], STATIC_DATA: [0]}  # the CPU suite pins it against the reference


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def differing(rep, host):
    return [c for c in zip(rep.chips, host.chips) if c[0] != c[1]][:2], [e for e in zip(rep.cells, host.cells) if e[0] != e[1]][:4]


def audit_all(provers, w, **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device, which the
    interpreting prover's context takes from the other context of the same device.  All must say the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.coverage_audit_host(provers["basic"].machine, mt, prep, **{k: v for k, v in kw.items() if k != "max_workgroups"})
    reps = [p.coverage_audit(*upload(p, mt, prep), **kw) for p in provers.values()]
    main, pre = generate(provers["basic"], w)
    reps += [p.coverage_audit(main, pre, **kw) for p in provers.values()]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), differing(rep, host)
        assert rep.device_ms > 0 and rep.evaluations >= host.evaluations  # (the device repeats the baselines in every column slice)
    return host, reps[0]


def dead_constraints(rep):
    return {chip: rep.dead(chip)[0] for chip in range(14) if rep.dead(chip)[0]}


@pytest.mark.parametrize("name", list(INPUTS))
def test_device_equals_host(provers, name):
    """Chips of height 1 ride along in every witness; mixed_ops:40 is a failing witness (newly failing, not non-zero)."""
    host, rep = audit_all(provers, INPUTS[name]())
    assert not rep.truncated and rep.total_cells == rep.reported > 0
    if name == "fib25":
        assert dead_constraints(rep) == FIB_DEAD and rep.chips[CPU]["free"] == [3131, 3047] and rep.total_cells == 1070
    if name == "alu50":
        assert dead_constraints(rep) == {OUTPUT: [0, 1], STATIC_DATA: [0]}


@pytest.mark.parametrize("kw", [dict(deltas=(1,)), dict(deltas=(2, 1, P - 1, 12345)), dict(max_cells=3), dict(max_cells=500)], ids=["+1", "four deltas", "3 cells", "500 cells"])
def test_deltas_and_the_cut(provers, kw):
    host, rep = audit_all(provers, va.Workload.alu(50), **kw)
    assert rep.truncated == ("max_cells" in kw) and rep.reported == min(rep.total_cells, kw.get("max_cells", 8192))


def test_fib582_workgroups_over_several_tiles(provers):
    """cpu height 4096: 16 row tiles, the halo rows between them and the wrap between row 0 and row n - 1; walked by the default number of
    workgroups and by 1, 3 and 5 (uneven shares) — the report does not depend on it."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w)
    assert dead_constraints(rep) == FIB_DEAD
    main, pre = upload(provers["basic"], w.main_traces(), w.preprocessed())
    for wgs in (1, 3, 5):
        got = provers["basic"].coverage_audit(main, pre, max_workgroups=wgs)
        assert np.array_equal(got.words, host.words), (wgs, differing(got, host))
    got = provers["ffi"].coverage_audit(main, pre, max_workgroups=3)
    assert np.array_equal(got.words, host.words), differing(got, host)


def test_largest_fib_of_cpu_height_2_14(provers):
    """64 row tiles of cpu: in the default launch shape a workgroup walks several tiles and flushes its table once."""
    w = va.Workload.fib(2338)
    assert w.cpu_height == 1 << 14 and va.Workload.fib(2339).cpu_height == 1 << 15
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.coverage_audit_host(provers["basic"].machine, mt, prep)
    main, pre = generate(provers["basic"], w)
    for p in provers.values():
        rep = p.coverage_audit(main, pre)
        assert np.array_equal(rep.words, host.words), differing(rep, host)
        print("fib(2338): device %.3f ms (%.0f row evaluations), host audit %.1f ms" % (rep.device_ms, rep.evaluations, host.host_ms))
    assert dead_constraints(host) == FIB_DEAD


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.coverage_audit(main, pre) for _ in range(5)]
        for rep in reps[1:]:
            assert np.array_equal(rep.words, reps[0].words)


def test_context_stays_usable(prover):
    """An audit leaves nothing behind: the pool's live bytes are what they were, the other audits say what they said, the next proof is the
    golden one."""
    with open(os.path.join(ROOT, "tests", "golden", "fib582_oracle.json")) as f:
        g = json.load(f)
    w = va.Workload.fib(g["n"])
    main, pre = upload(prover, w.main_traces(), w.preprocessed())
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]
    live_before = prover.memory()[0]
    mu = prover.mutation_audit(main, pre)
    rep = prover.coverage_audit(main, pre)
    assert rep.total_cells > 0 and prover.memory()[0] == live_before
    assert [c["free"] for c in rep.chips] == [c["free"] for c in mu.chips]
    assert prover.bus_audit(main, pre).balanced and np.array_equal(prover.mutation_audit(main, pre).words, mu.words)
    assert hashlib.sha256(prover.prove(main, pre).bytes()).hexdigest() == g["proof_sha256"]


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_cells", dict(max_cells=0)),
                      ("max_cells is at most", dict(max_cells=(1 << 24) + 1)), ("the deltas must be distinct", dict(deltas=(3, 3))),
                      ("a delta must be a canonical value", dict(deltas=(0,))), ("1 to 4 deltas", dict(deltas=(1, 2, 3, 4, 5)))):
        with pytest.raises(va.VgpuError, match=match) as e:
            prover.coverage_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1
    import ctypes

    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 14)(*[t._h for t in main])
    chips = (ctypes.c_uint32 * 2)(*[c for c, _ in pre])
    parr = (ctypes.c_void_p * 2)(*[t._h for _, t in pre])
    opts = va.CoverageAuditOpts(0, 0, (ctypes.c_uint32 * 4)(0, 0, 0, 0), 0, (ctypes.c_uint32 * 2)(1, 0))
    assert va.lib().vgpu_coverage_audit(prover._h, arr, 14, chips, parr, 2, ctypes.byref(opts), ctypes.byref(h)) == -1 and b"reserved" in va.lib().vgpu_last_error()
    assert va.lib().vgpu_coverage_audit(prover._h, None, 14, chips, parr, 2, None, ctypes.byref(h)) == -1 and b"null" in va.lib().vgpu_last_error()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_coverage_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--coverage")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--coverage")
    assert h.returncode == 0, h.stderr[-3000:]
    dev, host = json.loads(out.read_text())["coverage"], json.loads(out_host.read_text())["coverage"]
    from valida_amd import cli

    lines = cli.coverage_lines(va.CoverageReport.from_dict(dev))
    assert r.stdout == h.stdout and lines and r.stdout.strip().split("\n")[-len(lines):] == lines
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")  # (the device repeats the baselines in every column slice)
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
