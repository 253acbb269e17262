"""The product audit on the MI355X (vgpu_product_audit; kernels/product_audit.hip) against the host audit (vgpu_product_audit_host, itself held
to the reference by tests/test_product_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips, from
uploaded traces and from traces generated on the device; fib(1) (the height-1 chips), fib(25) and alu(50) with the pinned facts, fib(582)
(many workgroups in every phase, lists of 300 rows); the captured quad AIRs (n = 1, 2, 8 and the lane-word boundary) and the three needle traces
at 4096 rows (128 slices of basis rows whose lists the merge tree orders); limits and chip mask; a captured AIR that does not fit is refused
with the arithmetic; determinism; argument validation; the context still proves the oracle's proof afterwards; `check --products` on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import product_audit_cases as cases
import valida_amd as va
import valida_programs as vp
from test_rank_audit_cpu import ADD, BITWISE, CPU, MEM
from test_rank_audit_gpu import too_wide_machine

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


def audit_all(provers, w, **kw):
    """The host audit's report and the device's: uploaded traces under both machine kinds and traces generated on the device.  All must say
    the same words."""
    mt, prep = w.main_traces(), w.preprocessed()
    host = va.product_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].product_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].product_audit(*upload(provers["ffi"], mt, prep), chips=FFI_CHIPS, **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].product_audit(main, pre, **kw), provers["ffi"].product_audit(main, pre, chips=FFI_CHIPS, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations == host.evaluations > 0
    return host, reps[0]


def counts(c):
    return (c["rank"], c["pairs"], c["relations"], c["boolean"], c["zero"])


def test_fib1_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(1))
    assert sum(1 for c in rep.chips if c["height"] == 1) >= 8 and all(c["audited"] for c in rep.chips)
    assert all((c["rank"], c["independent"], c["pairs"], c["relations"]) == (1, 0, 0, 0) for c in rep.chips if c["height"] == 1)
    assert rep.chips[CPU]["relations"] > 0


def test_fib25(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=1 << 20, max_terms=32)
    assert not rep.truncated and rep.total_entries == rep.reported > 0 and rep.holds(w.main_traces()) == []
    # tests/test_product_audit_cpu.py pins these against the reference
    assert counts(rep.chips[CPU]) == (29, 406, 213, 10, 65) and counts(rep.chips[MEM]) == (9, 36, 4, 3, 1) and counts(rep.chips[ADD]) == (10, 45, 29, 5, 7)


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50), max_entries=1 << 20, max_rows_per_entry=7, max_terms=32)
    assert counts(rep.chips[CPU])[2:] == (136, 5, 45) and counts(rep.chips[BITWISE]) == (66, 2145, 301, 56, 10)


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: many slices of basis rows and a merge tree over their lists, 64 and 256 row tiles in the sweeps, several waves
    per workgroup in the enforcement phase with the halo rows between workgroups and the wrap between row 0 and row n - 1; lists of 300 rows
    run over several workgroups and over the waves of a workgroup."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert any(len(e["rows"]) == 300 and e["rows"][-1] - e["rows"][0] >= 299 for e in rep.entries if e["chip"] in (MEM, ADD, CPU))
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["free_rows"], 300)


@pytest.mark.parametrize("n,width", [(1, 7), (2, 7), (8, 7), (128, 63), (128, 64), (128, 65)])
def test_quad_airs(rc, n, width):
    machine, t = cases.quad_machine(width), cases.quad_trace(n, width)
    p = va.Prover(machine, rc, interpret_air=True)
    rep = p.product_audit([p.upload(t)], [], max_rows_per_entry=8)
    assert np.array_equal(rep.words, va.product_audit_host(machine, [t], [], max_rows_per_entry=8).words)
    if n == 128:
        assert {(e["i"], e["j"]): e["terms"] for e in rep.entries} == {k: [(c, 1)] for k, c in cases.QUAD_RELATIONS.items()}
        by = {(e["i"], e["j"]): e["enforced_rows"] for e in rep.entries}
        assert (by[(1, 1)], by[(1, 2)], by[(2, 2)]) == (n, n, 0)


def test_needle_traces(rc):
    machine = cases.free_machine(cases.NEEDLE_W)
    p = va.Prover(machine, rc, interpret_air=True)
    for kind in ("first", "last", "clean"):
        t = cases.needle(kind)
        rep = p.product_audit([p.upload(t)], [])
        assert np.array_equal(rep.words, va.product_audit_host(machine, [t], []).words), kind
        assert rep.relations(0) == cases.NEEDLE_RELATIONS[kind] and rep.chips[0]["rank"] == 41


def test_limits_and_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=9, max_rows_per_entry=2, max_terms=2)
    assert rep.truncated and rep.reported == 9 and rep.total_entries > 9
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    rep = p.product_audit(*upload(p, mt, prep), chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["relations"] == 0
    assert np.array_equal(rep.words, va.product_audit_host(p.machine, mt, prep, chips=[ADD, MEM]).words)


def test_a_chip_that_does_not_fit_the_lds_is_refused(rc):
    machine = too_wide_machine()
    mt = [np.arange(2 * 200, dtype=np.uint32).reshape(2, 200)]
    p = va.Prover(machine, rc, interpret_air=True)
    with pytest.raises(va.VgpuError, match="product_audit: .*does not fit a workgroup's LDS") as e:
        p.product_audit([p.upload(m) for m in mt], [])
    assert e.value.code == -1 and "too_wide" in str(e.value) and "163840" in str(e.value) and "200 columns" in str(e.value)  # VGPU_ERR_INVALID_ARG, with the arithmetic
    host = va.product_audit_host(machine, mt, [])  # the host audit has no limit
    assert (host.chips[0]["rank"], host.chips[0]["pairs"]) == (2, 1)


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.product_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.product_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("chip_mask names a chip", dict(chips=[20])), ("max_terms is at most 4096", dict(max_terms=5000)), ("max_terms", dict(max_terms=0))):
        with pytest.raises(va.VgpuError, match="product_audit: .*" + match) as e:
            prover.product_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_products_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--products")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--products")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(" product relation" in line and line.startswith("cpu: ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["products"], json.loads(out_host.read_text())["products"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
