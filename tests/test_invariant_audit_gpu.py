"""The invariant audit on the MI355X (vgpu_invariant_audit; kernels/invariant_audit.hip) against the host audit (vgpu_invariant_audit_host,
itself held to the reference by tests/test_invariant_audit_cpu.py) word for word: the basic prover and the interpreting prover over the
captured chips, from uploaded traces and from traces generated on the device; fib(1) (the height-1 chips), fib(25) and alu(50) with the pinned
facts, fib(582) (NW = 2 / 4, halo, wrap, many workgroups in both phases, lists of 300 rows); the captured analytic AIRs (width 5 and the
lane-word boundary) and the needle traces (128 phase-1 workgroups whose bases the merge eliminates); limits and chip mask; a captured AIR that
does not fit is refused with the arithmetic; determinism; argument validation; the context still proves the oracle's proof afterwards;
`check --invariants` on device 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import invariant_audit_cases as cases
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
    host = va.invariant_audit_host(provers["basic"].machine, mt, prep, **kw)
    reps = [provers["basic"].invariant_audit(*upload(provers["basic"], mt, prep), **kw), provers["ffi"].invariant_audit(*upload(provers["ffi"], mt, prep), chips=FFI_CHIPS, **kw)]
    main, pre = generate(provers["basic"], w)
    reps += [provers["basic"].invariant_audit(main, pre, **kw), provers["ffi"].invariant_audit(main, pre, chips=FFI_CHIPS, **kw)]
    for rep in reps:
        assert np.array_equal(rep.words, host.words), ([c for c in zip(rep.chips, host.chips) if c[0] != c[1]], [e for e in zip(rep.entries, host.entries) if e[0] != e[1]][:4])
        assert rep.device_ms > 0 and rep.evaluations == host.evaluations > 0
    return host, reps[0]


def relations_of(rep, chip):
    return {e["column"]: e for e in rep.entries if e["chip"] == chip and e["kind"] == "relation"}


def test_fib1_height_one_chips(provers):
    host, rep = audit_all(provers, va.Workload.fib(1))
    assert sum(1 for c in rep.chips if c["height"] == 1) >= 8 and all(c["audited"] for c in rep.chips)
    assert all(c["constant_columns"] == c["width"] for c in rep.chips if c["height"] == 1)


def test_fib25(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=1 << 20, max_terms=16)
    assert not rep.truncated and rep.total_entries == rep.reported > 0 and rep.holds(w.main_traces()) == []
    # tests/test_invariant_audit_cpu.py pins these against the reference
    assert rep.relations(ADD) == [12, 13, 14] and all(e["enforced_rows"] == 128 for e in relations_of(rep, ADD).values())
    assert {k: e["enforced_rows"] for k, e in relations_of(rep, CPU).items()} == {22: 105, 24: 105, 29: 256, 36: 256, 38: 104, 43: 105}


def test_alu50(provers):
    host, rep = audit_all(provers, va.Workload.alu(50), max_entries=1 << 20, max_rows_per_entry=7, max_terms=32)
    assert rep.chips[CPU]["height"] == 512 and relations_of(rep, CPU)[38]["enforced_rows"] == 0 and rep.chips[BITWISE]["relations"] == 14


def test_fib582_many_workgroups(provers):
    """cpu height 4096, mem 16384: many workgroups in the streaming elimination and a merge of all their bases; several waves per workgroup in
    the enforcement phase, the halo rows between workgroups and the wrap between row 0 and row n - 1; lists of 300 rows run over several
    workgroups and over the waves of a workgroup."""
    w = va.Workload.fib(582)
    assert w.cpu_height == 4096
    host, rep = audit_all(provers, w, max_rows_per_entry=300)
    print("fib(582): device %.3f ms, host audit %.1f ms (%.0f row evaluations)" % (rep.device_ms, host.host_ms, host.evaluations))
    assert any(len(e["rows"]) == 300 and e["rows"][-1] - e["rows"][0] >= 299 for e in rep.entries if e["chip"] in (MEM, ADD, CPU))
    for e in rep.entries:
        assert e["rows"] == sorted(set(e["rows"])) and len(e["rows"]) == min(e["free_rows"], 300)


@pytest.mark.parametrize("n,width", [(1, 5), (2, 5), (8, 5), (128, 63), (128, 64), (128, 65)])
def test_affine_airs(rc, n, width):
    machine, t = cases.affine_machine(width), cases.affine_trace(n, width)
    p = va.Prover(machine, rc, interpret_air=True)
    rep = p.invariant_audit([p.upload(t)], [], max_rows_per_entry=8)
    assert np.array_equal(rep.words, va.invariant_audit_host(machine, [t], [], max_rows_per_entry=8).words)
    if n == 8:
        assert [(e["column"], e["enforced_rows"]) for e in rep.entries] == [(2, 8), (3, 0), (4, 0)]
    if n == 128:
        assert [(e["column"], e["enforced_rows"]) for e in rep.entries] == [(2, n), (3, 0), (4, 0), (width - 1, 0)]


def test_needle_traces(rc):
    machine = cases.free_machine(cases.NEEDLE_W)
    p = va.Prover(machine, rc, interpret_air=True)
    for kind in ("first", "last", "stairs"):
        t = cases.needle(kind)
        rep = p.invariant_audit([p.upload(t)], [])
        assert np.array_equal(rep.words, va.invariant_audit_host(machine, [t], []).words), kind
        assert rep.relations(0) == cases.NEEDLE_INVARIANTS[kind] and all(e["rows"] == [0, 1, 2, 3] for e in rep.entries)


def test_limits_and_chip_mask(provers):
    w = va.Workload.fib(25)
    host, rep = audit_all(provers, w, max_entries=9, max_rows_per_entry=2, max_terms=2)
    assert rep.truncated and rep.reported == 9 and rep.total_entries > 9
    mt, prep = w.main_traces(), w.preprocessed()
    p = provers["basic"]
    rep = p.invariant_audit(*upload(p, mt, prep), chips=[ADD, MEM])
    assert [c["chip"] for c in rep.chips if c["audited"]] == [MEM, ADD] and rep.chips[CPU]["invariants"] == 0
    assert np.array_equal(rep.words, va.invariant_audit_host(p.machine, mt, prep, chips=[ADD, MEM]).words)


def test_a_chip_that_does_not_fit_the_lds_is_refused(rc):
    machine = too_wide_machine()
    mt = [np.arange(2 * 200, dtype=np.uint32).reshape(2, 200)]
    p = va.Prover(machine, rc, interpret_air=True)
    with pytest.raises(va.VgpuError, match="invariant_audit: .*does not fit a workgroup's LDS") as e:
        p.invariant_audit([p.upload(m) for m in mt], [])
    assert e.value.code == -1 and "too_wide" in str(e.value) and "163840" in str(e.value) and "200 columns" in str(e.value)  # VGPU_ERR_INVALID_ARG, with the arithmetic
    host = va.invariant_audit_host(machine, mt, [])  # the host audit has no limit
    assert host.chips[0]["rank"] == 2 and host.chips[0]["invariants"] == 199


def test_determinism(provers):
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    for p in provers.values():
        main, pre = upload(p, mt, prep)
        reps = [p.invariant_audit(main, pre, max_rows_per_entry=64) for _ in range(2)]
        assert np.array_equal(reps[1].words, reps[0].words)


def test_context_stays_usable(prover, rc):
    """An audit leaves nothing behind: the pool's live bytes are what they were and the next fib(25) proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    w = va.Workload.fib(25)
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.invariant_audit(main, pre)
    assert rep.total_entries > 0 and prover.memory()[0] == live_before
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def test_device_argument_validation(prover, fib25):
    main, pre = upload(prover, fib25.main_traces(), fib25.preprocessed())
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("max_entries", dict(max_entries=0)),
                      ("chip_mask names a chip", dict(chips=[20])), ("max_terms is at most 4096", dict(max_terms=5000)), ("max_terms", dict(max_terms=0))):
        with pytest.raises(va.VgpuError, match="invariant_audit: .*" + match) as e:
            prover.invariant_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_invariants_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--invariants")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--invariants")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and any(" invariant" in line and line.startswith("cpu: ") for line in r.stdout.split("\n"))
    dev, host = json.loads(out.read_text())["invariants"], json.loads(out_host.read_text())["invariants"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}
