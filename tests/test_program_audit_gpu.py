"""The program audit on the MI355X (vgpu_program_audit; kernels/program_audit.hip) against the host audit (vgpu_program_audit_host, itself held
to the numpy reference by tests/test_program_audit_cpu.py) word for word: the basic prover and the interpreting prover over the captured chips,
from uploaded traces and from traces generated on the device; the VM's witnesses with their pinned numbers, fib(582) from the operation logs;
fib(25) tampered seven ways; every edge trace of tests/program_audit_cases.py, the two-slice table with hot bins on the slice edges and a bin
count above 2^16; synthetic fetch traces at the heights where the passes get a second run, table entry and scan chunk; the limits;
determinism; the pool's live bytes; refusals that leave the prover usable; `check --program` on device 0; the fifteen audits back to back on
one context."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import program_audit_cases as cases
import valida_amd as va
import valida_programs as vp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product", "domain", "memory", "program"]
PINNED = {"fib25": (256, 32, 23, 7, 65, 138, 64, 53), "fib582": (4096, 32, 23, 13, 583, 2923, 5, 1167), "alu100": (1024, 16, 14, 13, 120, 805, 119, 99),
          "signed_inequality": (32, 32, 20, 19, 13, 19, 12, 0)}


@pytest.fixture(scope="module")
def provers(prover, rc):
    """The in-tree machine with its compiled chip kernels, and the same chips captured through the FFI on an interpreting prover."""
    return {"basic": prover, "ffi": va.Prover(va.Machine.basic_via_ffi(), rc, interpret_air=True)}


@pytest.fixture(scope="module")
def roms(rc):
    """The captured `rom` machines by field count, each with its interpreting prover."""
    made = {}

    def get(n_fields):
        if n_fields not in made:
            made[n_fields] = (cases.rom_machine(n_fields), va.Prover(cases.rom_machine(n_fields), rc, interpret_air=True))
        return made[n_fields]

    return get


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


def same(rep, host):
    assert np.array_equal(rep.words, host.words), (rep.counters, host.counters, rep.hard[:3], host.hard[:3], rep.unfetched[:3], host.unfetched[:3])
    assert rep.device_ms > 0 and rep.evaluations == host.evaluations


def audit_uploaded(provers, mt, prep, **kw):
    host = va.program_audit_host(provers["basic"].machine, mt, prep, **kw)
    for p in provers.values():
        same(p.program_audit(*upload(p, mt, prep), **kw), host)
    return host


def on_rom(roms, n_fields, main, prep, **kw):
    machine, p = roms(n_fields)
    kw = dict(cases.rom_opts(n_fields), **kw)
    host = va.program_audit_host(machine, main, prep, **kw)
    same(p.program_audit(*upload(p, main, prep), **kw), host)
    return host


@pytest.mark.parametrize("name", list(cases.VM))
def test_vm_witnesses_uploaded(provers, name):
    main, prep, rom_len = cases.witness(name)
    host = audit_uploaded(provers, main, prep, rom_len=rom_len)
    c = host.counters
    assert host.total_hard == 0 and c["unfetched_words"] == 0 and host.total_wrapped == (8 if name == "signed_inequality" else 0)
    if name in PINNED:
        assert (c["fetches"], c["table_rows"], c["rom_len"], c["hottest_pc"], c["hottest_count"], c["sequential"], c["stay"], c["jumps"]) == PINNED[name]
    if name == "signed_inequality":
        assert host.wrapped[0]["row"] == 5 and {j for f in host.wrapped for j in f["fields"]} == {2, 3}


@pytest.mark.parametrize("name", ["fib25", "fib582"])
def test_traces_generated_on_the_device(provers, name):
    """From the operation logs, no ingest copy: the audit reads the generated traces where they lie.  fib(582): 4096 cpu rows, one full
    histogram run and sixteen judge workgroups, 583 fetches in the hottest bin."""
    w = cases.workload(name)
    mt, prep, rom_len = cases.witness(name)
    host = va.program_audit_host(provers["basic"].machine, mt, prep, rom_len=rom_len)
    basic = provers["basic"]
    log = basic.upload_oplog(w.oplog())
    main, pre = [basic.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, basic.upload(m)) for c, m in prep]
    for p in provers.values():
        same(p.program_audit(main, pre, rom_len=rom_len), host)
    same(basic.program_audit(*upload(basic, mt, prep), rom_len=rom_len), host)
    assert host.total_hard == 0 and host.counters["hottest_count"] == PINNED[name][4]


@pytest.mark.parametrize("kind", cases.TAMPERINGS)
def test_tampered_fib25(provers, kind):
    main, prep, rom_len = cases.vm_tampered(kind)
    host = audit_uploaded(provers, main, prep, rom_len=rom_len)
    want = {"operand": (1, 0), "wrapped": (0, 1), "pc_other_word": (3, 0), "pc_padding": (3, 0), "pc_p_minus_1": (2, 0), "multiplicity": (1, 0), "key": (1, 0)}[kind]
    assert (host.total_hard, host.total_wrapped) == want


def test_edge_traces(roms):
    """Fetch heights 1 to 8192, table heights 1 to 65536 (two histogram slices, the table in LDS or in device memory), one pc, 63 lanes and one,
    two bins, the hot bins on the slice edges, the tamperings, the planted rows, one and eight fields."""
    for name, nf, (main, prep), rom_len in cases.edge_cases():
        on_rom(roms, nf, main, prep, rom_len=rom_len)


def test_a_bin_count_above_2_to_the_16(roms):
    host = on_rom(roms, 2, *cases.big_bin())
    assert host.counters["hottest_count"] == 1 << 17


@pytest.mark.parametrize("n", [4096, 8192, 32768, 1 << 20])
def test_block_boundaries(roms, n):
    """4096 fetches fill one histogram run (PG_HIST_RUN) exactly: sixteen judge workgroups, one histogram workgroup; 8192 is the first height with a
    second histogram workgroup, whose bins meet the first's in device memory; 32768 has eight runs and 128 entries in each judge table, half of
    the scan workgroup's threads; at 2^20 the tables have 4096 entries and every thread of the scan takes sixteen (above 65536 rows a thread
    takes more than one)."""
    main, prep = cases.synthetic(n)
    host = on_rom(roms, 2, main, prep, max_findings=300)
    c = host.counters
    assert c["fetches"] == n and c["wrong_instruction"] > 0 and c["wrapped_operand"] > 0 and c["pc_out_of_rom"] == len(range(4098, n, 4099))
    assert c["pc_out_of_rom"] >= c["multiplicity"] and (c["multiplicity"] > 0) == (c["pc_out_of_rom"] > 0)  # a word's multiplicity is wrong iff it lost a fetch to a moved pc
    assert c["hard"] == c["wrong_instruction"] + c["pc_out_of_rom"] + c["multiplicity"] and len(host.hard) == min(300, c["hard"])


def test_limits_and_determinism(roms):
    main, prep = cases.many()
    for k in (0, 1, 300, 301, 601, 1 << 20):
        host = on_rom(roms, 2, main, prep, max_findings=k, max_ranges=k)
        assert host.total_hard == 900 and len(host.hard) == min(k, 900) and len(host.wrapped) == min(k, 300) and len(host.unfetched) == min(k, 512)
    machine, p = roms(2)
    up = upload(p, *cases.synthetic(8192))
    reps = [p.program_audit(*up, max_findings=1000, **cases.rom_opts(2)) for _ in range(2)]
    assert np.array_equal(reps[0].words, reps[1].words) and reps[0].total_hard > 0


def test_context_stays_usable_after_a_pass_and_after_refusals(prover, rc, fib25, roms):
    """An audit leaves nothing behind: the pool's live bytes are what they were; a refusal returns its status and message; the next fib(25)
    proof is the oracle's."""
    from oracle import pyoracle as po  # checker only

    mt, prep = fib25.main_traces(), fib25.preprocessed()
    main, pre = upload(prover, mt, prep)
    live_before = prover.memory()[0]
    rep = prover.program_audit(main, pre, rom_len=fib25.program_len)
    assert rep.counters["hottest_count"] == 65 and prover.memory()[0] == live_before
    for match, kw in (("one main trace per chip", dict(main=main[:-1])), ("needs its preprocessed trace", dict(pre=pre[:1])), ("at most 2\\^20", dict(max_findings=(1 << 20) + 1)),
                      ("rom_len 33 is above the table's height 32", dict(rom_len=33)), ("pc_col 99 is outside chip cpu's trace", dict(fetch=(0, 99, [3]), table=(1, 0, [1], 0))),
                      ("table chip cpu has no preprocessed trace", dict(table=(0, 0, [1, 2, 3, 4, 5, 6], 0))), ("mult_col 1 is outside chip program's trace", dict(table=(1, 0, [1, 2, 3, 4, 5, 6], 1))),
                      ("table column 7 .* is outside chip program's preprocessed trace", dict(table=(1, 0, [1, 2, 3, 4, 5, 7], 0))), ("fetch_chip 14 is not a chip", dict(fetch=(14, 1, [3, 4, 5, 6, 7, 8])))):
        with pytest.raises(va.VgpuError, match="program_audit: .*" + match) as e:
            prover.program_audit(kw.pop("main", main), kw.pop("pre", pre), **kw)
        assert e.value.code == -1
    machine, p = roms(2)
    m2, p2 = cases.clean(cases.loop_pcs(64, 32), 32)
    with pytest.raises(va.VgpuError, match="program_audit: the table chip's main trace has 32 rows and its preprocessed trace 16"):
        p.program_audit([p.upload(m) for m in m2], [(1, p.upload(p2[0][1][:16]))], **cases.rom_opts(2))
    assert prover.memory()[0] == live_before and prover.program_audit(main, pre, rom_len=fib25.program_len).counters == rep.counters
    proof = prover.prove(main, pre)
    assert proof.bytes() == po.prove_basic(mt, prep[0][1], prep[1][1], rc).bytes()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "valida_amd.cli"] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_cli_check_program_on_the_device(tmp_path):
    loop, adv, out, out_host = tmp_path / "loop.bin", tmp_path / "advice", tmp_path / "report.json", tmp_path / "report_host.json"
    loop.write_bytes(vp.machine_code(vp.byte_loop_program(50)))
    adv.write_bytes(bytes(range(30)))
    r = _cli("check", loop, out, adv, "--device", 0, "--program")
    assert r.returncode == 0, r.stderr[-3000:]
    h = _cli("check", loop, out_host, adv, "--host", "--program")
    assert h.returncode == 0, h.stderr[-3000:]
    assert r.stdout == h.stdout and [line for line in r.stdout.split("\n") if line.startswith("cpu: ")][-1].endswith("no finding")
    dev, host = json.loads(out.read_text())["program"], json.loads(out_host.read_text())["program"]
    assert dev["device_ms"] > 0 and host["device_ms"] == 0
    timing = ("device_ms", "host_ms", "evaluations")
    assert {k: v for k, v in dev.items() if k not in timing} == {k: v for k, v in host.items() if k not in timing}


def test_fifteen_audits_back_to_back_on_one_context(prover, machine, fib25):
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
        for name in AUDITS + ["program", "memory"]:  # and the program audit twice in a row, then the audit whose scan it shares
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
