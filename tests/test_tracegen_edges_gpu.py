"""The device trace generators (valida_amd/csrc/kernels/tracegen.hip, and the heights and output-window sums of host/prover.cpp) on operation
logs at their edges: every synthetic case of tests/oplog_corpus.py and three VM programs, against the Python reference of Chip::generate_trace
(tests/tracegen_ref.py, pinned to the host and judged by the AIR in tests/test_tracegen_edges_cpu.py).  Exact equality; nothing is skipped or
sampled."""
import time

import pytest

import oplog_corpus as oc
import tracegen_ref as tr
import valida_amd as va
from conftest import first_mismatch
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [c.name for c in oc.cases()])
def test_generated_traces_of_a_synthetic_log_match_the_reference(prover, case):
    c = oc.case(case)
    want = {chip: oc.reference(case, chip) for chip in c.chips}  # computed once per case, shared with the CPU tests of the same session
    t0 = time.perf_counter()
    log = prover.upload_oplog(c.log.desc())
    for chip in c.chips:
        got = prover.generate_trace(log, chip)
        assert got.shape == want[chip].shape, (case, va.CHIP_NAMES[chip])
        assert first_mismatch(got.download(), want[chip]) is None, (case, va.CHIP_NAMES[chip])
    print("%s: %d chips, %d rows, %.1f ms on the device path" % (case, len(c.chips), sum(w.shape[0] for w in want.values()), 1e3 * (time.perf_counter() - t0)))


@pytest.mark.parametrize("name", list(oc.VM_PROGRAMS))
def test_vm_program_on_the_device(prover, machine, rc, name):
    w, pinned = oc.vm_workload(name), oc.VM_PROGRAMS[name]
    mt, prep = w.main_traces(), w.preprocessed()
    ref_log = tr.OpLog.from_desc(w.oplog())
    log = prover.upload_oplog(w.oplog())
    dmain = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
    for chip, d in enumerate(dmain):
        got = d.download()
        assert got.shape == mt[chip].shape, va.CHIP_NAMES[chip]
        assert first_mismatch(got, tr.generate_trace(ref_log, chip)) is None, "reference, " + va.CHIP_NAMES[chip]
        assert first_mismatch(got, mt[chip]) is None, "host, " + va.CHIP_NAMES[chip]
    proof = prover.prove(dmain, [(c, prover.upload(m)) for c, m in prep])
    ref = po.prove_basic(mt, prep[0][1], prep[1][1], rc)
    assert first_mismatch(proof.words, ref.words) is None
    commit = va.host_commit_root([m for _, m in prep], rc)
    oracle = po.verify_basic(prep[0][1], prep[1][1], proof.words, rc)
    host = va.verify(machine, rc, proof.words, commit)
    batched = va.Verifier(machine, rc, device=0).verify_batch([proof.words], [commit])[0]
    assert oracle == pinned["oracle"]
    assert host == batched and (host is None) == (oracle is None)
    if oracle is not None:
        assert oracle in host and "chip %s:" % pinned["rejected_at"] in host
