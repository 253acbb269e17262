"""The twelve witness audits back to back on one prover context and fib(25), the product audit among them: from traces generated on the device
and again from the same matrices uploaded, every report word for word the host audit's; the pool's live bytes afterwards are what they were
and the next proof is byte for byte the proof made before them.  (tests/test_eleven_audits_gpu.py does the same for the eleven audits before
this one and stays as it is.)"""
import numpy as np
import pytest

import valida_amd as va

pytestmark = pytest.mark.gpu
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product"]


def test_twelve_audits_back_to_back_on_one_context(prover, machine, fib25):
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    host = {name: getattr(va, name + "_audit_host")(machine, mt, prep) for name in AUDITS}
    pre = [(c, prover.upload(m)) for c, m in prep]
    proof_before = prover.prove([prover.upload(m) for m in mt], pre).bytes()
    log = prover.upload_oplog(fib25.oplog())
    generated = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
    uploaded = [prover.upload(t.download()) for t in generated]
    live_before = prover.memory()[0]
    for main in (generated, uploaded):
        for name in AUDITS + ["product", "invariant", "rank"]:  # and the product audit twice in a row, then the audits whose code it shares
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
