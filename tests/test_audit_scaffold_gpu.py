"""What the nine witness audits share on the device (host/audit_pass.hpp), on one prover context and fib(25): all nine back to back from traces
generated on the device (already in the working layout) and again from the same matrices uploaded (ingested into copies the pass owns), every
report word for word the host audit's; the device pass lies inside the call (0 < device_ms <= host_ms); the pool's live bytes after the
eighteen passes are what they were; the next proof is byte for byte the proof made before them; and a refused call leaves the context free for
the next audit."""
import numpy as np
import pytest

import valida_amd as va

pytestmark = pytest.mark.gpu
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step"]


class NullTrace:
    """A null vgpu_trace_t* in a trace list."""
    _h = None


def test_nine_audits_back_to_back_on_one_context(prover, machine, fib25):
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    host = {name: getattr(va, name + "_audit_host")(machine, mt, prep) for name in AUDITS}
    pre = [(c, prover.upload(m)) for c, m in prep]
    proof_before = prover.prove([prover.upload(m) for m in mt], pre).bytes()
    log = prover.upload_oplog(fib25.oplog())
    generated = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
    uploaded = [prover.upload(t.download()) for t in generated]
    live_before = prover.memory()[0]
    for main in (generated, uploaded):
        for name in AUDITS:
            rep = getattr(prover, name + "_audit")(main, pre)
            assert np.array_equal(rep.words, host[name].words), name
            assert 0 < rep.device_ms <= rep.host_ms, (name, rep.device_ms, rep.host_ms)
    assert prover.memory()[0] == live_before
    assert prover.prove(uploaded, pre).bytes() == proof_before
    for name in AUDITS:
        with pytest.raises(va.VgpuError, match="null trace") as e:
            getattr(prover, name + "_audit")(uploaded[:-1] + [NullTrace()], pre)
        assert e.value.code == -1
    rep = prover.rank_audit(uploaded, pre)
    assert np.array_equal(rep.words, host["rank"].words) and prover.memory()[0] == live_before
