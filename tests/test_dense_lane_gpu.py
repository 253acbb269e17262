"""The dense lane on the GPU (valida_amd/csrc/host/dense_lane.hpp, DeviceTree::build_impl): pure scheduling, so every proof word must stay what it
was — with several contexts sharing the lane, with one alone, behind a context destroyed while it was the lane's tail, and with a proof that fails
beside the others.  Workload fib(582) (cpu 2^12, mem 2^14 rows) with VGPU_DENSE_LANE_MIN_NODES=1, so that every tree with a thread-per-node
launch takes the lane.  Each scenario runs in a process of its own (this file as a script) under a time limit; the lane switch is read when a
context is created, so the lane-off reference context is created in the same process, before the switch is turned on."""
import gc
import hashlib
import json
import os
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fib582_oracle.json")
STEP_TIMEOUT_S = 120

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the scenarios (child process)
class _Bench:
    def __init__(self, hash_name="keccak", log_blowup=1):
        import valida_amd as va

        self.va = va
        with open(GOLDEN) as f:
            self.golden = json.load(f)
        w = va.Workload.fib(self.golden["n"])
        assert w.cpu_height == 1 << 12
        self.mt, self.prep = w.main_traces(), w.preprocessed()
        self.kw = dict(device=0, log_blowup=log_blowup, hash_kind=va.HASH_POSEIDON16 if hash_name == "poseidon" else va.HASH_KECCAK256)
        self.is_golden_config = hash_name == "keccak" and log_blowup == 1
        self.rc = va.poseidon_round_constants()
        os.environ["VGPU_DENSE_LANE"] = "0"
        off = self.context()
        ref = self.prove(off)
        self.ref = ref.words.copy()
        assert off[0].lane_stats() == (0, 0), "a lane-off context touched the lane"
        if self.is_golden_config:
            assert hashlib.sha256(ref.bytes()).hexdigest() == self.golden["proof_sha256"], "the lane-off proof is not the oracle's"
        os.environ["VGPU_DENSE_LANE"] = "1"

    def context(self):
        p = self.va.Prover(self.va.Machine.basic(), self.rc, **self.kw)
        return p, [p.upload(m) for m in self.mt], [(c, p.upload(m)) for c, m in self.prep]

    @staticmethod
    def prove(ctx, asynchronous=False):
        p, dm, dp = ctx
        return p.prove_async(dm, dp).wait() if asynchronous else p.prove(dm, dp)

    def check(self, proof, what):
        import numpy as np

        assert np.array_equal(proof.words, self.ref), "%s: words differ from the lane-off proof" % what
        if self.is_golden_config:
            assert hashlib.sha256(proof.bytes()).hexdigest() == self.golden["proof_sha256"], "%s: not the oracle's proof" % what

    def run_threads(self, jobs):
        """jobs: callables; each runs on a thread of its own; the first exception of any is raised here."""
        errors = []

        def wrap(f):
            try:
                f()
            except BaseException as e:  # noqa: BLE001 - reported by the parent below
                errors.append(e)

        ts = [threading.Thread(target=wrap, args=(j,)) for j in jobs]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errors:
            raise errors[0]


def _prove_n(b, ctx, n, what, asynchronous=True):
    def job():
        for i in range(n):
            b.check(b.prove(ctx, asynchronous), "%s, proof %d" % (what, i))
    return job


def scenario_three(hash_name):
    b = _Bench(hash_name)
    ctxs = [b.context() for _ in range(3)]
    b.run_threads([_prove_n(b, c, 8, "context %d of three" % i) for i, c in enumerate(ctxs)])
    stats = [c[0].lane_stats() for c in ctxs]
    assert all(e > 0 for e, _ in stats), "a context never entered the lane: %s" % stats
    assert all(w <= e for e, w in stats)
    assert sum(w for _, w in stats) > 0, "no context ever waited for another's event with three proving at once: %s" % stats
    return {"lane_stats": stats}


def scenario_alone():
    b = _Bench()
    ctx = b.context()
    for i in range(4):
        b.check(b.prove(ctx, True), "one context alone, proof %d" % i)
    entered, waited = ctx[0].lane_stats()
    assert entered > 0, "the lone context never entered the lane"
    assert waited == 0, "a context alone on the lane waited %d times: only its own event can have been the tail" % waited
    return {"lane_stats": [entered, waited]}


def scenario_destroy_tail():
    b = _Bench()
    a, c2, tail = b.context(), b.context(), b.context()
    b.check(b.prove(a), "first context")
    b.check(b.prove(c2), "second context")
    b.check(b.prove(tail), "third context")  # the last to leave the lane: its event is the tail

    # destroyed BEFORE the others' next enter(): whoever enters first meets what the destroyed tail left behind
    tail = None
    gc.collect()
    b.run_threads([_prove_n(b, a, 4, "behind the destroyed tail, first"), _prove_n(b, c2, 4, "behind the destroyed tail, second")])
    return {"lane_stats": [a[0].lane_stats(), c2[0].lane_stats()]}


def scenario_invalid():
    b = _Bench()
    va = b.va
    bad_ctx, o1, o2 = b.context(), b.context(), b.context()
    bad = [m.copy() for m in b.mt]
    bad[3][5, 11] = (int(bad[3][5, 11]) + 1) % va.P  # ADD32 row 5: output byte 0 (column 11) is off by one
    msg = []

    def fails():
        p, _, dp = bad_ctx
        try:
            p.prove([p.upload(m) for m in bad], dp, check=True)  # debug_flags | 2
        except va.VgpuError as e:
            msg.append(str(e))

    b.run_threads([fails, _prove_n(b, o1, 4, "beside a failing proof, first"), _prove_n(b, o2, 4, "beside a failing proof, second")])
    assert msg and "chip add" in msg[0].lower() and "row 5" in msg[0], "the invalid witness was not refused with its message: %r" % msg
    b.check(b.prove(bad_ctx), "the failed context's next valid proof")
    b.check(b.prove(bad_ctx, True), "the failed context's next valid asynchronous proof")
    return {"message": msg[0][:200]}


def scenario_switch(log_blowup):
    b = _Bench(log_blowup=int(log_blowup))  # the reference is the VGPU_DENSE_LANE=0 proof
    c1, c2 = b.context(), b.context()
    b.run_threads([_prove_n(b, c1, 3, "lane on, log_blowup %s, first" % log_blowup), _prove_n(b, c2, 3, "lane on, log_blowup %s, second" % log_blowup)])
    stats = [c1[0].lane_stats(), c2[0].lane_stats()]
    assert all(e > 0 for e, _ in stats), stats
    return {"lane_stats": stats}


SCENARIOS = {"three": scenario_three, "alone": scenario_alone, "destroy_tail": scenario_destroy_tail, "invalid": scenario_invalid, "switch": scenario_switch}


# ---------------------------------------------------------------------------------------------------------------- the tests (parent process)
def _run(*args):
    env = dict(os.environ, VGPU_DENSE_LANE_MIN_NODES="1")
    env.pop("VGPU_DENSE_LANE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, env=env, timeout=STEP_TIMEOUT_S)
    assert r.returncode == 0, "scenario %s ended with status %d\n%s" % (args, r.returncode, (r.stdout + r.stderr)[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(args, out)
    return out


@pytest.mark.parametrize("hash_name", ["keccak", "poseidon"])
def test_three_contexts_share_the_lane_and_prove_the_same_words(hash_name):
    _run("three", hash_name)


def test_a_context_alone_never_waits_on_its_own_event():
    _run("alone")


def test_a_context_destroyed_as_the_tail_does_not_disturb_the_others():
    _run("destroy_tail")


def test_a_failing_proof_leaves_the_lane_usable():
    _run("invalid")


@pytest.mark.parametrize("log_blowup", [1, 2])
def test_lane_on_and_off_give_identical_words(log_blowup):
    _run("switch", log_blowup)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print(json.dumps(SCENARIOS[sys.argv[1]](*sys.argv[2:])))
