"""Every stage of the device path with the HBM pool made adversarial (vgpu_prover_set_pool_poison): each block the pool hands out,
fresh or recycled, and each block that returns to its cache is first filled with a poison word.  A stage that reads a cell it has not written, a
host pass that forgets a memset in front of its atomics, or a view used after its buffer went back to the pool then computes from the poison
instead of from zeros or from the previous identical call's right answer.  Every comparison is bit-exact against the reference the unpoisoned
tests use (the oracle, tests/tracegen_ref.py, the audits' host twins), never against a device result; every test ends by asserting that the pool
did fill blocks during it.

The provers are this module's own (the hook synchronises the device twice per pool operation: the session `prover` stays clean).  Words:
0x00000001 turns a flag that should be 0 on and puts a counter off by one; 0x5A5A5A5A is below p, a valid Montgomery word that enters arithmetic
silently; 0xFFFFFFFF is non-canonical, the bus audit's dead key, and the worst case for atomicMin / atomicAnd targets.

Wall time of this file on one MI355X: profiles/pool_poison.txt."""
import contextlib

import numpy as np
import pytest

import edge_stage_cases as esc
import memory_audit_cases as mcases
import oplog_corpus as oc
import program_audit_cases as pcases
import valida_amd as va
import verify_corpus as vc
from conftest import first_mismatch
from oracle import pyoracle as po  # checker only
from test_bus_audit_cpu import ADD, witness

pytestmark = pytest.mark.gpu
P = va.P
WORDS = [0x00000001, 0x5A5A5A5A, 0xFFFFFFFF]
KECCAK, POSEIDON = va.HASH_KECCAK256, va.HASH_POSEIDON16
AUDITS = ["bus", "constraint", "mutation", "coverage", "pair", "rank", "field", "link", "step", "invariant", "transition", "product", "domain", "memory", "program"]

_REF = {}  # references are computed once and shared by the three words


def ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


@contextlib.contextmanager
def oracle_mmcs(hash_kind, rc):
    po.set_mmcs_hash(1 if hash_kind == POSEIDON else 0, rc)
    try:
        yield
    finally:
        po.set_mmcs_hash(0)


class Pool:
    """The poisoned prover contexts of one word, one per configuration, made on first use and kept for the module."""

    def __init__(self, word, rc):
        self.word, self.rc, self._provers, self._machines = word, rc, {}, {}

    def machine(self, ffi=False):
        if ffi not in self._machines:
            self._machines[ffi] = va.Machine.basic_via_ffi() if ffi else va.Machine.basic()
        return self._machines[ffi]

    def fresh(self, ffi=False, **cfg):
        p = va.Prover(self.machine(ffi), self.rc, **cfg)
        p.set_pool_poison(self.word)  # mode 3: on alloc and on release
        return p

    def prover(self, ffi=False, **cfg):
        cfg = {k: v for k, v in cfg.items() if v != {"log_blowup": 1, "hash_kind": KECCAK, "interpret_air": False}.get(k, None)}  # one context per configuration
        key = (ffi,) + tuple(sorted(cfg.items()))
        if key not in self._provers:
            self._provers[key] = self.fresh(ffi, **cfg)
        return self._provers[key]

    def prover_of(self, name, make_machine, **cfg):
        """A poisoned context over a machine of a test's own."""
        if name not in self._provers:
            self._machines[name] = make_machine()
            p = va.Prover(self._machines[name], self.rc, **cfg)
            p.set_pool_poison(self.word)
            self._provers[name] = p
        return self._machines[name], self._provers[name]


@pytest.fixture(scope="module", params=WORDS, ids=["%08x" % w for w in WORDS])
def pool(request, rc):
    yield Pool(request.param, rc)


@contextlib.contextmanager
def drew_poison(*provers):
    """The body really ran on poisoned blocks: every context filled blocks on allocation and on release meanwhile."""
    before = [p.pool_poison_stats() for p in provers]
    yield
    for p, b in zip(provers, before):
        a = p.pool_poison_stats()
        assert all(x > y for x, y in zip(a, b)), "the pool filled nothing during this test: %r -> %r" % (b, a)


def rand_matrix(rng, h, w):
    return rng.integers(0, P, size=(h, w), dtype=np.uint32)


def upload(p, mt, prep):
    return [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]


# ---- the hook itself ------------------------------------------------------------------------------------------------------------------------
def test_peek_sees_the_word_in_a_fresh_and_in_a_recycled_block(pool):
    p = pool.fresh()
    with drew_poison(p):
        p.trim()  # nothing cached: the next block of this size comes from the driver
        head, last = p.pool_peek(1000, 250)  # 1000 bytes round to 1024: the last word of the block is word 255, beyond what the "stage" asked for
        assert np.all(head == pool.word) and last == pool.word, "fresh block"
        head, last = p.pool_peek(1000, 250)  # the same block, back from the cache
        assert np.all(head == pool.word) and last == pool.word, "recycled block"
        head, last = p.pool_peek(1, 0)
        assert head.size == 0 and last == pool.word
        for bad in ((0, 0), (1000, 251)):
            with pytest.raises(va.VgpuError) as e:
                p.pool_peek(*bad)
            assert e.value.code == -1


def test_a_released_matrix_is_gone_from_the_block_the_next_stage_gets(pool):
    """The hazard, then the hook: without poison a stage that reads before it writes sees the previous buffer of its size word for word; with the
    release fill alone (nothing is filled on the way out) it sees the word: the fill on release and the exact-size reuse."""
    p = pool.fresh()
    m = rand_matrix(np.random.default_rng(3), 50, 5)  # 1000 bytes
    m[m == pool.word] ^= 2
    p.set_pool_poison(None)
    before = p.pool_poison_stats()
    p.trim()
    t = p.upload(m)
    del t
    head, _ = p.pool_peek(1000, 250)
    assert np.array_equal(head, m.ravel()), "the pool did not hand the released block to the next request of its size"
    assert p.pool_poison_stats() == before, "the hook filled blocks while it was off"
    p.set_pool_poison(pool.word, on_alloc=False, on_release=True)
    p.trim()
    t = p.upload(m)
    del t
    head, last = p.pool_peek(1000, 250)
    assert np.all(head == pool.word) and last == pool.word
    after = p.pool_poison_stats()
    assert after[:2] == before[:2] and after[2] > before[2] and after[3] >= before[3] + 1024


def test_with_the_hook_off_nothing_is_filled(pool, rc, fib25):
    p = pool.fresh()
    p.set_pool_poison(None)
    before = p.pool_poison_stats()
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    proof = p.prove(*upload(p, mt, prep))
    assert proof.bytes() == ref("proof fib25", lambda: po.prove_basic(mt, prep[0][1], prep[1][1], rc)).bytes()
    assert p.pool_poison_stats() == before
    with drew_poison(p):
        p.set_pool_poison(pool.word)
        assert p.prove(*upload(p, mt, prep)).bytes() == proof.bytes()


def test_the_switch_is_refused_while_a_ticket_is_outstanding(pool, rc):
    p = pool.fresh()
    _, mt, prep, want = _workload("fib582", rc)
    want = want.bytes()
    with drew_poison(p):
        main, pre = upload(p, mt, prep)
        ticket = p.prove_async(main, pre)
        with pytest.raises(va.VgpuError, match="a proof or an audit is running") as e:
            p.set_pool_poison(None)
        assert e.value.code == -1
        assert ticket.wait().bytes() == want  # and the proof kept the poison it started with
        p.set_pool_poison(pool.word)  # accepted again
        assert p.prove(main, pre).bytes() == want


def test_trim_still_frees_and_the_next_proof_is_the_oracles(pool, rc, fib25):
    p = pool.fresh()
    mt, prep = fib25.main_traces(), fib25.preprocessed()
    want = ref("proof fib25", lambda: po.prove_basic(mt, prep[0][1], prep[1][1], rc)).bytes()
    with drew_poison(p):
        main, pre = upload(p, mt, prep)
        assert p.prove(main, pre).bytes() == want
        live = p.memory()[0]
        assert p.trim() > 0 and p.memory()[0] == live
        assert p.prove(main, pre).bytes() == want


# ---- LDE and commit ---------------------------------------------------------------------------------------------------------------------------
# the dispatch of launch_lde_natural, each kernel at the smallest height that reaches it: k_lde_mid alone; the generic three-kernel path through the
# scratch matrices s1 / s2; k_lde_mid12; the fixed <8, 6> and <10, 4> strided shapes; k_lde_mid14
LDE_SHAPES = [(0, 3, 1), (3, 5, 1), (12, 2, 1), (13, 3, 1), (14, 2, 2), (16, 1, 1), (20, 1, 1), (22, 1, 1), (23, 1, 1)]


@pytest.mark.parametrize("log_h,w,log_blowup", LDE_SHAPES)
def test_lde_and_root(pool, log_h, w, log_blowup):
    m = ref(("lde m", log_h, w), lambda: rand_matrix(np.random.default_rng(1000 + log_h), 1 << log_h, w))
    want = ref(("lde", log_h, w, log_blowup), lambda: (po.committed_lde(m, log_blowup, 31), po.commit_root([m], log_blowup=log_blowup)))
    p = pool.prover(log_blowup=log_blowup)
    with drew_poison(p):
        pd = p.commit_batches([p.upload(m)])
        assert first_mismatch(pd.lde(0), want[0]) is None
        assert first_mismatch(pd.root, want[1]) is None
        del pd


BATCHES = {
    "mixed_height": (11, [(1 << 8, 51), (1 << 5, 1), (1 << 9, 14), (1 << 7, 16), (1, 16), (1 << 8, 34), (1, 79), (1 << 5, 33), (1 << 9, 68)]),
    "lane_pair_threshold": (13, [(1 << 16, 2), (1 << 15, 35), (1 << 14, 69), (1 << 13, 34), (1 << 12, 33), (1 << 11, 67), (1 << 10, 68), (1 << 9, 1), (1 << 14, 1)]),
    "single_row": (12, [(1, 3), (1, 40), (1, 7)]),
}


@pytest.mark.parametrize("hash_kind", [KECCAK, POSEIDON], ids=["keccak", "poseidon"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_roots(pool, rc, name, hash_kind):
    seed, shapes = BATCHES[name]
    rng = np.random.default_rng(seed)
    mats = ref(("batch", name), lambda: [rand_matrix(rng, h, w) for h, w in shapes])
    with oracle_mmcs(hash_kind, rc):
        want = ref(("batch root", name, hash_kind), lambda: po.commit_root(mats))
    p = pool.prover(hash_kind=hash_kind)
    with drew_poison(p):
        assert first_mismatch(p.commit_batches([p.upload(m) for m in mats]).root, want) is None


@pytest.mark.parametrize("hash_kind", [KECCAK, POSEIDON], ids=["keccak", "poseidon"])
def test_shifted_coset_lde(pool, rc, hash_kind):
    m = ref("shifted m", lambda: rand_matrix(np.random.default_rng(7), 1 << 9, 10))
    shift = 31 * 31 % P
    with oracle_mmcs(hash_kind, rc):
        want = ref(("shifted", hash_kind), lambda: (po.committed_lde(m, 1, pow(31, P - 2, P)), po.commit_root([m], shifts=[shift])))
    p = pool.prover(hash_kind=hash_kind)
    with drew_poison(p):
        pd = p.commit_batches([p.upload(m)], coset_shifts=[shift])
        assert first_mismatch(pd.lde(0), want[0]) is None
        assert first_mismatch(pd.root, want[1]) is None


OPEN_SHAPES = {
    "valu": [[(64, 130), (64, 3)], [(256, 2), (8, 7), (1, 4)]],
    "mfma": [[(2048, 130), (1024, 3)], [(4096, 17), (1024, 33), (64, 5)]],
    "dropped_layers": [[(1 << 15, 3), (1 << 14, 2)], [(1 << 16, 2), (1 << 13, 4), (1 << 16, 1)]],  # trees that dropped their bottom digest layers
}


def _open_case(name, hash_kind, rc):
    rng = np.random.default_rng(99)
    rounds = [[rand_matrix(rng, h, w) for h, w in rnd] for rnd in OPEN_SHAPES[name]]
    pts = [[int(x) for x in rng.integers(1, P, 5)] for _ in range(6)]
    points = [[[pts[0]], [pts[0], pts[1], pts[2], pts[3], pts[4]]], [[pts[5], pts[0]], [pts[1]], [pts[2], pts[3], pts[4]]]]
    if name == "dropped_layers":  # fewer points: the oracle's barycentric sums are the slow part there
        points = [[[pts[0]], [pts[0], pts[1]]], [[pts[5], pts[0]], [pts[1]], [pts[2]]]]
    obs = [int(x) for x in rng.integers(0, P, 11)]
    with oracle_mmcs(hash_kind, rc):
        return rounds, points, obs, po.pcs_open(rounds, points, rc, observed=obs, num_queries=9, pow_bits=3)


@pytest.mark.parametrize("name,hash_kind", [("valu", KECCAK), ("mfma", KECCAK), ("dropped_layers", KECCAK), ("dropped_layers", POSEIDON)],
                         ids=["valu", "mfma", "dropped_layers_keccak", "dropped_layers_poseidon"])
def test_open_multi_batches(pool, rc, name, hash_kind):
    rounds, points, obs, (roots, values, proof) = ref(("open", name, hash_kind), lambda: _open_case(name, hash_kind, rc))
    p = pool.prover(num_queries=9, pow_bits=3, hash_kind=hash_kind)
    with drew_poison(p):
        pds = [p.commit_batches([p.upload(m) for m in rnd]) for rnd in rounds]
        for k, pd in enumerate(pds):
            assert first_mismatch(pd.root, roots[k]) is None
        ch = va.Challenger(rc)
        ch.observe(obs)
        opened, words = p.open_multi_batches(pds, points, ch)
        assert first_mismatch(np.concatenate([v.ravel() for rnd in opened for mat in rnd for v in mat]), values) is None
        assert first_mismatch(words, proof) is None
        if hash_kind == KECCAK:  # the product's own pcs.verify_multi_batches (host side) accepts what the device produced
            ch2 = va.Challenger(rc)
            ch2.observe(obs)
            heights, widths = [[m.shape[0] for m in rnd] for rnd in rounds], [[m.shape[1] for m in rnd] for rnd in rounds]
            assert va.verify_multi_batches([pd.root for pd in pds], heights, widths, points, opened, words, ch2, rc, num_queries=9, pow_bits=3) is None
        del pds


# ---- permutation trace, FRI fold --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chip", [0, 2, 5, 13])
def test_perm_trace(pool, fib25, chip):
    ch = np.random.default_rng(100 + chip).integers(0, P, size=15, dtype=np.uint32)
    main = fib25.main_trace(chip)
    want = ref(("perm", chip), lambda: po.perm_trace(chip, main, ch))
    p = pool.prover()
    with drew_poison(p):
        got, cs = p.generate_permutation_trace(chip, p.upload(main), ch)
        assert first_mismatch(got, want) is None
        assert first_mismatch(cs, want[-1, -5:]) is None


def test_perm_trace_long_scan(pool):
    rng = np.random.default_rng(6)
    main, ch = rand_matrix(rng, 1 << 13, 14), rng.integers(0, P, size=15, dtype=np.uint32)  # beyond one scan block and beyond one sums block
    want = ref("perm long", lambda: po.perm_trace(2, main, ch))
    p = pool.prover()
    with drew_poison(p):
        assert first_mismatch(p.generate_permutation_trace(2, p.upload(main), ch)[0], want) is None


@pytest.mark.parametrize("log_n", [2, 5, 12, 14])
def test_fri_fold(pool, log_n):
    rng = np.random.default_rng(200 + log_n)
    f, beta = rng.integers(0, P, size=(1 << log_n, 5), dtype=np.uint32), rng.integers(0, P, size=5, dtype=np.uint32)
    want = ref(("fold", log_n), lambda: po.fri_fold(f, beta))
    p = pool.prover()
    with drew_poison(p):
        assert first_mismatch(p.fri_fold(f, beta), want) is None


# ---- trace generation ---------------------------------------------------------------------------------------------------------------------------
GENERATED = {"fib25": lambda: va.Workload.fib(25), "alu1": lambda: va.Workload.alu(1), "static_data": lambda: va.Workload.named("static_data")}


@pytest.mark.parametrize("name", list(GENERATED))  # alu(1) and static_data: the padding-only and the one-row generators
def test_generated_traces(pool, name):
    w = ref(("workload", name), GENERATED[name])
    p = pool.prover()
    with drew_poison(p):
        log = p.upload_oplog(w.oplog())
        for chip in va.GENERATED_CHIPS:
            got, want = p.generate_trace(log, chip), w.main_trace(chip)
            assert got.shape == want.shape, va.CHIP_NAMES[chip]
            assert first_mismatch(got.download(), want) is None, va.CHIP_NAMES[chip]


# the padding-heavy logs of tests/oplog_corpus.py: empty and one-entry logs, one entry past a block or a power of two (the rest of the height is padding)
PADDING_LOGS = ["alu_len_0", "alu_len_1", "alu_len_257", "cpu_n1", "cpu_n257", "cpu_n4097", "pc_rom1", "pc_rom4097_sweep", "mem_n0_static0", "mem_n1_static3",
                "mem_n257_static0", "mem_n8193_static0", "out_n0", "out_n1", "static_0", "static_1"]


@pytest.mark.parametrize("case", PADDING_LOGS)
def test_generated_traces_of_padding_heavy_logs(pool, case):
    c = oc.case(case)
    p = pool.prover()
    with drew_poison(p):
        log = p.upload_oplog(c.log.desc())
        for chip in c.chips:
            want = oc.reference(case, chip)  # tests/tracegen_ref.py, computed once per case
            got = p.generate_trace(log, chip)
            assert got.shape == want.shape, (case, va.CHIP_NAMES[chip])
            assert first_mismatch(got.download(), want) is None, (case, va.CHIP_NAMES[chip])


# ---- whole proofs -------------------------------------------------------------------------------------------------------------------------------
WORKLOADS = {"fib25": lambda: va.Workload.fib(25), "alu40": lambda: va.Workload.alu(40), "static_data": lambda: va.Workload.named("static_data"),
             "fib582": lambda: va.Workload.fib(582)}
OTHER = {"fib25": "alu40", "alu40": "fib25", "static_data": "fib25", "fib582": "alu40"}  # the proof in between: a recycled block then holds another proof's data


def _workload(name, rc, hash_kind=KECCAK, log_blowup=1):
    w = ref(("workload", name), WORKLOADS[name])
    mt, prep = ref(("traces", name), lambda: (w.main_traces(), w.preprocessed()))

    def prove():
        with oracle_mmcs(hash_kind, rc):
            return po.prove_basic(mt, prep[0][1], prep[1][1], rc, log_blowup=log_blowup)
    return w, mt, prep, ref(("proof", name, hash_kind, log_blowup), prove)


def assert_the_oracles_proof(proof, want, what):
    """Located by permutation trace or quotient first, then every word."""
    for chip in range(va.NUM_CHIPS):
        assert first_mismatch(proof.debug_perm_trace(chip), want.perm_trace(chip)) is None, "%s: perm trace of chip %d (%s)" % (what, chip, va.CHIP_NAMES[chip])
    for chip in range(va.NUM_CHIPS):
        assert first_mismatch(proof.debug_quotient(chip), want.quotient(chip)) is None, "%s: quotient chunks of chip %d (%s)" % (what, chip, va.CHIP_NAMES[chip])
    assert first_mismatch(proof.words, want.words) is None, what
    assert proof.bytes() == want.bytes(), what


def twice_around_another(p, rc, name, main_of=None, **cfg):
    """The proof of `name`, a proof of another workload, the proof of `name` again: each the oracle's."""
    _, mt, prep, want = _workload(name, rc, **cfg)
    _, omt, oprep, owant = _workload(OTHER[name], rc, **cfg)
    with drew_poison(p):
        main = main_of(p) if main_of else [p.upload(m) for m in mt]
        pre = [(c, p.upload(m)) for c, m in prep]
        assert_the_oracles_proof(p.prove(main, pre, debug=True), want, name + ", first")
        assert_the_oracles_proof(p.prove(*upload(p, omt, oprep), debug=True), owant, OTHER[name] + ", in between")
        assert_the_oracles_proof(p.prove(main, pre, debug=True), want, name + ", again")


@pytest.mark.parametrize("interpret", [False, True], ids=["compiled", "interpreted"])
@pytest.mark.parametrize("name", list(WORKLOADS))
def test_proofs(pool, rc, name, interpret):
    twice_around_another(pool.prover(interpret_air=interpret), rc, name)


def test_proof_blowup4(pool, rc):
    twice_around_another(pool.prover(log_blowup=2), rc, "fib25", log_blowup=2)


def test_proof_poseidon(pool, rc):
    twice_around_another(pool.prover(hash_kind=POSEIDON), rc, "fib25", hash_kind=POSEIDON)


def test_proof_of_the_ffi_captured_machine(pool, rc):
    twice_around_another(pool.prover(ffi=True), rc, "fib25")


def test_proof_from_generated_traces(pool, rc):
    w = _workload("fib25", rc)[0]
    keep = []

    def generate(p):
        keep.append(p.upload_oplog(w.oplog()))
        return [p.generate_trace(keep[0], chip) for chip in range(va.NUM_CHIPS)]
    twice_around_another(pool.prover(), rc, "fib25", main_of=generate)


def test_proof_with_the_preprocessed_commitment_cached(pool, rc):
    p = pool.fresh()
    p.set_prep_cache(True)
    _, mt, prep, want = _workload("fib25", rc)
    with drew_poison(p):
        main, pre = upload(p, mt, prep)
        assert_the_oracles_proof(p.prove(main, pre, debug=True), want, "the miss")
        assert_the_oracles_proof(p.prove(main, pre, debug=True), want, "the hit")  # its LDEs and tree stayed live between the proofs
    twice_around_another(p, rc, "fib25")


def test_proof_of_an_edge_trace(pool, rc):
    case = {"traces": "edge_mix", "mmcs": esc.KECCAK, "log_blowup": 1}
    assert case in esc.PROOF_CASES
    want = ref("proof edge", lambda: esc.oracle_proof(case, rc))
    p = pool.prover()
    with drew_poison(p):
        assert_the_oracles_proof(p.prove(*upload(p, *esc.proof_inputs(case)), debug=True), want, esc.case_id(case))


# ---- the fifteen audits -------------------------------------------------------------------------------------------------------------------------
def _witnesses():
    fib, alu = va.Workload.fib(25), va.Workload.alu(50)
    return {"fib25": witness(fib) + (fib.program_len,), "alu50": witness(alu) + (alu.program_len,),
            "faulted": witness(fib, [(ADD, 5, 11)]) + (fib.program_len,)}  # ADD32 row 5: output byte 0 off by one (constraints and three buses notice)


def _audit_kw(name, rom_len):
    return {"rom_len": rom_len} if name == "program" else {}


def _audit_provers(pool):
    return {"basic": pool.prover(), "ffi": pool.prover(ffi=True, interpret_air=True)}


@pytest.mark.parametrize("name", AUDITS)
def test_audit(pool, name):
    """fib(25), alu(50) and a faulted fib(25), on the basic and on the interpreting FFI prover: the report of the host twin, word for word."""
    ws = ref("audit witnesses", _witnesses)
    provers = _audit_provers(pool)
    with drew_poison(*provers.values()):
        for wname, (mt, prep, rom_len) in ws.items():
            kw = _audit_kw(name, rom_len)
            host = ref(("audit", name, wname), lambda: getattr(va, name + "_audit_host")(provers["basic"].machine, mt, prep, **kw))
            for kind, p in provers.items():
                rep = getattr(p, name + "_audit")(*upload(p, mt, prep), **kw)
                assert np.array_equal(rep.words, host.words), (name, wname, kind)
                assert rep.device_ms > 0


def test_bus_audit_exact_path(pool):
    """hash_bits = 8 cuts the grouping key until tuples collide: the pass re-zeroes its counters and groups by the full tuples; the report must not change."""
    mt, prep, _ = ref("audit witnesses", _witnesses)["faulted"]
    provers = _audit_provers(pool)
    host = ref(("audit", "bus", "faulted"), lambda: va.bus_audit_host(provers["basic"].machine, mt, prep))
    assert host.total_unbalanced == 4
    with drew_poison(*provers.values()):
        for kind, p in provers.items():
            assert np.array_equal(p.bus_audit(*upload(p, mt, prep), hash_bits=8).words, host.words), kind


def test_memory_audit_planted_witnesses(pool):
    provers = _audit_provers(pool)
    mt, prep, row = ref("memory tampered", lambda: mcases.tampered("read"))
    host = ref("memory tampered host", lambda: va.memory_audit_host(provers["basic"].machine, mt, prep))
    assert host.total_findings >= 1 and host.findings[0]["row"] == row
    machine, ram = pool.prover_of("ram", mcases.ram_machine, interpret_air=True)
    with drew_poison(ram, *provers.values()):
        for kind, p in provers.items():
            assert np.array_equal(p.memory_audit(*upload(p, mt, prep)).words, host.words), kind
        for key, make, kw in (("synthetic8192", lambda: mcases.synthetic(8192), {}), ("many_findings", mcases.many_findings, {"max_findings": 64})):
            t = ref(("memory", key), make)
            h = ref(("memory host", key), lambda: va.memory_audit_host(machine, [t], [], **kw))
            assert h.total_findings > 0
            assert np.array_equal(ram.memory_audit([ram.upload(t)], [], **kw).words, h.words), key


def test_program_audit_tampered_fetch(pool):
    provers = _audit_provers(pool)
    main, prep, rom_len = ref("program tampered", lambda: pcases.vm_tampered("operand"))
    host = ref("program tampered host", lambda: va.program_audit_host(provers["basic"].machine, main, prep, rom_len=rom_len))
    assert host.words.size > 48
    with drew_poison(*provers.values()):
        for kind, p in provers.items():
            assert np.array_equal(p.program_audit(*upload(p, main, prep), rom_len=rom_len).words, host.words), kind


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_fifteen_audits_back_to_back_on_one_context(pool, order):
    """One audit's scratch is the next one's recycled block: in the order of the list and in the reverse order, the faulted witness then the clean one."""
    ws = ref("audit witnesses", _witnesses)
    p = pool.prover()
    names = AUDITS if order == "forward" else AUDITS[::-1]
    with drew_poison(p):
        for wname in ("faulted", "fib25"):
            mt, prep, rom_len = ws[wname]
            main, pre = upload(p, mt, prep)
            live = p.memory()[0]
            for name in names:
                kw = _audit_kw(name, rom_len)
                host = ref(("audit", name, wname), lambda: getattr(va, name + "_audit_host")(p.machine, mt, prep, **kw))
                assert np.array_equal(getattr(p, name + "_audit")(main, pre, **kw).words, host.words), (name, wname)
            assert p.memory()[0] == live


# ---- sharded ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_kind", [KECCAK, POSEIDON], ids=["keccak", "poseidon"])
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_commit(pool, rc, world, hash_kind):
    """tests/test_gpu_parity.py's test_sharded_commit_gives_the_single_gpu_root with every shard context poisoned, against the oracle's root."""
    provers = [pool.fresh(hash_kind=hash_kind) for _ in range(world)]
    rng = np.random.default_rng(world)
    mats = ref(("shard mats", world), lambda: [rand_matrix(rng, 1 << 10, 7), rand_matrix(rng, 1 << 12, 3), rand_matrix(rng, 1 << 10, 1), rand_matrix(rng, 64, 19),
                                               rand_matrix(rng, 2, 5), rand_matrix(rng, 1, 4), rand_matrix(rng, 1, 2)])
    shifts = ref(("shard shifts", world), lambda: [int(x) for x in rng.integers(1, P, len(mats))])
    with oracle_mmcs(hash_kind, rc):
        want = ref(("shard roots", world, hash_kind), lambda: (po.commit_root(mats), po.commit_root(mats, shifts=shifts)))
    with drew_poison(*provers):
        assert first_mismatch(va.commit_batches_sharded_local(provers, mats), want[0]) is None
        assert first_mismatch(va.commit_batches_sharded_local(provers, mats, coset_shifts=shifts), want[1]) is None


def test_sharded_proof(pool, rc):
    _, mt, prep, want = _workload("fib25", rc)
    provers = [pool.fresh() for _ in range(2)]
    with drew_poison(*provers):
        sharded = va.prove_sharded_local(provers, mt, prep, log_min_sharded=2)
        assert first_mismatch(sharded.words, want.words) is None


# ---- verifier -----------------------------------------------------------------------------------------------------------------------------------
def test_verifier_on_a_poisoned_buffer(pool, rc):
    """One proof per chunk: every chunk reuses the buffer the previous one filled, and the whole buffer is poisoned in front of each."""
    machine = pool.machine()
    _, mt, prep, want = _workload("fib25", rc)
    p = pool.prover()
    with drew_poison(p):
        words = p.prove(*upload(p, mt, prep)).words
        assert first_mismatch(words, want.words) is None
        pc = ref("prep commit fib25", lambda: va.host_commit_root([m for _, m in prep], rc))
        corpus = ref("verify corpus", lambda: vc.mutations(want.words, 50, seed=3, stride=23) + [w for _, w in vc.hostile(want.words)] + [want.words])
        host = ref("verify host", lambda: [va.verify(machine, rc, w, pc) for w in corpus])
        assert host[-1] is None and all(h is not None for h in host[:-1])
        v = va.Verifier(machine, rc)
        v.set_poison(pool.word)
        assert v.verify_batch([words], [pc]) == [None]
        v.set_chunk_words(max(w.size for w in corpus))  # one proof per chunk
        assert v.verify_batch(corpus, [pc] * len(corpus)) == host
        v.set_poison(None)
        assert v.verify_batch(corpus, [pc] * len(corpus)) == host
