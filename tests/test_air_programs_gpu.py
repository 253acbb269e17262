"""Captured AIRs, device half: the scripted corpus of tests/air_script.py through every interpreter of kernels/quotient.hip on the MI355X --
k_quotient<0, 1, 2> (LDS register file, one VGPR bank, two), k_quotient_general<0, 1, 2> (log_quotient_degree 2 and 3) and
k_check_constraints<INTERPRET> -- against the oracle's scripted chip (oracle/chips.hpp), word for word.  The host half
(tests/test_air_programs_cpu.py) has run the oracle alone on every case, the same kernels' source under emulation, and every refusal: nothing
out of range is ever sent to the device here.

Cases are proven in machines of up to sixteen chips (the oracle's script slots), grouped by log_quotient_degree (log_blowup = that degree: 1 is
the product's configuration) and by whether a constraint reads a preprocessed column (a proof opens none: such a machine's honest proof is
rejected by every verifier).  Within a machine the heights 1, 2, 4, 64 rotate over the chips, so every case meets every height.
"""
import re

import numpy as np
import pytest

import air_script as A
import valida_amd as va
from conftest import first_mismatch
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
P = va.P
CASES = A.all_cases()
ACCEPTED = [n for n in CASES if n not in A.REFUSED]
FRI = dict(num_queries=5, pow_bits=4)
HEIGHTS = (1, 2, 4, 64)


def _reads_prep(s):
    return any(e[0] == "prep" for e in A._postorder(s.constraints))


def _batches():
    groups = {}
    for n in ACCEPTED:
        groups.setdefault((A.degree_py(CASES[n])[1], _reads_prep(CASES[n])), []).append(n)
    out = []
    for (lqd, pre), names in sorted(groups.items()):
        out += [(lqd, pre, names[i:i + po.NUM_SCRIPT_SLOTS]) for i in range(0, len(names), po.NUM_SCRIPT_SLOTS)]
    return out


BATCHES = _batches()
BATCH_IDS = ["lqd%d%s-%s..%s" % (q, "-prep" if pre else "", names[0], names[-1]) for q, pre, names in BATCHES]


def _bitrev(h):
    k = h.bit_length() - 1
    return np.array([int(format(r, "0%db" % k)[::-1], 2) if k else 0 for r in range(h)])


def _oracle(scripts, traces, preps, lqd, rc):
    ids = [A.set_oracle(s, slot) for slot, s in enumerate(scripts)]
    return ids, po.prove_machine(ids, traces, rc, log_blowup=lqd, prep=preps, **FRI)


def _device_stages(p, scripts, traces, preps, rc):
    """upload, commit_batches, permutation_trace_device, commit_batches, quotient -- as a host drives them (basic/src/lib.rs:185-590).
    -> ([chunk matrix per chip, downloaded], the 15 permutation challenge words)"""
    dmain = [p.upload(t) for t in traces]
    dprep = [(i, p.upload(m)) for i, m in enumerate(preps) if m is not None]
    slot = {c: k for k, (c, _) in enumerate(dprep)}
    ch = va.Challenger(rc)
    prep_pd = p.commit_batches([t for _, t in dprep]) if dprep else None
    if prep_pd is not None:
        ch.observe(prep_pd.root)
    main_pd = p.commit_batches(dmain)
    ch.observe(main_pd.root)
    rnd = ch.sample(15)
    perm, cums = [], []
    for i in range(len(scripts)):
        t, cs = p.permutation_trace_device(i, dmain[i], rnd, dprep[slot[i]][1] if i in slot else None)
        perm.append(t)
        cums.append(cs)
    perm_pd = p.commit_batches(perm)
    ch.observe(perm_pd.root)
    alpha = ch.sample(5)
    quot = [p.quotient(i, main_pd, i, perm_pd, i, rnd, alpha, cums[i], prep_pd if i in slot else None, slot.get(i, 0)).download() for i in range(len(scripts))]
    return quot, np.asarray(rnd, dtype=np.uint32)


def _compare(p, scripts, traces, preps, lqd, rc, check=False):
    """Quotient chunk matrices and proof words of the device against the oracle's; returns the proof words."""
    ids, ref = _oracle(scripts, traces, preps, lqd, rc)
    quot, rnd = _device_stages(p, scripts, traces, preps, rc)
    assert rnd.tolist() == ref.transcript[8:23].tolist()
    for i, s in enumerate(scripts):
        h = traces[i].shape[0]
        assert quot[i].shape == (h, 5 << lqd)
        bad = first_mismatch(quot[i][_bitrev(h)], ref.quotient(i).reshape(h, 5 << lqd))
        assert bad is None, "%s at height %d: %s" % (s.name, h, bad)
    proof = p.prove([p.upload(t) for t in traces], [(i, p.upload(m)) for i, m in enumerate(preps) if m is not None], check=check)
    assert first_mismatch(proof.words, ref.words) is None, [s.name for s in scripts]
    return ids, proof.words


def _preps(scripts, heights, seed=7):
    return [A.trace(seed, h, s.prep_width) if s.prep_width else None for s, h in zip(scripts, heights)]


@pytest.mark.parametrize("lqd,pre,names", BATCHES, ids=BATCH_IDS)
def test_quotient_and_proof_words_are_the_oracles(rc, lqd, pre, names):
    """Seeded (unsatisfied) traces with rows of 0, 1 and p - 1: every chip's chunk matrix equals the oracle's quotient(chip), and the proof equals
    the oracle's proof word for word -- each case at heights 1, 2, 4 and 64."""
    scripts = [CASES[n] for n in names]
    p = va.Prover(A.to_ffi(scripts), rc, log_blowup=lqd, **FRI)
    for k in range(len(HEIGHTS)):
        heights = [HEIGHTS[(i + k) % len(HEIGHTS)] for i in range(len(scripts))]
        _compare(p, scripts, [A.trace(3 + k, h, s.width) for s, h in zip(scripts, heights)], _preps(scripts, heights), lqd, rc)


@pytest.mark.parametrize("lqd,pre,names", BATCHES, ids=BATCH_IDS)
def test_satisfiable_traces_pass_the_check_and_verdicts_agree(rc, lqd, pre, names):
    """The satisfiable variant of every case: prove(check=True) passes on the witness the 0 / 1 selectors accept; the proof of the witness the
    selector polynomials accept is the oracle's and is accepted by Verifier.verify_batch exactly when va.verify accepts it (always, unless a
    constraint reads a preprocessed column); one changed cell gives a proof both reject."""
    sat = [A.satisfiable_case(n) for n in names if CASES[n].constraints]
    scripts = [c.script for c in sat]
    mach = A.to_ffi(scripts)
    p = va.Prover(mach, rc, log_blowup=lqd, **FRI)
    ver = va.Verifier(mach, rc, log_blowup=lqd, **FRI)
    for k in (0, 2):
        heights = [HEIGHTS[(i + k) % len(HEIGHTS)] for i in range(len(scripts))]
        preps = _preps(scripts, heights)
        free = [A.trace(3 + k, h, c.free_width) for c, h in zip(sat, heights)]
        boolean = [c.fill(f, m) for c, f, m in zip(sat, free, preps)]
        dprep = [(i, p.upload(m)) for i, m in enumerate(preps) if m is not None]
        p.prove([p.upload(t) for t in boolean], dprep, check=True)  # raises if k_check_constraints<INTERPRET> finds a failing row
        good = [c.fill(f, m, domain=True) for c, f, m in zip(sat, free, preps)]
        ids, words = _compare(p, scripts, good, preps, lqd, rc)
        broken = [t.copy() for t in good]
        cell = (heights[-1] // 2, sat[-1].break_col)
        broken[-1][cell] = (int(broken[-1][cell]) + 1) % P
        bad_words = p.prove([p.upload(t) for t in broken], dprep).words
        pc = va.host_commit_root([m for m in preps if m is not None], rc, log_blowup=lqd) if dprep else None
        host = [va.verify(mach, rc, w, pc, log_blowup=lqd, **FRI) for w in (words, bad_words)]
        assert ver.verify_batch([words, bad_words], [pc, pc] if dprep else None) == host
        assert host[1] is not None and (host[0] is None) == (not pre or po.verify_machine(ids, words, rc, log_blowup=lqd, prep=preps, **FRI) is None)
        assert pre or host[0] is None


KINDS = [(32, 1), (64, 1), (65, 1), (200, 1), (A.MAX_REGS_PAIR, 1), (32, 2), (64, 3), (65, 3), (200, 2), (A.MAX_REGS_GENERAL, 2)]


@pytest.mark.parametrize("regs,lqd", KINDS)
def test_each_interpreter_at_larger_heights(rc, regs, lqd):
    """One case per kernel and register-file size at heights that take more than one workgroup: 1024 rows (four workgroups of 256, the tiled
    point order and the natural-order store of k_quotient<1, 2>), and for the LDS register files 128 and 512 rows (workgroups of 128 or 64
    threads) -- the largest register files once per kernel, at 128 rows."""
    s = CASES["regs_%d_lqd%d" % (regs, lqd)]
    p = va.Prover(A.to_ffi(s), rc, log_blowup=lqd, **FRI)
    for h in ((128,) if regs >= A.MAX_REGS_PAIR else (128, 512) if regs > 64 else (1024,)):
        _compare(p, [s], [A.trace(11, h, s.width)], [None], lqd, rc)


@pytest.mark.parametrize("regs,lqd", [(32, 1), (64, 2), (65, 1), (200, 3), (A.MAX_REGS_PAIR, 1), (A.MAX_REGS_GENERAL, 2)])
def test_check_names_the_first_failing_row(rc, regs, lqd):
    """One unsatisfied witness per register-file size of k_check_constraints<INTERPRET> (256, 128 and 64 threads): two changed cells, and
    prove(check=True) names the first failing row eval_py gives."""
    s, fill, free_width, break_col = A.satisfiable_case("regs_%d_lqd%d" % (regs, lqd))
    p = va.Prover(A.to_ffi(s), rc, log_blowup=lqd, **FRI)
    h = 512 if regs <= 200 else 128
    t = fill(A.trace(5, h, free_width))
    p.prove([p.upload(t)], [], check=True)
    for r in (h - 3, h // 3):  # the later row first: the earlier one then takes over
        t[r, break_col] = (int(t[r, break_col]) + 1) % P
        want = A.first_failing_row(s, t)
        assert want == r
        with pytest.raises(va.VgpuError) as e:
            p.prove([p.upload(t)], [], check=True)
        assert re.search(r"chip %s: an AIR constraint is not satisfied on row %d$" % (re.escape(s.name), want), str(e.value)), str(e.value)


def test_a_trace_too_wide_for_the_ingest_tile_is_refused_with_a_reason(rc):
    """The ingest kernel stages 64 rows of every column in LDS: 639 columns fit.  A wider trace used to end in the launch's bare "invalid
    argument"; the launcher now refuses it on the host, before any launch, and says why.  The widest trace that fits still proves."""
    wide = A.Script("wide", 640, 0, [A.sub(A.main(639), A.main(0))])
    p = va.Prover(A.to_ffi(wide), rc, **FRI)
    with pytest.raises(va.VgpuError) as e:
        p.prove([p.upload(A.trace(1, 4, 640))], [])
    assert "ingest: a matrix of 640 columns" in str(e.value)
    fits = A.Script("fits", 639, 0, [A.sub(A.main(638), A.main(0))])
    p = va.Prover(A.to_ffi(fits), rc, **FRI)
    _compare(p, [fits], [A.trace(1, 4, 639)], [None], 1, rc)


def test_the_cases_reach_every_interpreter_and_every_opcode(rc):
    """From chip_info of the machines the tests above prove: all six interpreter instantiations (one bank up to 32 registers, two up to 64, the
    LDS file above; log_quotient_degree 1 and above), the LDS file at 128 and at 64 threads, and programs that load preprocessed columns
    (OP_LOAD_PREP: their constraint values move with the preprocessed row)."""
    reached, lds_threads = set(), set()
    for lqd, pre, names in BATCHES:
        mach = A.to_ffi([CASES[n] for n in names])
        for i in range(len(names)):
            info = mach.chip_info(i)
            assert info["log_quotient_degree"] == lqd
            if info["constraints"]:
                kind = 1 if info["registers"] <= 32 else 2 if info["registers"] <= 64 else 0
                reached.add(("k_quotient" if lqd == 1 else "k_quotient_general", kind))
                if kind == 0:
                    lds_threads.add(128 if info["registers"] <= 128 else 64)
    assert reached == {(k, r) for k in ("k_quotient", "k_quotient_general") for r in (0, 1, 2)} and lds_threads == {128, 64}
    assert {("k_quotient" if q == 1 else "k_quotient_general", 1 if r <= 32 else 2 if r <= 64 else 0) for r, q in KINDS} == reached
    loads_prep = 0
    for lqd, pre, names in BATCHES:
        for n in names if pre else []:
            s = CASES[n]
            m = A.to_ffi(s)
            z, a, b = np.zeros(s.width, np.uint32), np.full(s.prep_width, 5, np.uint32), np.full(s.prep_width, 9, np.uint32)
            loads_prep += m.eval_constraints(0, z + 3, z + 4, a, a).tolist() != m.eval_constraints(0, z + 3, z + 4, b, b).tolist()
    assert loads_prep >= 4 and sum(pre for _, pre, _ in BATCHES) >= 1
