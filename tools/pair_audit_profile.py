#!/usr/bin/env python3
"""The pair audit's measurements (profiles/r10_pair_audit.txt), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows) and on alu(50), split per chip by the in-library profiler;
  * the time per Air::eval row evaluation of the counting pass, k_pa_count.* time / evaluations performed (the profile's ops column), against
    the mutation audit's k_ma_count.* time / evaluations on the same witness in the same session (the mutation audit's kernels are unchanged
    by the pair audit), per chip and summed, and their ratio (target: at most 1.5);
  * device audit against vgpu_pair_audit_host on fib(582) (cpu 2^12 rows).

    python tools/pair_audit_profile.py [--runs 5] > profiles/r10_pair_audit.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def profiled(p, call, runs):
    """Median device_ms over `runs` calls and the profiler's mean per launch {kernel: (ms, bytes, ops, launches)} over the same calls."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, nbytes / runs, ops / runs, launches / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), reps[0], prof


def section(p, title, w, runs):
    main, pre = generate(p, w)
    pa_ms, pa, pa_prof = profiled(p, lambda: p.pair_audit(main, pre), runs)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in pa.chips if c["height"] > 1)))
    ma_ms, ma, ma_prof = profiled(p, lambda: p.mutation_audit(main, pre), runs)
    print("pair audit     (deltas +1, -1): device pass %9.3f ms (median of %d; profiled runs), %d entries, %.0f row evaluations; slack pairs %s" % (
        pa_ms, runs, pa.total_entries, pa.evaluations, " ".join("%s %d/%d" % (va.CHIP_NAMES[c["chip"]], c["slack"], c["coupled"]) for c in pa.chips if c["slack"])))
    print("mutation audit (deltas +1, -1): device pass %9.3f ms, %.0f row evaluations" % (ma_ms, ma.evaluations))
    print("%-24s %10s %14s %12s   | %-24s %10s %14s %12s | %s" % ("kernel", "ms", "evaluations", "ns/eval", "kernel", "ms", "evaluations", "ns/eval", "ratio"))
    tot = [0.0, 0.0, 0.0, 0.0]
    for name in sorted(pa_prof):
        ms, _, ops, launches = pa_prof[name]
        chip = name.split(".", 1)[1] if "." in name else ""
        ma_name = "k_ma_count." + chip
        line = "%-24s %10.4f %14.0f %12.5f" % (name, ms, ops, 1e6 * ms / ops if ops else float("nan"))
        if name.startswith("k_pa_count.") and ma_name in ma_prof and ops and ma_prof[ma_name][2]:
            mms, _, mops, _ = ma_prof[ma_name]
            line += "   | %-24s %10.4f %14.0f %12.5f | %.3f" % (ma_name, mms, mops, 1e6 * mms / mops, (ms / ops) / (mms / mops))
            tot = [tot[0] + ms, tot[1] + ops, tot[2] + mms, tot[3] + mops]
        print(line)
    if tot[1] and tot[3]:
        print("chips with constraints, summed: %.4f ms / %.0f evaluations = %.5f ns per row evaluation; k_ma_count: %.4f ms / %.0f evaluations = %.5f ns; ratio %.3f (target: <= 1.5)" % (
            tot[0], tot[1], 1e6 * tot[0] / tot[1], tot[2], tot[3], 1e6 * tot[2] / tot[3], (tot[0] / tot[1]) / (tot[2] / tot[3])))
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Pair audit (vgpu_pair_audit) - measurements on one MI355X; times from the in-library profiler (HIP events around each launch),")
    print("mean per launch over %d profiled runs after a warm-up; device pass = vgpu_pair_report_timing out[0].\n" % args.runs)
    section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs)
    section(p, "alu(50)", va.Workload.alu(50), args.runs)
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    main_t, pre_t = [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]
    p.pair_audit(main_t, pre_t)
    dev = [p.pair_audit(main_t, pre_t) for _ in range(args.runs)]
    host = va.pair_audit_host(p.machine, mt, prep)
    assert all((d.words == host.words).all() for d in dev)
    d_ms, c_ms = statistics.median(d.device_ms for d in dev), statistics.median(d.host_ms for d in dev)
    print("== fib(582) (cpu 2^12 rows, %.0f row evaluations on the device, %.0f on the host), uploaded traces, same words from both" % (dev[0].evaluations, host.evaluations))
    print("device pass %.3f ms, whole call %.3f ms (median of %d); vgpu_pair_audit_host on one core %.1f ms: %.0f x the device pass" % (d_ms, c_ms, args.runs, host.host_ms, host.host_ms / d_ms))


if __name__ == "__main__":
    main()
