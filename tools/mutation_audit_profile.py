#!/usr/bin/env python3
"""The mutation audit's measurements (profiles/r08_mutation_audit.txt), on GPU 0:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows) and on alu(50), split per chip by the in-library profiler;
  * the same witnesses through vgpu_constraint_audit, for comparison;
  * the time per Air::eval row evaluation of the two counting passes: k_ma_count.* time / evaluations performed (the profile's ops column)
    against k_ca_count.* time / rows, per chip and summed, and their ratio;
  * device audit against vgpu_mutation_audit_host on the largest fib(n) of cpu height 2^14.

    python tools/mutation_audit_profile.py [--runs 11] > profiles/r08_mutation_audit.txt
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
    """Median device_ms over `runs` calls and the profiler's mean per launch {kernel: (ms, bytes, ops)} over the same calls."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, nbytes / runs, ops / runs, launches / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), reps[0], prof


def section(p, title, w, runs):
    main, pre = generate(p, w)
    ma_ms, ma, ma_prof = profiled(p, lambda: p.mutation_audit(main, pre), runs)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in ma.chips if c["height"] > 1)))
    ca_ms, ca, ca_prof = profiled(p, lambda: p.constraint_audit(main, pre), runs)
    print("mutation audit   (deltas +1, -1): device pass %9.3f ms (median of %d; profiled runs), %d entries, %.0f row evaluations" % (ma_ms, runs, ma.total_entries, ma.evaluations))
    print("constraint audit (parent commit's kernels): device pass %9.3f ms, satisfied %s" % (ca_ms, ca.satisfied))
    print("%-24s %10s %14s %12s   | %-22s %10s %10s %12s | %s" % ("kernel", "ms", "evaluations", "ns/eval", "kernel", "ms", "rows", "ns/row", "ratio"))
    tot = [0.0, 0.0, 0.0, 0.0]
    for name in sorted(ma_prof):
        ms, _, ops, launches = ma_prof[name]
        chip = name.split(".", 1)[1] if "." in name else ""
        ca_name = "k_ca_count." + chip
        line = "%-24s %10.4f %14.0f %12.5f" % (name, ms, ops, 1e6 * ms / ops if ops else float("nan"))
        if name.startswith("k_ma_count.") and ca_name in ca_prof and ops:
            cms = ca_prof[ca_name][0]
            n = ma.chips[va.CHIP_NAMES.index(chip)]["height"]
            line += "   | %-22s %10.4f %10d %12.5f | %.3f" % (ca_name, cms, n, 1e6 * cms / n, (ms / ops) / (cms / n))
            tot = [tot[0] + ms, tot[1] + ops, tot[2] + cms, tot[3] + n]
        print(line)
    if tot[1] and tot[3]:
        print("chips with constraints, summed: %.4f ms / %.0f evaluations = %.5f ns per row evaluation; k_ca_count: %.4f ms / %d rows = %.5f ns per row; ratio %.3f (target: <= 1.0)" % (
            tot[0], tot[1], 1e6 * tot[0] / tot[1], tot[2], tot[3], 1e6 * tot[2] / tot[3], (tot[0] / tot[1]) / (tot[2] / tot[3])))
    for name in sorted(ca_prof):
        if not name.startswith("k_ca_count."):
            print("%-24s %10.4f" % (name, ca_prof[name][0]))
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=11)
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Mutation audit (vgpu_mutation_audit) - measurements on one MI355X; times from the in-library profiler (HIP events around each launch),")
    print("mean per launch over %d profiled runs after a warm-up; device pass = vgpu_mutation_report_timing out[0].\n" % args.runs)
    section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs)
    section(p, "alu(50)", va.Workload.alu(50), args.runs)
    w = va.Workload.fib(2338)
    assert w.cpu_height == 1 << 14
    mt, prep = w.main_traces(), w.preprocessed()
    main_t, pre_t = [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]
    p.mutation_audit(main_t, pre_t)
    dev = [p.mutation_audit(main_t, pre_t) for _ in range(args.runs)]
    host = [va.mutation_audit_host(p.machine, mt, prep) for _ in range(3)]
    assert all((d.words == host[0].words).all() for d in dev)
    d_ms, c_ms, h_ms = statistics.median(d.device_ms for d in dev), statistics.median(d.host_ms for d in dev), statistics.median(h.host_ms for h in host)
    print("== fib(2338) (cpu 2^14 rows, %.0f row evaluations), uploaded traces, same words from both" % dev[0].evaluations)
    print("device pass %.3f ms, whole call %.3f ms (median of %d); vgpu_mutation_audit_host on one core %.1f ms (median of 3): %.0f x the device pass" % (d_ms, c_ms, args.runs, h_ms, h_ms / d_ms))


if __name__ == "__main__":
    main()
