#!/usr/bin/env python3
"""The coverage audit's measurements (profiles/r09_coverage_audit.txt), on GPU 0:

  * c2        the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows), split per chip by the in-library profiler, INTERLEAVED with
              the mutation audit on the same trace handles in one process (the yardstick: k_ma_count.* against k_cov_audit.*, same
              evaluations), and the native-to-interpreted ratio of the coverage pass;
  * fib2338   the same interleaved comparison on the largest fib(n) of cpu height 2^14, and the device pass against
              vgpu_coverage_audit_host (same words from both).

Every step runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the run (nothing more
is started on the GPU after a failure).

    python tools/coverage_audit_profile.py [--runs 11] > profiles/r09_coverage_audit.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = (("c2", 240), ("fib2338", 120))  # (step, seconds)


def generate(va, p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def interleaved(va, p, main, pre, runs):
    """`runs` rounds of (mutation audit, coverage audit) on the same handles after a warm-up of each: the medians of the two device passes,
    the first reports and the profiler's mean per launch {kernel: (ms, ops)}."""
    p.mutation_audit(main, pre)
    p.coverage_audit(main, pre)
    p.set_profiling(True)
    ma, cov = [], []
    for _ in range(runs):
        ma.append(p.mutation_audit(main, pre))
        cov.append(p.coverage_audit(main, pre))
    prof = {k: (ms / runs, ops / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in ma), statistics.median(r.device_ms for r in cov), ma[0], cov[0], prof


def table(va, title, ma_ms, cov_ms, ma, cov, prof, runs):
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in cov.chips if c["height"] > 1)))
    print("mutation audit (parent commit's kernels): device pass %9.3f ms (median of %d, interleaved), %.0f row evaluations" % (ma_ms, runs, ma.evaluations))
    print("coverage audit                          : device pass %9.3f ms, %d cells, %.0f row evaluations" % (cov_ms, cov.total_cells, cov.evaluations))
    print("%-26s %10s %14s %12s   | %-24s %10s %14s %12s | %s" % ("kernel", "ms", "evaluations", "ns/eval", "yardstick", "ms", "evaluations", "ns/eval", "ratio"))
    tot = [0.0, 0.0, 0.0, 0.0]
    for name in sorted(prof):
        if not name.startswith("k_cov_"):
            continue
        ms, ops = prof[name]
        line = "%-26s %10.4f %14.0f %12.5f" % (name, ms, ops, 1e6 * ms / ops if ops else float("nan"))
        ya = "k_ma_count." + name.split(".", 1)[1] if "." in name else ""
        if ya in prof:
            yms, yops = prof[ya]
            line += "   | %-24s %10.4f %14.0f %12.5f | time %.3f" % (ya, yms, yops, 1e6 * yms / yops if yops else float("nan"), ms / yms)
            if ops and yops:
                line += ", per evaluation %.3f" % ((ms / ops) / (yms / yops))
                tot = [tot[0] + ms, tot[1] + ops, tot[2] + yms, tot[3] + yops]
        print(line)
    for name in ("k_ma_scan", "k_ma_list"):
        if name in prof:
            print("%-26s %10s %14s %12s   | %-24s %10.4f" % ("", "", "", "", name, prof[name][0]))
    if tot[1] and tot[3]:
        print("chips with constraints, summed: coverage %.4f ms / %.0f evaluations, mutation counting %.4f ms / %.0f: time ratio %.3f, per evaluation %.3f" % (
            tot[0], tot[1], tot[2], tot[3], tot[0] / tot[2], (tot[0] / tot[1]) / (tot[2] / tot[3])))
    print()


def step_c2(va, runs):
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    w = va.Workload.fib(149794)
    assert w.cpu_height == 1 << 20
    main, pre = generate(va, p, w)
    ma_ms, cov_ms, ma, cov, prof = interleaved(va, p, main, pre, runs)
    assert [c["free"] for c in cov.chips] == [c["free"] for c in ma.chips]
    table(va, "C2 fib(149794), traces generated on the device", ma_ms, cov_ms, ma, cov, prof, runs)
    q = va.Prover(va.Machine.basic_via_ffi(), va.poseidon_round_constants(), device=0, interpret_air=True)
    q.coverage_audit(main, pre)
    ffi = [q.coverage_audit(main, pre) for _ in range(3)]
    assert all((f.words == cov.words).all() for f in ffi)
    i_ms = statistics.median(f.device_ms for f in ffi)
    print("C2 interpreted (captured AIRs, the register program): device pass %.3f ms (median of 3), same words; %.2f x the native pass\n" % (i_ms, i_ms / cov_ms))


def step_fib2338(va, runs):
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    w = va.Workload.fib(2338)
    assert w.cpu_height == 1 << 14
    mt, prep = w.main_traces(), w.preprocessed()
    main, pre = [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]
    ma_ms, cov_ms, ma, cov, prof = interleaved(va, p, main, pre, runs)
    table(va, "fib(2338) (cpu 2^14 rows), uploaded traces", ma_ms, cov_ms, ma, cov, prof, runs)
    host = [va.coverage_audit_host(p.machine, mt, prep) for _ in range(3)]
    assert (cov.words == host[0].words).all()
    h_ms = statistics.median(h.host_ms for h in host)
    print("fib(2338): device pass %.3f ms; vgpu_coverage_audit_host on one core %.1f ms (median of 3), same words: %.0f x the device pass\n" % (cov_ms, h_ms, h_ms / cov_ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        import valida_amd as va

        {"c2": step_c2, "fib2338": step_fib2338}[args.step](va, args.runs)
        return 0
    print("Coverage audit (vgpu_coverage_audit) - measurements on one MI355X; times from the in-library profiler (HIP events around each launch),")
    print("mean per launch over %d profiled runs after a warm-up, the mutation audit and the coverage audit alternating in one process.\n" % args.runs, flush=True)
    for step, seconds in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--runs", str(args.runs)], timeout=seconds)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s: stopping" % (step, seconds))
            return 1
        if r.returncode != 0:
            print("step %s failed with status %d: stopping" % (step, r.returncode))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
