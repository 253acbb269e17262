#!/usr/bin/env python3
"""The field audit's measurements (profiles/r12_field_audit.txt), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows, mem 2^22), split per kernel by the in-library profiler
    (k_fa_count.cpu, the bus-only chips k_fa_count.bus, k_fa_scan, k_fa_list), against the rank audit's device pass on the SAME trace handles
    in the same process (the rank audit's kernels are unchanged by the field audit); the aim is no slower than the rank audit's device pass;
  * the same on alu(50);
  * device audit against vgpu_field_audit_host on fib(582) (cpu 2^12 rows).

    python tools/field_audit_profile.py [--runs 3] > profiles/r12_field_audit.txt
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
    """Median device_ms over `runs` calls and the profiler's totals PER RUN {kernel: (ms, bytes, ops, launches)} over the same calls: the
    profiler accumulates a kernel's time, bytes and ops over all its launches, so these are sums over the launches of one run (mean over the
    runs), not values per launch."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, nbytes / runs, ops / runs, launches / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), reps[0], prof


def section(p, title, w, runs):
    main, pre = generate(p, w)
    fa_ms, fa, fa_prof = profiled(p, lambda: p.field_audit(main, pre), runs)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in fa.chips if c["height"] > 1)))
    ra_ms, ra, ra_prof = profiled(p, lambda: p.rank_audit(main, pre), runs)
    print("field audit: device pass %9.3f ms (median of %d; profiled runs), %d entries, %.0f dual row evaluations; floating fields %s" % (
        fa_ms, runs, fa.total_entries, fa.evaluations, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], len(fa.floating(c["chip"]))) for c in fa.chips if fa.floating(c["chip"]))))
    print("rank audit, same trace handles: device pass %9.3f ms; field / rank = %.3f (aim: <= 1)" % (ra_ms, fa_ms / ra_ms))
    print("rank audit per kernel: " + ", ".join("%s %.3f" % (k, v[0]) for k, v in sorted(ra_prof.items())))
    print("%-24s %10s %10s %16s %12s" % ("kernel", "ms per run", "launches", "dual evaluations", "ns/eval"))
    split = {"cpu": 0.0, "bus-only chips": 0.0, "other chips": 0.0, "listing": 0.0, "scan": 0.0}
    for name in sorted(fa_prof):
        ms, _, ops, launches = fa_prof[name]
        print("%-24s %10.4f %10.1f %16.0f %12.5f" % (name, ms, launches, ops, 1e6 * ms / ops if ops else float("nan")))
        key = "cpu" if name == "k_fa_count.cpu" else "bus-only chips" if name == "k_fa_count.bus" else "listing" if name == "k_fa_list" else "scan" if name == "k_fa_scan" else (
            "other chips" if name.startswith("k_fa_count") else None)
        if key:
            split[key] += ms
    print("split: " + ", ".join("%s %.3f ms" % kv for kv in split.items()))
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the C2 witness")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Field audit (vgpu_field_audit) - measurements on one MI355X; times from the in-library profiler (HIP events around each launch),")
    print("summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_field_report_timing out[0].\n" % args.runs)
    if not args.small:
        section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs)
    section(p, "alu(50)", va.Workload.alu(50), args.runs)
    w = va.Workload.fib(582)
    mt, prep = w.main_traces(), w.preprocessed()
    main_t, pre_t = [p.upload(m) for m in mt], [(c, p.upload(m)) for c, m in prep]
    p.field_audit(main_t, pre_t)
    dev = [p.field_audit(main_t, pre_t) for _ in range(args.runs)]
    host = va.field_audit_host(p.machine, mt, prep)
    assert all((d.words == host.words).all() for d in dev)
    d_ms, c_ms = statistics.median(d.device_ms for d in dev), statistics.median(d.host_ms for d in dev)
    print("== fib(582) (cpu 2^12 rows, %.0f dual row evaluations), uploaded traces, same words from both" % host.evaluations)
    print("device pass %.3f ms, whole call %.3f ms (median of %d); vgpu_field_audit_host on one core %.1f ms: %.0f x the device pass" % (d_ms, c_ms, args.runs, host.host_ms, host.host_ms / d_ms))


if __name__ == "__main__":
    main()
