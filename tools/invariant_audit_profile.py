#!/usr/bin/env python3
"""The invariant audit's measurements (profiles/invariant_audit.txt), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows, mem 2^22), split by the in-library profiler into phase 1 (k_ia_basis),
    merge (k_ia_merge), phase 2 (k_ia_count.<chip>) and listing (k_ra_scan, k_ia_list);
  * against the rank audit's device pass on the SAME trace handles in the same process: the code the invariant audit shares its evaluation and
    elimination with and leaves unchanged.  The expectation is invariant <= 1.5 x rank; not a merge gate.  The per-chip ratio of phase 2 to
    the rank audit's counting kernel says which part grew;
  * fib(582): the device pass against the host audit on one core.

    python tools/invariant_audit_profile.py [--runs 3] [--json FILE] > profiles/invariant_audit.txt
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402

TARGET = 1.5


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def profiled(p, call, runs):
    """Median device_ms over `runs` calls and the profiler's totals PER RUN {kernel: (ms, launches)} over the same calls."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, launches / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), [r.device_ms for r in reps], reps[0], prof


def split(prof):
    def total(keep):
        return sum(ms for k, (ms, _) in prof.items() if keep(k))

    return dict(phase1_ms=total(lambda k: k == "k_ia_basis"), merge_ms=total(lambda k: k == "k_ia_merge"), phase2_ms=total(lambda k: k.startswith("k_ia_count")),
                listing_ms=total(lambda k: k in ("k_ra_scan", "k_ia_list")))


def section(p, title, w, runs):
    main, pre = generate(p, w)
    ia_ms, ia_all, ia, ia_prof = profiled(p, lambda: p.invariant_audit(main, pre), runs)
    ra_ms, ra_all, ra, ra_prof = profiled(p, lambda: p.rank_audit(main, pre), runs)
    ratio = ia_ms / ra_ms
    parts = split(ia_prof)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in ia.chips if c["height"] > 1)))
    print("invariant audit: device pass %9.3f ms (median of %d profiled runs: %s); %d invariants, %d relations; enforced on every row %d, on some %d, on none %d" % (
        ia_ms, runs, " ".join("%.3f" % x for x in ia_all), ia.total_entries, sum(c["relations"] for c in ia.chips), sum(c["every"] for c in ia.chips),
        sum(c["some"] for c in ia.chips), sum(c["never"] for c in ia.chips)))
    print("  split (kernel time): phase 1 %.3f ms, merge %.3f ms, phase 2 %.3f ms, listing %.3f ms" % (parts["phase1_ms"], parts["merge_ms"], parts["phase2_ms"], parts["listing_ms"]))
    print("rank audit, same trace handles: device pass %9.3f ms (%s)" % (ra_ms, " ".join("%.3f" % x for x in ra_all)))
    print("invariant / rank = %.3f (expectation: <= %.2f; %s)" % (ratio, TARGET, "met" if ratio <= TARGET else "MISSED"))
    print("%-26s %10s %10s %12s %8s" % ("kernel", "ms per run", "launches", "rank's ms", "ratio"))
    per_kernel = {}
    for name in sorted(ia_prof):
        twin = name.replace("k_ia_count", "k_ra_count")
        other = ra_prof.get(twin, (0.0, 0))[0] if twin != name else 0.0
        per_kernel[name] = dict(invariant_ms=ia_prof[name][0], launches=ia_prof[name][1], rank_ms=other)
        print("%-26s %10.4f %10.1f %12.4f %8s" % (name, ia_prof[name][0], ia_prof[name][1], other, "%.3f" % (ia_prof[name][0] / other) if other else "-"))
    print()
    return dict(workload=title, runs=runs, invariant_device_ms=ia_ms, rank_device_ms=ra_ms, ratio=ratio, target=TARGET, met=ratio <= TARGET, invariant_runs_ms=ia_all, rank_runs_ms=ra_all,
                kernels=per_kernel, invariants=ia.total_entries, **parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the C2 witness")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Invariant audit (vgpu_invariant_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_*_report_timing out[0].\n" % args.runs)
    sections = []
    if not args.small:
        sections.append(section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs))
    sections.append(section(p, "alu(50)", va.Workload.alu(50), args.runs))
    w = va.Workload.fib(582)
    main_t, pre = generate(p, w)
    p.invariant_audit(main_t, pre)
    dev = statistics.median(p.invariant_audit(main_t, pre).device_ms for _ in range(args.runs))
    host = va.invariant_audit_host(p.machine, w.main_traces(), w.preprocessed())
    print("== fib(582) (cpu 4096 rows, mem 16384): device pass %.3f ms, host audit on one core %.1f ms (%.0f row evaluations)" % (dev, host.host_ms, host.evaluations))
    sections.append(dict(workload="fib(582)", invariant_device_ms=dev, host_audit_ms=host.host_ms, host_evaluations=host.evaluations))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/invariant_audit_profile.py", gpu="MI355X", sections=sections), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
