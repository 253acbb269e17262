#!/usr/bin/env python3
"""The step audit's measurements (profiles/r14_step_audit.txt and .json), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows, mem 2^22) and on alu(50), split per kernel by the in-library
    profiler (k_sa_count.<chip>, k_ra_scan, k_sa_list);
  * against the rank audit's device pass on the SAME trace handles in the same process: the code the step audit shares its evaluation and
    elimination with and leaves unchanged.  The target is step <= 1.34 x rank (the moves add at most a third of the evaluation part); not a
    merge gate.  The per-chip ratio says which part grew;
  * fib(582): the device pass against the host audit.

    python tools/step_audit_profile.py [--runs 3] [--json profiles/r14_step_audit.json] > profiles/r14_step_audit.txt
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402

TARGET = 1.34


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


def section(p, title, w, runs):
    main, pre = generate(p, w)
    sa_ms, sa_all, sa, sa_prof = profiled(p, lambda: p.step_audit(main, pre), runs)
    ra_ms, ra_all, ra, ra_prof = profiled(p, lambda: p.rank_audit(main, pre), runs)
    for c, rc in zip(sa.chips, ra.chips):  # the cross-check that costs nothing: the directions are the rank audit's
        assert c["loose"] == rc["loose"] and c["zeros"] == rc["zeros"]
    ratio = sa_ms / ra_ms
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in sa.chips if c["height"] > 1)))
    print("step audit: device pass %9.3f ms (median of %d profiled runs: %s); %d loose cells, %d exact, %d coupled and exact; %d entries" % (
        sa_ms, runs, " ".join("%.3f" % x for x in sa_all), sum(c["loose_cells"] for c in sa.chips), sum(c["exact_cells"] for c in sa.chips),
        sum(c["coupled_exact_cells"] for c in sa.chips), sa.total_entries))
    print("rank audit, same trace handles: device pass %9.3f ms (%s)" % (ra_ms, " ".join("%.3f" % x for x in ra_all)))
    print("step / rank = %.3f (target: <= %.2f; %s)" % (ratio, TARGET, "met" if ratio <= TARGET else "MISSED"))
    print("%-26s %10s %10s %12s %8s" % ("kernel", "ms per run", "launches", "rank's ms", "ratio"))
    per_chip = {}
    for name in sorted(sa_prof):
        twin = name.replace("k_sa_", "k_ra_")
        other = ra_prof.get(twin, (0.0, 0))[0]
        per_chip[name] = dict(step_ms=sa_prof[name][0], rank_ms=other)
        print("%-26s %10.4f %10.1f %12.4f %8s" % (name, sa_prof[name][0], sa_prof[name][1], other, "%.3f" % (sa_prof[name][0] / other) if other else "-"))
    print()
    return dict(workload=title, runs=runs, step_device_ms=sa_ms, rank_device_ms=ra_ms, ratio=ratio, target=TARGET, met=ratio <= TARGET, step_runs_ms=sa_all, rank_runs_ms=ra_all,
                kernels=per_chip, loose_cells=sum(c["loose_cells"] for c in sa.chips), exact_cells=sum(c["exact_cells"] for c in sa.chips), entries=sa.total_entries)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the C2 witness")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Step audit (vgpu_step_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each launch),")
    print("summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_*_report_timing out[0].\n" % args.runs)
    sections = []
    if not args.small:
        sections.append(section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs))
    sections.append(section(p, "alu(50)", va.Workload.alu(50), args.runs))
    w = va.Workload.fib(582)
    main_t, pre = generate(p, w)
    p.step_audit(main_t, pre)
    dev = statistics.median(p.step_audit(main_t, pre).device_ms for _ in range(args.runs))
    host = va.step_audit_host(p.machine, w.main_traces(), w.preprocessed())
    print("== fib(582) (cpu 4096 rows, mem 16384): device pass %.3f ms, host audit %.1f ms (%.0f row evaluations)" % (dev, host.host_ms, host.evaluations))
    sections.append(dict(workload="fib(582)", step_device_ms=dev, host_audit_ms=host.host_ms, host_evaluations=host.evaluations))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/step_audit_profile.py", gpu="MI355X", sections=sections), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
