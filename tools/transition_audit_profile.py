#!/usr/bin/env python3
"""The transition audit's measurements (profiles/transition_audit.txt), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows, mem 2^22), on alu(50) and on fib(582), split by the in-library
    profiler into flags (k_ta_flags), phase 1 (k_ta_basis), merge (k_ta_merge), phase 2 (k_ta_enforce.<chip>) and count / scan / list;
  * against the invariant audit's device pass on the SAME trace handles in the same process: the audit whose streaming elimination and
    enforcement sweep this one extends to two-row windows and gates.  No target is fixed: the ratio and the kernel that carries it are what
    the file states.

    python tools/transition_audit_profile.py [--runs 3] [--small] [--json FILE] > profiles/transition_audit.txt
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402


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

    return dict(flags_ms=total(lambda k: k == "k_ta_flags"), phase1_ms=total(lambda k: k == "k_ta_basis"), merge_ms=total(lambda k: k == "k_ta_merge"),
                phase2_ms=total(lambda k: k.startswith("k_ta_enforce")), listing_ms=total(lambda k: k in ("k_ta_count", "k_ta_scan", "k_ta_list")))


def section(p, title, w, runs):
    main, pre = generate(p, w)
    ta_ms, ta_all, ta, ta_prof = profiled(p, lambda: p.transition_audit(main, pre), runs)
    ia_ms, ia_all, ia, ia_prof = profiled(p, lambda: p.invariant_audit(main, pre), runs)
    ratio = ta_ms / ia_ms
    parts = split(ta_prof)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in ta.chips if c["height"] > 1)))
    print("transition audit: device pass %9.3f ms (median of %d profiled runs: %s); %d gates audited of %d, %d entries (%d listed and judged): %d transition relations, %d gated" % (
        ta_ms, runs, " ".join("%.3f" % x for x in ta_all), sum(c["gates_audited"] for c in ta.chips), sum(c["n_gates"] for c in ta.chips), ta.total_entries, ta.reported,
        sum(c["transitions"] for c in ta.chips), sum(c["gated"] for c in ta.chips)))
    print("  split (kernel time): flags %.3f ms, phase 1 %.3f ms, merge %.3f ms, phase 2 %.3f ms, count / scan / list %.3f ms" % (
        parts["flags_ms"], parts["phase1_ms"], parts["merge_ms"], parts["phase2_ms"], parts["listing_ms"]))
    print("invariant audit, same trace handles: device pass %9.3f ms (%s)" % (ia_ms, " ".join("%.3f" % x for x in ia_all)))
    carrier = max(ta_prof, key=lambda k: ta_prof[k][0])
    print("transition / invariant = %.3f; the largest kernel: %s, %.3f ms per run" % (ratio, carrier, ta_prof[carrier][0]))
    print("%-28s %10s %10s" % ("kernel", "ms per run", "launches"))
    per_kernel = {}
    for name in sorted(ta_prof):
        per_kernel[name] = dict(ms=ta_prof[name][0], launches=ta_prof[name][1])
        print("%-28s %10.4f %10.1f" % (name, ta_prof[name][0], ta_prof[name][1]))
    print()
    sys.stdout.flush()
    return dict(workload=title, runs=runs, transition_device_ms=ta_ms, invariant_device_ms=ia_ms, ratio=ratio, carrier=carrier, transition_runs_ms=ta_all, invariant_runs_ms=ia_all,
                kernels=per_kernel, entries=ta.total_entries, listed=ta.reported, **parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the C2 witness")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Transition audit (vgpu_transition_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_*_report_timing out[0].\n" % args.runs)
    sections = [section(p, "alu(50)", va.Workload.alu(50), args.runs), section(p, "fib(582)", va.Workload.fib(582), args.runs)]
    if not args.small:
        sections.append(section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/transition_audit_profile.py", gpu="MI355X", sections=sections), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
