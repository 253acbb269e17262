#!/usr/bin/env python3
"""The link audit's measurements (profiles/r13_link_audit.txt and .json), on GPU 0, one session:

  * the device pass on the clean C2 witness (fib(149794), cpu 2^20 rows, mem 2^22) and on alu(50), split per kernel by the in-library
    profiler: the masks per chip class (k_la_masks.native / .bus / .interpret), the bus audit's records / sort / groups / reduce, join, tally
    and the report (select, its sort, k_la_report);
  * against the field audit's device pass PLUS the bus audit's device pass on the SAME trace handles in the same process.  Both are the code
    the link audit is built from and leaves unchanged; the aim is link <= 1.05 x (field + bus).  It is never the link audit against itself.

    python tools/link_audit_profile.py [--runs 3] [--json profiles/r13_link_audit.json] > profiles/r13_link_audit.txt
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402

GROUPS = (("masks, compiled chips", ("k_la_masks.native",)), ("masks, bus-only chips", ("k_la_masks.bus",)), ("masks, interpreted chips", ("k_la_masks.interpret",)),
          ("records", ("k_ba_records",)), ("sort", ("k_ba_sort",)), ("groups", ("k_ba_groups",)), ("reduce", ("k_ba_reduce",)), ("exact path", ("k_ba_exact_keys",)),
          ("join", ("k_la_join",)), ("tally", ("k_la_tally",)), ("report", ("k_la_select", "k_la_report")))


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def profiled(p, call, runs):
    """Median device_ms over `runs` calls and the profiler's totals PER RUN {kernel: (ms, launches)} over the same calls (sums over the
    launches of one run, mean over the runs)."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, launches / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), [r.device_ms for r in reps], reps[0], prof


def section(p, title, w, runs):
    main, pre = generate(p, w)
    la_ms, la_all, la, la_prof = profiled(p, lambda: p.link_audit(main, pre), runs)
    fa_ms, fa_all, fa, _ = profiled(p, lambda: p.field_audit(main, pre), runs)
    ba_ms, ba_all, ba, _ = profiled(p, lambda: p.bus_audit(main, pre), runs)
    for c, fc in zip(la.chips, fa.chips):  # the cross-check that costs nothing
        assert [r["floating"] for r in c["records"]] == [r["floating"] for r in fc["records"]]
    ratio = la_ms / (fa_ms + ba_ms)
    print("== %s: heights %s" % (title, " ".join("%s %d" % (va.CHIP_NAMES[c["chip"]], c["height"]) for c in fa.chips if c["height"] > 1)))
    print("link audit: device pass %9.3f ms (median of %d profiled runs: %s); %d live records, %d tuples, %d open" % (
        la_ms, runs, " ".join("%.3f" % x for x in la_all), sum(b["live"] for b in la.buses), sum(b["tuples"] for b in la.buses), la.open_tuples))
    print("field audit, same trace handles: device pass %9.3f ms (%s)" % (fa_ms, " ".join("%.3f" % x for x in fa_all)))
    print("bus audit, same trace handles:   device pass %9.3f ms (%s)" % (ba_ms, " ".join("%.3f" % x for x in ba_all)))
    print("link / (field + bus) = %.3f (aim: <= 1.05)" % ratio)
    print("%-26s %10s %10s" % ("kernel", "ms per run", "launches"))
    for name in sorted(la_prof):
        print("%-26s %10.4f %10.1f" % (name, la_prof[name][0], la_prof[name][1]))
    split = {g: sum(la_prof[k][0] for k in names if k in la_prof) for g, names in GROUPS}
    # the report's sort of the open tuples runs under the same profiler name as the records' sort
    print("split: " + ", ".join("%s %.3f ms" % kv for kv in split.items() if kv[1]))
    print()
    return dict(workload=title, runs=runs, link_device_ms=la_ms, field_device_ms=fa_ms, bus_device_ms=ba_ms, ratio=ratio, aim=1.05, met=ratio <= 1.05, link_runs_ms=la_all,
                field_runs_ms=fa_all, bus_runs_ms=ba_all, live_records=sum(b["live"] for b in la.buses), tuples=sum(b["tuples"] for b in la.buses), open_tuples=la.open_tuples,
                kernels_ms_per_run={k: v[0] for k, v in sorted(la_prof.items())}, split_ms=split)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the C2 witness")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Link audit (vgpu_link_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each launch),")
    print("summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_*_report_timing out[0].\n" % args.runs)
    sections = []
    if not args.small:
        sections.append(section(p, "C2 fib(149794), traces generated on the device", va.Workload.fib(149794), args.runs))
    sections.append(section(p, "alu(50)", va.Workload.alu(50), args.runs))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/link_audit_profile.py", gpu="MI355X", sections=sections), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
