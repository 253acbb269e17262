#!/usr/bin/env python3
"""The product audit's measurements (profiles/product_audit.txt), on GPU 0, one session:

  * fib(582) (cpu 4096 rows, mem 16384): the device pass against the host audit on one core;
  * one tall trace: the C2 witness (fib(149794), cpu 2^20 rows), traces generated on the device, audited with chips=[cpu]: the device pass split
    by the in-library profiler into its kernels, the sweep's prefix launch (256 rows, all pairs) and survivor launch (all rows, the survivors)
    separately; the host audit of the same trace on one core unless --no-tall-host.

    python tools/product_audit_profile.py [--runs 3] [--small] [--json FILE] > profiles/product_audit.txt
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import valida_amd as va  # noqa: E402

CPU = 0


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the tall trace")
    ap.add_argument("--no-tall-host", action="store_true", help="skip the host audit of the tall trace")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Product audit (vgpu_product_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_product_report_timing out[0].\n" % args.runs)
    sections = []
    w = va.Workload.fib(582)
    main_t, pre = generate(p, w)
    p.product_audit(main_t, pre)
    dev = statistics.median(p.product_audit(main_t, pre).device_ms for _ in range(args.runs))
    host = va.product_audit_host(p.machine, w.main_traces(), w.preprocessed())
    print("== fib(582) (cpu 4096 rows, mem 16384): device pass %.3f ms, host audit on one core %.1f ms (%d relations, %.0f row evaluations)\n" % (
        dev, host.host_ms, host.total_entries, host.evaluations))
    sections.append(dict(workload="fib(582)", device_ms=dev, host_audit_ms=host.host_ms, relations=host.total_entries, host_evaluations=host.evaluations))
    if not args.small:
        w = va.Workload.fib(149794)
        main_t, pre = generate(p, w)
        ms, all_ms, rep, prof = profiled(p, lambda: p.product_audit(main_t, pre, chips=[CPU]), args.runs)
        c = rep.chips[CPU]
        print("== C2 fib(149794), traces generated on the device, chips=[cpu]: height %d, rho %d, %d pairs, %d relations" % (c["height"], c["rank"], c["pairs"], c["relations"]))
        print("device pass %9.3f ms (median of %d profiled runs: %s)" % (ms, args.runs, " ".join("%.3f" % x for x in all_ms)))
        print("%-26s %10s %10s" % ("kernel", "ms per run", "launches"))
        for name in sorted(prof):
            print("%-26s %10.4f %10.1f" % (name, prof[name][0], prof[name][1]))
        sec = dict(workload="C2 fib(149794), chips=[cpu]", device_ms=ms, runs_ms=all_ms, height=c["height"], rank=c["rank"], pairs=c["pairs"], relations=c["relations"],
                   kernels={k: dict(ms=v[0], launches=v[1]) for k, v in prof.items()},
                   sweep_prefix_ms=prof.get("k_pq_sweep.prefix", (0.0, 0))[0], sweep_survivors_ms=prof.get("k_pq_sweep.survivors", (0.0, 0))[0])
        print("sweep: prefix launch (256 rows x %d pairs) %.4f ms, survivor launch (%d rows x the survivors) %.4f ms" % (
            c["pairs"], sec["sweep_prefix_ms"], c["height"], sec["sweep_survivors_ms"]))
        if not args.no_tall_host:
            host = va.product_audit_host(p.machine, w.main_traces(), w.preprocessed(), chips=[CPU])
            assert (host.words == rep.words).all()
            print("host audit of the same trace on one core: %.1f ms (the same words)" % host.host_ms)
            sec["host_audit_ms"] = host.host_ms
        sections.append(sec)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/product_audit_profile.py", gpu="MI355X", sections=sections), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
