#!/usr/bin/env python3
"""The domain audit's measurements (profiles/domain_audit.txt), on GPU 0, one session:

  * fib(582) (cpu 4096 rows, mem 16384), traces generated on the device;
  * one tall trace: the C2 witness (fib(149794), cpu 2^20 rows), traces generated on the device;

each after a warm-up, three runs with the in-library profiler: the device pass split into its kernels, beside the host audit's wall time on the
same inputs (one core); for k_da_scan on the tall trace the achieved bytes/s (4 bytes per scanned cell: every cell a virtual column reads, the
count's included) against the measured copy ceiling.  The kernels' registers, scratch and occupancy are read from the compiler's resource-usage
remarks when hipcc is on the path.

    python tools/domain_audit_profile.py [--runs 3] [--small] [--no-tall-host] [--json FILE] > profiles/domain_audit.txt
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import valida_amd as va  # noqa: E402

COPY_CEILING = 6.3e12  # bytes/s, the measured device-to-device copy ceiling of one MI355X


def generate(p, w):
    log = p.upload_oplog(w.oplog())
    return [p.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)], [(c, p.upload(m)) for c, m in w.preprocessed()]


def profiled(p, call, runs):
    """Median device_ms over `runs` calls and the profiler's totals PER RUN {kernel: (ms, launches, bytes)} over the same calls."""
    call()  # warm-up: code objects, the pool
    p.set_profiling(True)
    reps = [call() for _ in range(runs)]
    prof = {k: (ms / runs, launches / runs, nbytes / runs) for k, (launches, ms, nbytes, ops) in p.profile().items()}
    p.set_profiling(False)
    return statistics.median(r.device_ms for r in reps), [r.device_ms for r in reps], reps[0], prof


def scanned_bytes(machine, w):
    """4 bytes per cell the scan reads: per main column one per row, per field vcol its terms' and its count's."""
    total = 0
    for chip, t in enumerate(w.main_traces()):
        n = t.shape[0]
        total += 4 * n * t.shape[1]
        for it in machine.interactions(chip):
            for f in it["fields"]:
                total += 4 * n * (len(it["count"][1]) + len(f[1]))
    return total


def resource_usage():
    """[(kernel, vgprs, sgprs, scratch, occupancy, lds)] from hipcc's kernel-resource-usage remarks of kernels/domain_audit.hip, or None."""
    src = os.path.join(ROOT, "valida_amd", "csrc", "kernels", "domain_audit.hip")
    try:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-c", src, "-o", os.devnull, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired):
        return None
    out, cur = [], None
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = dict(name=m.group(1))
            out.append(cur)
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    return [k for k in out if "k_da_" in k["name"]] or None


def section(p, name, w, runs, host):
    main_t, pre = generate(p, w)
    ms, all_ms, rep, prof = profiled(p, lambda: p.domain_audit(main_t, pre), runs)
    heights = {va.CHIP_NAMES[c["chip"]]: c["height"] for c in rep.chips}
    print("== %s, traces generated on the device: cpu %d rows, mem %d rows; %d entries, %.0f cells scanned" % (name, heights["cpu"], heights["mem"], rep.total_entries, rep.evaluations))
    print("device pass %9.3f ms (median of %d profiled runs: %s)" % (ms, runs, " ".join("%.3f" % x for x in all_ms)))
    print("%-16s %10s %10s" % ("kernel", "ms per run", "launches"))
    for k in sorted(prof):
        print("%-16s %10.4f %10.1f" % (k, prof[k][0], prof[k][1]))
    sec = dict(workload=name, device_ms=ms, runs_ms=all_ms, heights=heights, entries=rep.total_entries, cells=rep.evaluations,
               kernels={k: dict(ms=v[0], launches=v[1]) for k, v in prof.items()})
    if "k_da_scan" in prof and prof["k_da_scan"][0] > 0:
        nbytes = scanned_bytes(p.machine, w)
        rate = nbytes / (prof["k_da_scan"][0] * 1e-3)
        print("k_da_scan: %.1f MB read in %.4f ms = %.3f TB/s, %.1f %% of the %.1f TB/s copy ceiling" % (nbytes / 1e6, prof["k_da_scan"][0], rate / 1e12, 100 * rate / COPY_CEILING, COPY_CEILING / 1e12))
        sec.update(scan_bytes=nbytes, scan_bytes_per_s=rate)
    if host:
        h = va.domain_audit_host(p.machine, w.main_traces(), w.preprocessed())
        assert (h.words == rep.words).all()
        print("host audit of the same traces on one core: %.1f ms (the same words)" % h.host_ms)
        sec["host_audit_ms"] = h.host_ms
    print()
    return sec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="skip the tall trace")
    ap.add_argument("--no-tall-host", action="store_true", help="skip the host audit of the tall trace")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Domain audit (vgpu_domain_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_domain_report_timing out[0].\n" % args.runs)
    sections = [section(p, "fib(582)", va.Workload.fib(582), args.runs, True)]
    if not args.small:
        sections.append(section(p, "C2 fib(149794)", va.Workload.fib(149794), args.runs, not args.no_tall_host))
    usage = resource_usage()
    if usage:
        print("== kernels/domain_audit.hip for gfx950 (hipcc -O3, kernel-resource-usage remarks)")
        print("%-16s %6s %6s %16s %16s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "waves per SIMD", "static LDS B"))
        for k in usage:
            print("%-16s %6s %6s %16s %16s %12s" % (re.search(r"k_da_[a-z]+", k["name"]).group(0), k.get("vgprs", "?"), k.get("sgprs", "?"), k.get("scratch", "?"),
                                                    k.get("occupancy", "?"), k.get("lds", "?")))
        print("(dynamic LDS per workgroup of 256 threads: k_da_scan 9328 bytes, k_da_classify 1088, k_da_guard 4 x (table + 5 w + appearances + 280))")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/domain_audit_profile.py", gpu="MI355X", sections=sections, kernels=usage), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
