#!/usr/bin/env python3
"""The memory audit's measurements (profiles/memory_audit.txt), on GPU 0, one session:

  * fib(582) (mem 16384 rows), traces generated on the device;
  * one tall trace: the C2 witness (fib(149794), mem 2^22 rows), traces generated on the device;

each after a warm-up, three runs with the in-library profiler: the device pass split into its kernels, beside the host audit's wall time on the
same inputs (one core, the same words); for the sort the bytes its passes move (per pass and pair 8 bytes of key read for the histogram, 12 read
and 12 written by the scatter) against the measured copy ceiling.  The kernels' registers, scratch and occupancy are read from the compiler's
resource-usage remarks when hipcc is on the path.

    python tools/memory_audit_profile.py [--runs 3] [--small] [--no-tall-host] [--commit ID] [--json FILE] > profiles/memory_audit.txt
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
MEM = 2


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


def sort_passes(t):
    """The radix passes of a witness: the key bytes in which some live key differs, and the top byte when a slot is dead (host/memory_audit.hpp)."""
    c = t.counters
    if not c["live"]:
        return 0
    # the report does not carry the keys: an upper bound from the ranges (addr bytes that can differ, clk bytes up to max_clk, the static bit)
    addr = c["min_addr"] ^ c["max_addr"]
    bits = (((1 << addr.bit_length()) - 1) << 32) | ((1 << (c["max_clk"].bit_length() + 1)) - 1)
    return sum(1 for b in range(8) if (bits >> (8 * b)) & 0xFF or (b == 7 and c["live"] < c["slots"]))


def resource_usage():
    """[(kernel, vgprs, sgprs, scratch, occupancy, lds)] from hipcc's kernel-resource-usage remarks of kernels/memory_audit.hip, or None."""
    src = os.path.join(ROOT, "valida_amd", "csrc", "kernels", "memory_audit.hip")
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
    return [k for k in out if "k_mm_" in k["name"]] or None


def section(p, name, w, runs, host):
    main_t, pre = generate(p, w)
    ms, all_ms, rep, prof = profiled(p, lambda: p.memory_audit(main_t, pre), runs)
    c = rep.counters
    print("== %s, traces generated on the device: mem %d rows; %d live records, %d addresses, %d findings" % (name, c["slots"], c["live"], c["addresses"], c["findings"]))
    print("device pass %9.3f ms (median of %d profiled runs: %s)" % (ms, runs, " ".join("%.3f" % x for x in all_ms)))
    print("%-16s %10s %10s" % ("kernel", "ms per run", "launches"))
    for k in sorted(prof):
        print("%-16s %10.4f %10.1f" % (k, prof[k][0], prof[k][1]))
    sec = dict(workload=name, device_ms=ms, runs_ms=all_ms, counters=c, kernels={k: dict(ms=v[0], launches=v[1], bytes=v[2]) for k, v in prof.items()})
    if "k_ba_sort" in prof and prof["k_ba_sort"][0] > 0:
        nbytes = prof["k_ba_sort"][2]  # the launcher's own account: 32 bytes per pair and pass
        rate = nbytes / (prof["k_ba_sort"][0] * 1e-3)
        print("k_ba_sort: %d passes over %d slots (at most %d key bytes differ by the ranges), %.1f MB moved in %.4f ms = %.3f TB/s, %.1f %% of the %.1f TB/s copy ceiling" % (
            round(nbytes / (32.0 * c["slots"])), c["slots"], sort_passes(rep), nbytes / 1e6, prof["k_ba_sort"][0], rate / 1e12, 100 * rate / COPY_CEILING, COPY_CEILING / 1e12))
        sec.update(sort_bytes=nbytes, sort_bytes_per_s=rate)
    if host:
        h = va.memory_audit_host(p.machine, w.main_traces(), w.preprocessed())
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
    ap.add_argument("--commit", default="", help="the commit the tree was measured at, for the header")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    print("Memory audit (vgpu_memory_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_memory_report_timing out[0]." % args.runs)
    print("Measured at: %s\n" % (args.commit or "(not given)"))
    sections = [section(p, "fib(582)", va.Workload.fib(582), args.runs, True)]
    if not args.small:
        sections.append(section(p, "C2 fib(149794)", va.Workload.fib(149794), args.runs, not args.no_tall_host))
    usage = resource_usage()
    if usage:
        print("== kernels/memory_audit.hip for gfx950 (hipcc -O3, kernel-resource-usage remarks)")
        print("%-18s %6s %6s %16s %16s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "waves per SIMD", "static LDS B"))
        for k in usage:
            print("%-18s %6s %6s %16s %16s %12s" % (re.search(r"k_mm_[a-z_]+", k["name"]).group(0), k.get("vgprs", "?"), k.get("sgprs", "?"), k.get("scratch", "?"),
                                                    k.get("occupancy", "?"), k.get("lds", "?")))
    print("Not measured: the bound of each kernel (no counters were collected), the sort alone against a library sort, a witness with findings at C2's size.")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/memory_audit_profile.py", gpu="MI355X", commit=args.commit, sections=sections, kernels=usage), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
