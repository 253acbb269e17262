#!/usr/bin/env python3
"""The program audit's measurements (profiles/program_audit.txt), on GPU 0, one session:

  * fib(582) (cpu 4096 rows), traces generated on the device;
  * one tall trace: the C2 witness (fib(149794), cpu 2^20 rows), traces generated on the device;

each after a warm-up, three runs with the in-library profiler: the device pass split into its kernels, beside the host audit's wall time on the
same inputs (one core, the same words); for k_pg_hist the time to read the pc column once at the measured copy ceiling beside its own time.  At
these sizes the pass is launch-bound: the ratio is for the record, not a target.  The kernels' registers, scratch and occupancy are read from the
compiler's resource-usage remarks when hipcc is on the path.

    python tools/program_audit_profile.py [--runs 3] [--small] [--no-tall-host] [--commit ID] [--json FILE] > profiles/program_audit.txt
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


def resource_usage():
    """[(kernel, vgprs, sgprs, scratch, occupancy, lds)] from hipcc's kernel-resource-usage remarks of kernels/program_audit.hip, or None."""
    src = os.path.join(ROOT, "valida_amd", "csrc", "kernels", "program_audit.hip")
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
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    return [k for k in out if "k_pg_" in k["name"]] or None


def section(p, name, w, runs, host):
    main_t, pre = generate(p, w)
    ms, all_ms, rep, prof = profiled(p, lambda: p.program_audit(main_t, pre, rom_len=w.program_len), runs)
    c = rep.counters
    print("== %s, traces generated on the device: cpu %d rows, table %d rows, ROM %d words; hottest pc %d (%d fetches), %d hard findings, %d wrapped" % (
        name, c["fetches"], c["table_rows"], c["rom_len"], c["hottest_pc"], c["hottest_count"], c["hard"], c["wrapped_operand"]))
    print("device pass %9.3f ms (median of %d profiled runs: %s)" % (ms, runs, " ".join("%.3f" % x for x in all_ms)))
    print("%-16s %10s %10s" % ("kernel", "ms per run", "launches"))
    for k in sorted(prof):
        print("%-16s %10.4f %10.1f" % (k, prof[k][0], prof[k][1]))
    sec = dict(workload=name, device_ms=ms, runs_ms=all_ms, counters=c, kernels={k: dict(ms=v[0], launches=v[1], bytes=v[2]) for k, v in prof.items()})
    if "k_pg_hist" in prof and prof["k_pg_hist"][0] > 0:
        floor_ms = 4.0 * c["fetches"] / COPY_CEILING * 1e3
        print("k_pg_hist: the pc column is %.3f MB; one read of it at the %.1f TB/s copy ceiling takes %.3f us, the kernel %.1f us (%.1f %% of the ceiling)" % (
            4.0 * c["fetches"] / 1e6, COPY_CEILING / 1e12, 1e3 * floor_ms, 1e3 * prof["k_pg_hist"][0], 100 * floor_ms / prof["k_pg_hist"][0]))
        sec.update(hist_floor_ms=floor_ms)
    if host:
        h = va.program_audit_host(p.machine, w.main_traces(), w.preprocessed(), rom_len=w.program_len)
        assert (h.words == rep.words).all()
        print("host audit of the same traces on one core: %.3f ms (the same words)" % h.host_ms)
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
    print("Program audit (vgpu_program_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    print("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_program_report_timing out[0]." % args.runs)
    print("Measured at: %s\n" % (args.commit or "(not given)"))
    sections = [section(p, "fib(582)", va.Workload.fib(582), args.runs, True)]
    if not args.small:
        sections.append(section(p, "C2 fib(149794)", va.Workload.fib(149794), args.runs, not args.no_tall_host))
    usage = resource_usage()
    if usage:
        print("== kernels/program_audit.hip for gfx950 (hipcc -O3, kernel-resource-usage remarks; the LDS is dynamic: at most 132128 bytes for k_pg_hist,")
        print("   2160 + 4 * n_fields * table rows (up to 8192 more) for k_pg_judge, 2192 for k_pg_table)")
        print("%-18s %6s %6s %16s %16s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "waves per SIMD"))
        for k in usage:
            print("%-18s %6s %6s %16s %16s" % (re.search(r"k_pg_[a-z_]+", k["name"]).group(0), k.get("vgprs", "?"), k.get("sgprs", "?"), k.get("scratch", "?"), k.get("occupancy", "?")))
    print("Not measured: LDS atomics under same-address contention against a wave-level pre-aggregation (no variant was built), a table taller than")
    print("one slice at C2's height, a witness with findings at C2's size, the bound of each kernel (no counters were collected).")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/program_audit_profile.py", gpu="MI355X", commit=args.commit, sections=sections, kernels=usage), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
