#!/usr/bin/env python3
"""The arithmetic audit's measurements (profiles/arithmetic_audit.txt), on GPU 0, one session:

  * fib(582) (add 4096 rows), traces generated on the device;
  * alu(116507), the size of tests/golden/full_c4_alu116507.json (cpu 2^20 rows), traces generated on the device;

each with the receives and with both sides, after a warm-up, `--runs` runs with the in-library profiler: the device pass (median, and every run)
split into its kernels, beside the host twin's wall time on the same inputs (one core, the same words).  No threshold is set: the file records
what the pass takes.  The GPU's clocks as rocm-smi shows them at the start are noted; the kernels' registers, scratch and occupancy are read from
the compiler's resource-usage remarks when hipcc is on the path.

    python tools/arithmetic_audit_profile.py [--runs 5] [--small] [--commit ID] [--out profiles/arithmetic_audit.txt] [--json FILE]
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


def clocks():
    """What rocm-smi shows for GPU 0's clocks (read only), or the reason there is nothing."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=60)
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["not read (%s)" % type(e).__name__]
    lines = [re.sub(r"\s+", " ", x).strip() for x in r.stdout.split("\n") if "clk" in x.lower()]
    return lines or ["not read (rocm-smi printed no clock line)"]


def resource_usage():
    """[dict(name, vgprs, sgprs, scratch, occupancy)] from hipcc's kernel-resource-usage remarks of kernels/arithmetic_audit.hip, or None."""
    src = os.path.join(ROOT, "valida_amd", "csrc", "kernels", "arithmetic_audit.hip")
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
    return [k for k in out if "k_ar_" in k["name"]] or None


def section(p, say, name, w, runs):
    main_t, pre = generate(p, w)
    mt, prep = w.main_traces(), w.preprocessed()
    out = []
    for sides in ("receives", "both"):
        ms, all_ms, rep, prof = profiled(p, lambda: p.arithmetic_audit(main_t, pre, sides=sides), runs)
        c = rep.counters
        say("== %s, traces generated on the device, sides = %s: %d entries, %d slots, %d live records, %d hard, %d soft, %d MULHS records where the sign matters" % (
            name, sides, len(rep.entries), c["slots"], c["live"], c["hard"], c["soft"], c["mulhs_sign_matters"]))
        say("device pass %9.3f ms (median of %d profiled runs after a warm-up: %s)" % (ms, runs, " ".join("%.3f" % x for x in all_ms)))
        say("%-16s %10s %10s" % ("kernel", "ms per run", "launches"))
        for k in sorted(prof):
            say("%-16s %10.4f %10.1f" % (k, prof[k][0], prof[k][1]))
        hosts = [va.arithmetic_audit_host(p.machine, mt, prep, sides=sides) for _ in range(3)]
        assert all((h.words == rep.words).all() for h in hosts)
        host_ms = statistics.median(h.host_ms for h in hosts)
        say("host twin on the same traces, one core: %.3f ms (median of 3; the same words)\n" % host_ms)
        out.append(dict(workload=name, sides=sides, device_ms=ms, runs_ms=all_ms, host_twin_ms=host_ms, counters=c, kernels={k: dict(ms=v[0], launches=v[1]) for k, v in prof.items()}))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="skip the tall trace")
    ap.add_argument("--commit", default="", help="the commit the tree was measured at, for the header")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arithmetic_audit.txt"))
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    lines = []

    def say(text=""):
        lines.append(text)
        print(text)

    p = va.Prover(va.Machine.basic(), va.poseidon_round_constants(), device=0)
    say("Arithmetic audit (vgpu_arithmetic_audit) - measurements on one MI355X; kernel times from the in-library profiler (HIP events around each")
    say("launch), summed over the launches of a run, mean over %d profiled runs after a warm-up; device pass = vgpu_arithmetic_report_timing out[0]," % args.runs)
    say("HIP events around the whole pass, the two downloads of totals and records included.  No threshold is set on any of these figures.")
    say("Measured at: %s" % (args.commit or "(not given)"))
    say("GPU 0 clocks at the start (rocm-smi --showclocks): " + "; ".join(clocks()) + "\n")
    sections = section(p, say, "fib(582)", va.Workload.fib(582), args.runs)
    if not args.small:
        sections += section(p, say, "alu(116507)", va.Workload.alu(116507), args.runs)
    usage = resource_usage()
    if usage:
        say("== kernels/arithmetic_audit.hip for gfx950 (hipcc -O3, kernel-resource-usage remarks)")
        say("%-18s %6s %6s %16s %16s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "waves per SIMD"))
        for k in usage:
            say("%-18s %6s %6s %16s %16s" % (re.search(r"k_ar_[a-z_]+", k["name"]).group(0), k.get("vgprs", "?"), k.get("sgprs", "?"), k.get("scratch", "?"), k.get("occupancy", "?")))
    say("Not measured: a witness with findings at the tall size (the listing pass runs only for entries with a finding), the bound of each kernel")
    say("(no counters were collected), one fused launch over all entries against the launch per entry.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/arithmetic_audit_profile.py", gpu="MI355X", commit=args.commit, sections=sections, kernels=usage), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
