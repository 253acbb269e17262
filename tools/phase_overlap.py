#!/usr/bin/env python3
"""How the proofs in flight share the GPU, phase by phase, from a rocprofv3 kernel trace of the default bench run:

    rocprofv3 --kernel-trace -d DIR -o run -- python bench.py --full --no-cpu-baseline --no-extra-legs --sustained-seconds 0 --steps 24 --warmup 3
    python tools/phase_overlap.py DIR [--steps 24] [--header "..."]  > profiles/rNN_phase_overlap.txt

(the run tools/profile_round.sh starts as `stats2`; kernel trace only, in a run of its own).  DIR holds the rocpd database (or a
*_kernel_trace.csv).  Over the timed region — the last --steps proofs of the trace, delimited by their k_pow_grind launches — it prints
the share of wall time during which 0, 1, 2, 3 ... launches of a class run at once:

  dense Keccak   thread-per-node tree launches: k_keccak_leaves* / k_keccak_compress* (not the *_pair forms) over more than 32768 nodes
  LDE            the passes of the coset LDE: k_lde_a, k_lde_mid*, k_lde_c

and how the two classes and the other chip-filling kernels (quotient, reduced openings) meet: the share of time with exactly one dense
Keccak launch running beside at least one LDE / quotient / opening launch of another proof.
"""
import argparse
import csv
import glob
import os
import re
import sqlite3
import sys

DENSE_MIN_NODES = 32768
CLASSES = ("dense_keccak", "lde", "quotient_open")


def classify(name, grid):
    m = re.search(r"(k_[a-z0-9_]+)", name)
    k = m.group(1) if m else name
    if (k.startswith("k_keccak_leaves") or k.startswith("k_keccak_compress")) and "_pair" not in k and grid > DENSE_MIN_NODES:
        return "dense_keccak"
    if k == "k_lde_a" or k == "k_lde_c" or k.startswith("k_lde_mid"):
        return "lde"
    if k.startswith("k_quotient") or k.startswith("k_reduce_openings"):
        return "quotient_open"
    if k == "k_pow_grind":
        return "pow"
    if k == "k_ingest":
        return "ingest"
    return None


def load(path):
    """[(name, start_ns, end_ns, grid work-items, queue)] sorted by start, from a rocpd database or a kernel-trace CSV under `path`."""
    dbs = [path] if path.endswith(".db") else sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True))
    if dbs:
        db = sqlite3.connect(dbs[0])
        cols = [r[1] for r in db.execute("pragma table_info(kernels)").fetchall()]
        grid = "grid_x * grid_y * grid_z" if "grid_x" in cols else ("grid_size" if "grid_size" in cols else "0")
        q = "queue_id" if "queue_id" in cols else "0"
        return [(n, s, e, g or 0, qq) for n, s, e, g, qq in db.execute("select name, start, end, %s, %s from kernels order by start" % (grid, q))]
    csvs = [path] if path.endswith(".csv") else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not csvs:
        raise SystemExit("phase_overlap: no rocpd database and no kernel-trace CSV under " + path)
    rows = []
    with open(csvs[0], newline="") as f:
        for r in csv.DictReader(f):
            g = int(r.get("Grid_Size_X", 0) or 0) * max(1, int(r.get("Grid_Size_Y", 1) or 1)) * max(1, int(r.get("Grid_Size_Z", 1) or 1))
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), g, r.get("Queue_Id", "0")))
    rows.sort(key=lambda r: r[1])
    return rows


def timed_region(rows, steps):
    """(t0, t1): from the first proof start behind the (steps+1)-th last k_pow_grind (the fence in front of the timed region lies between
    the two) to the end of the last kernel.  The whole trace when it holds no more than `steps` proofs."""
    pows = [r for r in rows if classify(r[0], r[3]) == "pow"]
    t1 = max(r[2] for r in rows)
    if steps <= 0 or len(pows) <= steps:
        return rows[0][1], t1, len(pows)
    edge = pows[-steps - 1][2]
    later = [r[1] for r in rows if r[1] >= edge and classify(r[0], r[3]) == "ingest"]
    return (later[0] if later else edge), t1, steps


def concurrency(intervals, t0, t1):
    """{n: nanoseconds of [t0, t1) during which exactly n of the intervals run}"""
    ev = []
    for s, e in intervals:
        s, e = max(s, t0), min(e, t1)
        if e > s:
            ev.append((s, 1))
            ev.append((e, -1))
    ev.sort()
    out, live, last = {}, 0, t0
    for t, d in ev:
        if t > last:
            out[live] = out.get(live, 0) + (t - last)
            last = t
        live += d
    if t1 > last:
        out[live] = out.get(live, 0) + (t1 - last)
    return out


def beside(a, b, t0, t1):
    """nanoseconds of [t0, t1) with EXACTLY one interval of `a` and at least one of `b` running"""
    ev = [(max(s, t0), 0, 1) for s, e in a if min(e, t1) > max(s, t0)] + [(min(e, t1), 0, -1) for s, e in a if min(e, t1) > max(s, t0)]
    ev += [(max(s, t0), 1, 1) for s, e in b if min(e, t1) > max(s, t0)] + [(min(e, t1), 1, -1) for s, e in b if min(e, t1) > max(s, t0)]
    ev.sort(key=lambda x: (x[0], x[2]))
    live, last, total = [0, 0], t0, 0
    for t, which, d in ev:
        if t > last:
            if live[0] == 1 and live[1] >= 1:
                total += t - last
            last = t
        live[which] += d
    return total


def report(rows, steps, out):
    t0, t1, proofs = timed_region(rows, steps)
    span = t1 - t0
    by = {c: [] for c in CLASSES}
    for n, s, e, g, _ in rows:
        c = classify(n, g)
        if c in by and e > t0 and s < t1:
            by[c].append((s, e))
    out.write("timed region: %d proofs, %.2f ms wall (%.3f ms per proof), %d launches\n" % (proofs, span / 1e6, span / 1e6 / max(1, proofs), sum(1 for r in rows if t0 <= r[1] < t1)))
    for c, label in (("dense_keccak", "dense Keccak launches (thread per node, > %d nodes)" % DENSE_MIN_NODES), ("lde", "LDE passes (k_lde_a / k_lde_mid* / k_lde_c)"),
                     ("quotient_open", "quotient and reduced-opening launches")):
        conc = concurrency(by[c], t0, t1)
        top = max(conc) if conc else 0
        busy = sum((e - s) for s, e in by[c])
        out.write("%s: %d launches, %.2f ms summed spans\n" % (label, len(by[c]), busy / 1e6))
        out.write("  share of wall time with n running at once: " + "  ".join("%d: %5.1f %%" % (n, 100.0 * conc.get(n, 0) / span) for n in range(0, max(3, top) + 1)) + "\n")
        out.write("  >= 2 at once: %.1f %%\n" % (100.0 * sum(v for n, v in conc.items() if n >= 2) / span))
    others = by["lde"] + by["quotient_open"]
    out.write("exactly one dense Keccak launch beside >= 1 LDE / quotient / opening launch: %.1f %% of wall time\n" % (100.0 * beside(by["dense_keccak"], others, t0, t1) / span))
    out.write("exactly one dense Keccak launch beside >= 1 LDE pass: %.1f %% of wall time\n" % (100.0 * beside(by["dense_keccak"], by["lde"], t0, t1) / span))
    dense2 = 100.0 * sum(v for n, v in concurrency(by["dense_keccak"], t0, t1).items() if n >= 2) / span
    out.write("gate (>= 2 dense Keccak launches overlapping for at least 15 %% of the region): %s (%.1f %%)\n" % ("PASSED" if dense2 >= 15.0 else "NOT passed", dense2))
    return dense2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="rocprofv3 output directory, a rocpd .db or a kernel-trace .csv")
    ap.add_argument("--steps", type=int, default=24, help="proofs of the timed region (the bench run's --steps); 0 = the whole trace")
    ap.add_argument("--header", default=None, help="first line of the record (what was traced, at which commit)")
    a = ap.parse_args()
    rows = load(a.trace)
    if not rows:
        raise SystemExit("phase_overlap: the trace holds no kernel launches")
    if a.header:
        sys.stdout.write("# %s\n" % a.header)
    report(rows, a.steps, sys.stdout)


if __name__ == "__main__":
    main()
