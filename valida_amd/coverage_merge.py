"""Merge the coverage audits of several witnesses into one corpus-level report.

    python -m valida_amd.coverage_merge OUT.json IN.json [IN.json ..]

Every IN.json is a report written by `python -m valida_amd.cli check .. --coverage`; their "coverage" keys (one machine, one delta set) are
added cell-wise by CoverageReport.merge — kills, sole, detected, free and heights add, the classes are recomputed, the row minima are dropped —
and written to OUT.json under the key "coverage".  Stdout gets `check --coverage`'s per-chip lines for the corpus: a constraint that is dead here
is reached by none of the programs.  Needs no device.  Exit status 0 unless a file cannot be read or the reports do not belong together."""
import json
import sys


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) < 2 or argv[0].startswith("-"):
        print(__doc__, file=sys.stderr)
        return 2
    import valida_amd as va
    from valida_amd import cli

    try:
        reports = []
        for path in argv[1:]:
            with open(path) as f:
                j = json.load(f)
            if "coverage" not in j:
                raise ValueError("%s has no \"coverage\" key (written without --coverage?)" % path)
            reports.append(va.CoverageReport.from_dict(j["coverage"]))
        merged = va.CoverageReport.merge(reports)
        with open(argv[0], "w") as f:
            f.write(json.dumps(dict(coverage=merged.to_dict(), merged=len(reports))) + "\n")
    except (OSError, ValueError, KeyError) as e:
        print("coverage_merge: %s" % e, file=sys.stderr)
        return 1
    for line in cli.coverage_lines(merged):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
