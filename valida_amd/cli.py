"""`valida run|prove|verify` (and `check`) for Valida executables (the reference's CLI: basic/src/bin/valida.rs:40-56, 330-449), on this backend.

    python -m valida_amd.cli run    PROGRAM OUTPUT_FILE [ADVICE] [--stack-height N] [--max-cycles N]
    python -m valida_amd.cli prove  PROGRAM PROOF_FILE  [ADVICE] [--stack-height N] [--max-cycles N] [--device D] [config flags]
    python -m valida_amd.cli verify PROGRAM PROOF_FILE  [ADVICE] [--device D] [config flags]
    python -m valida_amd.cli check  PROGRAM REPORT_FILE [ADVICE] [--stack-height N] [--max-cycles N] [--device D | --host] [--max-tuples N] [--max-records N]
                                                                [--constraints] [--max-constraints N] [--mutations] [--coverage] [--pairs] [--rank] [--fields] [--links] [--steps] [--step-sizes T[,T..]] [--invariants] [--transitions] [--min-gate-windows N] [--max-gates N] [--products] [--domains] [--max-bits N] [--lookup-buses B[,B..]] [--memory] [--program] [--arithmetic] [--sides receives|sends|both] [--max-findings N] [--chips C[,C..]] [--deltas D[,D..]]
    python -m valida_amd.coverage_merge OUT.json IN.json [IN.json ..]

PROGRAM: raw machine code (24-byte little-endian records) or a little-endian ELF, read as load_executable_file reads it (elf/src/lib.rs:19-120).
ADVICE: a file whose bytes are the advice tape (FixedAdviceProvider); without it the tape is empty (the reference reads stdin instead).
--stack-height: the initial frame pointer (default 16777216, as the reference's).  --max-cycles: a run that has not stopped after that many
cycles is refused (default 2^22, the largest cpu height this repository proves).

run     Machine::run on the host, then writes OutputChip::bytes to OUTPUT_FILE.
prove   the device path end to end: the VM on the host, its operation logs uploaded (vgpu_oplog_upload), all fourteen main traces generated
        on GPU D (vgpu_generate_trace), the preprocessed traces uploaded, Machine::prove, the proof written as CBOR.  One JSON line of
        phase times (milliseconds) goes to stderr.
verify  loads PROGRAM without running it (the preprocessed commitment depends on the ROM alone) and runs valida_amd.verify_cli on PROOF_FILE.

check   the bus audit of the program's witness (vgpu_bus_audit: which LogUp tuples are unbalanced, sent by which chip on which row, received by
        nobody — what a proof every verifier rejects for its cumulative sums cannot say): the VM on the host, then either the device path of
        `prove` up to the traces (operation logs uploaded, fourteen traces generated on GPU D, default 0) and the audit on the device, or, with
        --host, host traces and the host audit.  Writes the JSON report to REPORT_FILE, prints one line per reported tuple (bus, fields, net, the
        listed records; for a memory-bus tuple also pc and opcode of its cycle: cpu rows are indexed by clk) and a summary line.
        --constraints adds the constraint audit of the same witness (vgpu_constraint_audit: which AIR constraints fail, on which rows, with
        which value — what check_constraints and the debug path of `prove` report one chip and one row at a time), on the same path as the bus
        audit (device or --host).  The JSON report gets one more key, "constraints" (ConstraintReport.to_json's object); after the bus lines
        stdout gets one line per listed constraint, `<chip> constraint <k> fails on <count> rows: row r = value, ..` (for a cpu row also pc and
        opcode), and a summary line `satisfied: ..` or `violated: N constraints of M chips ..`; --max-constraints N cuts the list (default 64).
        Without the flag `check` does what it did before the flag existed, byte for byte.
        --mutations adds the mutation audit of the same witness (vgpu_mutation_audit: which trace cells could be changed by a delta without any
        AIR constraint or bus noticing — mutation testing of the AIRs), on the same path (device or --host); --deltas 1,-1,2 names 1 to 4 distinct
        deltas (integers mod p; default 1,-1).  The JSON report gets one more key, "mutations" (MutationReport.to_json's object); after the other
        lines stdout gets one line per chip that has a free cell, `<chip>: unbound columns 14, 15, 17; free cells 3131 (+1), 3047 (-1) of 13056`.
        An unbound column is slack of the AIR, not a fault of the witness: the exit status does not depend on this flag.
        --coverage adds the coverage audit of the same witness (vgpu_coverage_audit: per constraint and per bus interaction of every chip, which
        of the mutation audit's mutations it detects and of which it is the ONLY detector), on the same path (device or --host) and with the same
        --deltas.  The JSON report gets one more key, "coverage" (CoverageReport.to_json's object); after the other lines stdout gets one line per
        chip that has a dead or shadowed detector, `lt: dead constraints 21, 29-30, 32, 34; never the only detector: constraints 0-1, 6-17; 1
        interaction essential`.  "Dead" says what THIS program reaches with single-cell changes by these deltas — not a fault of the witness or of
        the AIR; "never the only detector" does not mean removable (it may be the only guard against a two-cell change).  The exit status does not
        depend on this flag.  coverage_merge adds the "coverage" keys of several reports of one machine and one delta set into a corpus report.
        --pairs adds the pair audit of the same witness (vgpu_pair_audit: which two cells of one row could be changed together without any AIR
        constraint or bus noticing although one of the changes alone is noticed), on the same path (device or --host) and with the same --deltas;
        --chips=cpu,3 restricts it to those chips (names or indices).  The JSON report gets one more key, "pairs" (PairReport.to_json's object);
        after the other lines stdout gets one line per chip that has a slack pair, `add: 6 slack pairs of 136 coupled: (0,4) (0,8) ..`.  Same-row
        pairs on THIS witness only, not a soundness proof: the exit status does not depend on this flag.
        --rank adds the rank audit of the same witness (vgpu_rank_audit: per trace row the null space of the Jacobian of every constraint and bus
        record that reads the row — every first-order degree of freedom, of any arity and with any coefficients), on the same path (device or
        --host), restricted by the same --chips.  The JSON report gets one more key, "rank" (RankReport.to_json's object); stdout gets one line
        per chip that has a coupled column (bound alone, slack together), `add: 12 coupled columns: 0 1 2 ..; max nullity 8; 23 coupled rows`.
        First order, one row, THIS witness, not a soundness proof: the exit status does not depend on this flag.
        --fields adds the field audit of the same witness (vgpu_field_audit: per trace row and live bus record, which of the record's fields the
        chip's constraints, the counts and the record's other fields leave undetermined to first order — the rank audit's Jacobian asked per
        record FIELD instead of per cell: a chip that receives (opcode, a, b, c) and never ties c to a and b), on the same path (device or --host),
        restricted by the same --chips.  The JSON report gets one more key, "fields" (FieldReport.to_json's object); stdout gets one line per
        (chip, interaction) with a floating field, `div: interaction 0 (receives on the general bus): fields 0-12 float on 2 of 2 live rows`
        (the largest row count of a floating field).  First order, on THIS witness, the other rows' cells held fixed: b (b - 1) = 0 pins b, x^2 = 0
        at x = 0 makes x look free, a field determined only for y != 0 floats on the rows where y = 0.  A floating field on a SEND usually means
        that the chip delegates (cpu's read values, shift's output): the finding is a field that also floats on the receiving chip; inputs are
        not functions of outputs, so lt's operands are expected to float.  The exit status does not depend on this flag.
        --links adds the link audit of the same witness (vgpu_link_audit: the field audit's float mask of every live record ANDed over the
        records of each bus tuple, sends and receives alike — a position that floats at EVERY record of a tuple is open: no chip on the bus pins
        it; a field that floats at a record whose tuple has it pinned elsewhere is answered), on the same path (device or --host), always over all
        chips; --max-tuples and --max-records cut the listed open tuples.  The JSON report gets one more key, "links" (LinkReport.to_json's
        object); stdout gets one line per bus with an open tuple, `memory bus: 349 of 349 tuples open; open positions 2, 4-7`, and one line per
        (chip, interaction) whose floating fields are not all answered, `mem: interaction 0 (receives on the memory bus): fields 2, 4-7 open on
        401 of 401 floating rows` (per field the largest counts).  First order, on THIS witness; each record is judged alone (sister records of
        the same row are not held fixed), so "open" means that no single record's own chip pins the position — a joint move may still be blocked
        by a sister record; "anchored" is per tuple as it stands: a lookup bus whose receiver can move multiplicities between tuples is not
        modelled.  The exit status does not depend on this flag.
        --steps adds the step audit of the same witness (vgpu_step_audit: the rank audit's canonical null vector of every (row, loose column),
        moved by finite steps and judged by the mutation audit's rule — which first-order freedoms are real trades every check accepts, and
        which are artefacts of a quadratic constraint at a degenerate point), on the same path (device or --host), restricted by the same
        --chips; --step-sizes=1,-1,2 names 1 to 4 distinct step sizes (integers mod p; default 1,-1,2).  The JSON report gets one more key,
        "steps" (StepReport.to_json's object); stdout gets one line per chip that has a confirmed or refuted column, `add: confirmed columns
        0-7, 11-14 on 23 rows (whole lines: degree 3 <= 3 steps); refuted columns 5-8 on 72 rows` (a half with nothing to say is omitted; the
        parenthesis only when the steps are enough for the chip's constraint degree).  One row, THIS witness, the canonical vectors only: the
        exit status does not depend on this flag.
        --invariants adds the invariant audit of the same witness (vgpu_invariant_audit: per chip every affine-linear relation among the main
        columns that holds on every row of the witness — one per non-pivot column of the reduced row echelon form of the rows (1, M[r]) — and
        per relation the rows on which the chip's own constraints and bus records enforce it to first order, judged against the rank audit's
        Jacobian), on the same path (device or --host), restricted by the same --chips.  The JSON report gets one more key, "invariants"
        (InvariantReport.to_json's object); stdout gets one line per chip that has an invariant, `add: 7 invariants (4 constant columns);
        enforced on every row: columns 12-14` (the parts name the RELATIONS by verdict — every row, `enforced on some rows`, `never enforced` —
        and appear only when present; constant columns are counted, with `, N never enforced` when some are).  Never enforced is a candidate
        missing constraint or a column this program never exercises.  Affine-linear relations only (b (b - 1) = 0 is not found), within one row
        (none between a row and its successor), on THIS witness (a short program has accidental relations), per basis vector (a sum of two
        free invariants can be enforced), first order with the rank audit's caveats: the exit status does not depend on this flag.
        --transitions adds the transition audit of the same witness (vgpu_transition_audit: the invariant audit over the two-row windows
        (1, M[r], M[r + 1]), r = 0 .. n - 2, on every window and on the windows where a boolean window column holds one value — the gates — and
        per listed relation the windows at which the rank audit's Jacobian of one of the two rows lets it break), on the same path (device or
        --host), restricted by the same --chips; --min-gate-windows N (default 64) is the fewest windows of an audited gate, --max-gates N
        (default 256) the gates listed per chip.  The JSON report gets one more key, "transitions" (TransitionReport.to_json's object); stdout
        gets one line per chip that has an entry, `mem: 1 transition relation (0 held on every window); 21 gated relations under 8 of 11
        audited gates (13 gates in all), 5 never held`.  Never held is a candidate missing transition constraint.  Affine-linear, single gates
        (no conjunction of two), THIS witness, per basis vector, first order and one row at a time (held is exact only for chips whose
        constraints do not read the next row): the exit status does not depend on this flag.
        --products adds the product audit of the same witness (vgpu_product_audit: per chip every product of two independent columns — the
        pivot main columns of the invariant audit's reduced row echelon form — that is an affine function of the row on every row of the
        witness, and per relation the rows on which the chip's own constraints and bus records enforce it to first order, judged against the
        rank audit's Jacobian), on the same path (device or --host), restricted by the same --chips.  The JSON report gets one more key,
        "products" (ProductReport.to_json's object); stdout gets one line per chip that has a relation, `add: 29 product relations of 45
        pairs (5 boolean, 7 zero, 9 select, 8 other); enforced on every row 17, on some rows 12, never 0`.  Never enforced is a candidate
        missing constraint (a forgotten b^2 = b, s t = 0, s x = y) or a column this program never exercises.  Single products only (s a - s b
        = 0 is found only when s a and s b are each affine), within one row, on THIS witness (a short program has accidental relations), first
        order with the rank audit's caveats: the exit status does not depend on this flag.
        --domains adds the domain audit of the same witness (vgpu_domain_audit: per chip and main column the set of values the witness puts
        there — min, max, the exact number of distinct values below 2^16, a class from constant to wide — and the rows on which a narrow
        column, byte or half-word valued below 2^N for --max-bits N (default 16), is not a bare field of a live send to a lookup table), on
        the same path (device or --host), restricted by the same --chips.  A lookup table is a bus all of whose receivers are chips without
        constraints and sends (on the BasicMachine the memory and the range bus); --lookup-buses=3 or =g3,l0 names them instead (g: global,
        l: local).  The JSON report gets one more key, "domains" (DomainReport.to_json's object); stdout gets one line per chip that has an
        entry, `add: 4 narrow columns unguarded (columns 2-3,6-7: byte-valued on up to 103 rows, on no lookup send)`.  A candidate missing
        range check, on THIS witness (a short program leaves columns accidentally narrow) and for bare fields only (a send of 256 a + b guards
        neither column): never changes the exit status.
        --memory adds the memory audit of the same witness (vgpu_memory_audit: the receives of the memory bus replayed as a memory — the live
        records ordered by (addr, clk, static first, trace order), per address the last write — and the records that break it: a malformed
        record, a duplicate static record, a read that does not return the last write to its address, a read of a non-zero value from an address
        nobody wrote), on the same path (device or --host); --max-findings N lists the first N (default 64).  The JSON report gets one more
        key, "memory" (MemoryReport.to_dict's object); stdout gets one line per finding kind present, `mem: 1 stale read (row 812, addr 4076,
        clk 55: read 5, last write 3 at row 811)`, and one summary line with the counters: live records, addresses, same-cycle pairs (verdicts
        that rest on the trace's own order), the largest clk gap, the dummy reads the reference's unfinished memory argument would need, and
        whether the trace as laid out is sorted.  It judges the table's receives (whether the senders agree is the bus audit's question).
        Findings are definite faults: with --memory, check exits 1 when there is one.
        --program adds the program audit of the same witness (vgpu_program_audit: every cpu row's (pc, opcode, a..e) held against the program
        chip's preprocessed ROM row, and the ROM's multiplicity column against the fetch counts: the reference's commented-out program bus
        replayed), on the same path (device or --host), with the ROM's real length so that the table's padding rows are not fetchable;
        --max-findings N lists the first N (default 64).  The JSON report gets one more key, "program" (ProgramReport.to_dict's object); stdout
        gets one line per hard kind present, `cpu: 1 wrong instruction (row 100, pc 12: operand a 7, ROM 0)`, one line for wrapped operands,
        `cpu: 8 fetches differ from the ROM only by 2^32 in an immediate (first row 5, pc 5, fields c)` (the reference writes the u32 value of a
        negative immediate mod p into the cpu row where the ROM holds p - |x|: counted apart, never a fault), and one summary line with the
        counters and the first ranges of words that never ran.  It judges the fetches against the table of THIS witness, not what the step did.
        Hard findings are definite faults: with --program, check exits 1 when there is one; wrapped operands never change the status.
        --arithmetic adds the arithmetic audit of the same witness (vgpu_arithmetic_audit: every live record (opcode, x, y, z) of the general
        bus recomputed in 32-bit integer arithmetic), on the same path (device or --host); --sides receives|sends|both selects the ALU chips'
        receives (the default), the senders' records (the cpu's, and shift's delegations to mul and div), or both; --max-findings N lists the
        first N of each list (default 64).  The JSON report gets one more key, "arithmetic" (ArithmeticReport.to_dict's object); stdout gets
        one line per hard kind present, `div: 1 wrong result (row 2, DIV32: 100 / 7 = 15, expected 14)`, one line per soft kind (an SDIV
        record by 2^k that holds the arithmetic shift: shift's delegation of SRA to div; an SHR record that holds the arithmetic shift: the
        reference logs SRA rows as Shr32; counted apart, never a fault) and one summary line with the counters.  It judges each record alone
        (whether senders and receivers agree is the bus audit's question).  Hard findings are definite faults: with --arithmetic, check exits
        1 when there is one; soft findings never change the status.

Config flags (--log-blowup, --queries, --pow-bits, --poseidon-mmcs, --constants) are verify_cli's and must match between prove and verify.
Exit status: 0 on success (run / prove done, proof accepted, witness balanced, with --constraints every constraint satisfied, with --memory no memory finding, with --program no hard program finding and with --arithmetic no hard arithmetic finding), 1 otherwise (the reference always exits 0)."""
import argparse
import json
import sys
import time


def _config_flags(ap):
    ap.add_argument("--log-blowup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=40)
    ap.add_argument("--pow-bits", type=int, default=8)
    ap.add_argument("--poseidon-mmcs", action="store_true", help="commit with the Poseidon-16 MMCS (hash_kind 1) instead of Keccak-256")
    ap.add_argument("--constants", choices=["splitmix", "cli"], default="splitmix")


def prove_on_device(w, prover):
    """Steps 2-4 of `prove` on an executed workload: (proof, device main traces, phase times in ms)."""
    import valida_amd as va

    times = {}
    t = time.perf_counter()
    log = prover.upload_oplog(w.oplog())
    times["upload_oplog_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    main = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
    times["generate_trace_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    prep = [(chip, prover.upload(m)) for chip, m in w.preprocessed()]
    times["upload_preprocessed_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    proof = prover.prove(main, prep)
    times["prove_ms"] = (time.perf_counter() - t) * 1e3
    return proof, main, times


OPCODE_NAMES = {1: "LOAD32", 2: "STORE32", 3: "JAL", 4: "JALV", 5: "BEQ", 6: "BNE", 7: "IMM32", 8: "STOP", 9: "READ_ADVICE", 10: "LOADFP", 11: "LOADU8", 12: "LOADS8",
                13: "STOREU8", 100: "ADD32", 101: "SUB32", 102: "MUL32", 103: "DIV32", 104: "LT32", 105: "SHL32", 106: "SHR32", 107: "AND32", 108: "OR32",
                109: "XOR32", 110: "SDIV32", 111: "NE32", 112: "MULHU32", 113: "SRA32", 114: "MULHS32", 115: "LTE32", 116: "EQ32", 117: "SLT32", 118: "SLE32",
                300: "WRITE"}  # opcodes/src/lib.rs:7-45
CPU_PC, CPU_OPCODE = 1, 3  # cpu/src/columns.rs


def report_lines(report, cpu_trace):
    """One line per reported tuple of a BasicMachine bus report, and the summary line."""
    import valida_amd as va

    lines = []
    for t in report.tuples:
        bus = "%s bus" % va.BUS_NAMES[t["bus"]] if t["bus"] in va.BUS_NAMES else "bus (%s, %d)" % ("global" if t["bus"][0] else "local", t["bus"][1])
        recs = ", ".join("%s row %d interaction %d %s %d" % (va.CHIP_NAMES[c] if c < len(va.CHIP_NAMES) else "chip %d" % c, row, m, "sends" if snd else "receives", cnt)
                         for c, row, m, snd, cnt in t["records"])
        more = t["n_send"] + t["n_recv"] - len(t["records"])
        line = "%s %s net %+d (%d sent in %d records, %d received in %d): %s%s" % (
            bus, t["fields"], t["net_signed"], t["send_sum"], t["n_send"], t["recv_sum"], t["n_recv"], recs, " and %d more" % more if more else "")
        if t["bus"] == (1, 2) and len(t["fields"]) > 1 and t["fields"][1] < cpu_trace.shape[0]:  # memory bus: [is_read, clk, addr, value..]
            clk = t["fields"][1]
            op = int(cpu_trace[clk, CPU_OPCODE])
            line += "; cycle %d: pc %d %s" % (clk, int(cpu_trace[clk, CPU_PC]), OPCODE_NAMES.get(op, "opcode %d" % op))
        lines.append(line)
    live = sum(b["live"] for b in report.buses)
    if report.balanced:
        lines.append("balanced: %d live bus records, no unbalanced tuple" % live)
    else:
        lines.append("unbalanced: %d tuples of %d live bus records do not cancel%s" % (
            report.total_unbalanced, live, " (the first %d are listed)" % report.reported if report.truncated else ""))
    return lines


def constraint_lines(report, cpu_trace):
    """One line per listed constraint of a constraint report, and the summary line."""
    import valida_amd as va

    lines = []
    for e in report.constraints:
        name = va.CHIP_NAMES[e["chip"]] if e["chip"] < len(va.CHIP_NAMES) else "chip %d" % e["chip"]
        rows = []
        for row, value in e["rows"]:
            text = "row %d = %d" % (row, value)
            if e["chip"] == 0 and row < cpu_trace.shape[0]:
                op = int(cpu_trace[row, CPU_OPCODE])
                text += " (pc %d %s)" % (int(cpu_trace[row, CPU_PC]), OPCODE_NAMES.get(op, "opcode %d" % op))
            rows.append(text)
        more = e["failing_rows"] - len(e["rows"])
        lines.append("%s constraint %d fails on %d rows: %s%s" % (name, e["constraint"], e["failing_rows"], ", ".join(rows), " and %d more" % more if more else ""))
    n_constraints = sum(c["constraints"] for c in report.chips)
    if report.satisfied:
        lines.append("satisfied: all %d constraints of %d chips hold on every row" % (n_constraints, len(report.chips)))
    else:
        lines.append("violated: %d constraints of %d chips fail, on %d rows%s" % (
            report.total_failing, sum(1 for c in report.chips if c["failing_constraints"]), sum(c["failing_rows"] for c in report.chips),
            " (the first %d are listed)" % report.reported if report.truncated else ""))
    return lines


def parse_deltas(text):
    """--deltas: comma-separated integers, taken mod p."""
    import valida_amd as va

    return [int(x) % va.P for x in text.split(",") if x.strip()]


def index_ranges(cols):
    """Ascending indices in range notation: 21, 29-30, 32."""
    out = []
    for c in cols:
        if out and out[-1][1] == c - 1:
            out[-1][1] = c
        else:
            out.append([c, c])
    return ", ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)


def mutation_lines(report):
    """One line per chip of a mutation report that has a free cell: its unbound columns by index and its free cells per delta."""
    import valida_amd as va

    def signed(d):
        return "%+d" % (d if d <= va.P // 2 else d - va.P)

    ranges = index_ranges

    lines = []
    for c in report.chips:
        if not any(c["free"]):
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        cols = report.unbound_columns(c["chip"])
        lines.append("%s: %s; free cells %s of %d" % (name, "unbound columns " + ranges(cols) if cols else "no unbound column",
                                                     ", ".join("%d (%s)" % (f, signed(d)) for f, d in zip(c["free"], report.deltas)), c["height"] * c["width"]))
    return lines


def parse_chips(text):
    """--chips: comma-separated chip names or indices; None (all chips) when empty."""
    import valida_amd as va

    out = []
    for x in (text or "").split(","):
        x = x.strip()
        if not x:
            continue
        if x in va.CHIP_NAMES:
            out.append(list(va.CHIP_NAMES).index(x))
        elif x.isdigit() and int(x) < va.NUM_CHIPS:
            out.append(int(x))
        else:
            raise va.VgpuError(-1, "check --chips: %r is neither a chip name (%s) nor an index below %d" % (x, ", ".join(va.CHIP_NAMES), va.NUM_CHIPS))
    return out or None


def pair_lines(report, limit=12):
    """One line per chip of a pair report that has a slack pair: how many of its coupled pairs, and the first of them as (c1,c2)."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        if not c["slack"]:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        pairs = report.slack_pairs(c["chip"])
        shown = " ".join("(%d,%d)" % p for p in pairs[:limit]) + (" .." if c["slack"] > min(limit, len(pairs)) else "")
        lines.append("%s: %d slack pair%s of %d coupled: %s" % (name, c["slack"], "" if c["slack"] == 1 else "s", c["coupled"], shown))
    return lines


def rank_lines(report, limit=16):
    """One line per chip of a rank report that has a coupled column: the columns, the largest nullity of a row, the coupled rows."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        cols = report.coupled_columns(c["chip"])
        if not cols:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        shown = " ".join(str(k) for k in cols[:limit]) + (" .." if len(cols) > limit else "")
        lines.append("%s: %d coupled column%s: %s; max nullity %d; %d coupled row%s" % (name, len(cols), "" if len(cols) == 1 else "s", shown, c["max_nullity"], c["coupled_rows"],
                                                                                  "" if c["coupled_rows"] == 1 else "s"))
    return lines


def step_lines(report):
    """One line per chip of a step report that has a confirmed (coupled and exact) or a refuted (curved) column."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        conf, ref = report.confirmed_columns(c["chip"]), report.refuted_columns(c["chip"])
        if not conf and not ref:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        parts = []
        if conf:
            whole = " (whole lines: degree %d <= %d steps)" % (c["max_degree"], len(report.steps)) if c["line_exact"] else ""
            parts.append("confirmed columns %s on %d rows%s" % (index_ranges(conf), c["confirmed_rows"], whole))
        if ref:
            parts.append("refuted columns %s on %d rows" % (index_ranges(ref), c["refuted_rows"]))
        lines.append("%s: %s" % (name, "; ".join(parts)))
    return lines


def transition_lines(report):
    """One line per chip of a transition report that has an entry: the ungated transition relations, the gated ones and their gates."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        if not c["transitions"] and not c["gated"]:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        mine = [e for e in report.entries if e["chip"] == c["chip"]]
        ungated = [e for e in mine if e["gate"] is None]
        gated = [e for e in mine if e["gate"] is not None]
        parts = []
        if c["transitions"]:
            parts.append("%d transition relation%s (%d held on every window)" % (c["transitions"], "" if c["transitions"] == 1 else "s", len([e for e in ungated if not e["free_windows"]])))
        if c["gated"]:
            under = len(set(e["gate"] for e in gated))
            cut = "" if len(gated) == c["gated"] else ", %d listed" % len(gated)
            parts.append("%d gated relation%s%s under %d of %d audited gates (%d gates in all), %d never held" % (
                c["gated"], "" if c["gated"] == 1 else "s", cut, under, c["gates_audited"], c["n_gates"], len([e for e in gated if not e["held_windows"]])))
        lines.append("%s: %s" % (name, "; ".join(parts)))
    return lines


def invariant_lines(report):
    """One line per chip of an invariant report that has an invariant: how many, the constant columns among them, the relations by verdict."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        if not c["invariants"]:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        mine = [e for e in report.entries if e["chip"] == c["chip"]]
        consts = [e for e in mine if e["kind"] == "constant"]
        rel = [e for e in mine if e["kind"] == "relation"]
        head = "%d invariant%s" % (c["invariants"], "" if c["invariants"] == 1 else "s")
        if c["constant_columns"]:
            loose = len([e for e in consts if e["enforced_rows"] == 0])
            head += " (%d constant column%s%s)" % (c["constant_columns"], "" if c["constant_columns"] == 1 else "s", ", %d never enforced" % loose if loose else "")
        parts = [head]
        for label, keep in (("enforced on every row", lambda e: e["free_rows"] == 0), ("enforced on some rows", lambda e: e["free_rows"] and e["enforced_rows"]),
                            ("never enforced", lambda e: e["enforced_rows"] == 0)):
            cols = [e["column"] for e in rel if keep(e)]
            if cols:
                parts.append("%s: columns %s" % (label, index_ranges(cols)))
        lines.append("%s: %s" % (name, "; ".join(parts)))
    return lines


def product_lines(report):
    """One line per chip of a product report that has a relation: how many of how many pairs, by kind and by verdict."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        if not c["relations"]:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        lines.append("%s: %d product relation%s of %d pair%s (%d boolean, %d zero, %d select, %d other); enforced on every row %d, on some rows %d, never %d" % (
            name, c["relations"], "" if c["relations"] == 1 else "s", c["pairs"], "" if c["pairs"] == 1 else "s", c["boolean"], c["zero"], c["select"], c["other"],
            c["every"], c["some"], c["never"]))
    return lines


def _column_ranges(cols):
    """[2, 3, 6, 7] as "2-3,6-7"."""
    out, k = [], 0
    while k < len(cols):
        j = k
        while j + 1 < len(cols) and cols[j + 1] == cols[j] + 1:
            j += 1
        out.append("%d" % cols[k] if j == k else "%d-%d" % (cols[k], cols[j]))
        k = j + 1
    return ",".join(out)


def domain_lines(report):
    """One line per chip of a domain report that has an entry: its narrow columns with a non-zero cell on a row that no lookup send guards."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        mine = [e for e in report.entries if e["chip"] == c["chip"]]
        if not mine:
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        cols = report.columns(c["chip"])
        never = all(cols[e["column"]]["guarded_rows"] == 0 for e in mine)
        lines.append("%s: %d narrow column%s unguarded (column%s %s: %s-valued on up to %d rows, %s)" % (
            name, c["entries"], "" if c["entries"] == 1 else "s", "" if c["entries"] == 1 else "s", _column_ranges([e["column"] for e in mine]) + (",.." if len(mine) < c["entries"] else ""),
            "half" if any(e["cls"] == "half" for e in mine) else "byte", max(e["unguarded_nonzero_rows"] for e in mine),
            "on no lookup send" if never else "lookup sends miss these rows"))
    return lines


def parse_lookup_buses(text):
    """--lookup-buses: None (the structural rule) or [(is_global, bus_index)] from 3 / g3 / l0, comma-separated."""
    if not text:
        return None
    out = []
    for t in text.split(","):
        t = t.strip()
        is_global = not t.startswith("l")
        out.append((is_global, int(t.lstrip("gl"))))
    return out


def memory_value(v):
    """The four value fields of a memory record as the number they spell when they are bytes (big-endian, as the VM's Word), else their list."""
    return (v[0] << 24) | (v[1] << 16) | (v[2] << 8) | v[3] if all(x < 256 for x in v) else list(v)


MEMORY_KIND_TEXT = {"malformed": "malformed record", "duplicate_static": "duplicate static record", "stale_read": "stale read", "uninit_read": "uninitialised read"}
MEMORY_REASONS = ("count is not 1", "is_read is not 0 or 1", "is_static is not 0 or 1", "static with is_read or clk", "a value field is no byte")


def memory_lines(report):
    """One line per finding kind of a memory report (the count and the first listed record of the kind), then one summary line with the counters."""
    import valida_amd as va

    c, lines = report.counters, []
    name = va.CHIP_NAMES[2] if report.receives == [(2, 0)] else "memory"  # the BasicMachine's table is its mem chip
    for kind in va.MEMORY_KINDS:
        if not c[kind]:
            continue
        head = "%s: %d %s%s" % (name, c[kind], MEMORY_KIND_TEXT[kind], "" if c[kind] == 1 else "s")
        first = [f for f in report.findings if f["kind"] == kind]
        if not first:
            lines.append(head)
            continue
        f = first[0]
        at = "row %d, addr %d, clk %d: " % (f["row"], f["addr"], f["clk"])
        if kind == "malformed":
            what = ", ".join(MEMORY_REASONS[b] for b in range(5) if f["reason"] >> b & 1)
        elif kind == "duplicate_static":
            what = "the record before it is a static record of this address"
        elif kind == "stale_read":
            what = "read %s, last write %s at row %d" % (memory_value(f["value"]), memory_value(f["expected"]), f["last_write"][2])
        else:
            what = "read %s, nothing written" % (memory_value(f["value"]),)
        lines.append("%s (%s%s)" % (head, at, what))
    lines.append("%s: %d live records (%d reads, %d writes, %d static) of %d addresses, %d same-cycle pair%s, largest clk gap %d, %d uninitialised zero read%s, dummy reads %d clk + %d addr, %s, %s" % (
        name, c["live"], c["reads"], c["writes"], c["statics"], c["addresses"], c["same_cycle_pairs"], "" if c["same_cycle_pairs"] == 1 else "s", c["max_clk_gap"], c["uninit_zero_reads"],
        "" if c["uninit_zero_reads"] == 1 else "s", c["dummy_reads_clk"], c["dummy_reads_addr"],
        "laid out sorted" if not c["layout_descents"] else "%d layout descent%s (the first at row %d)" % (c["layout_descents"], "" if c["layout_descents"] == 1 else "s", report.first_descent[1]),
        "no finding" if not c["findings"] else "%d finding%s" % (c["findings"], "" if c["findings"] == 1 else "s")))
    return lines


def check_status(balanced, creport, mreport, preport=None, areport=None):
    """The exit status of `check`: 1 for an unbalanced bus, a failing constraint (with --constraints), a memory finding (with --memory), a
    hard program finding (with --program; wrapped operands never count) or a hard arithmetic finding (with --arithmetic; soft ones never count)."""
    return 0 if balanced and (creport is None or creport.satisfied) and (mreport is None or mreport.total_findings == 0) and (preport is None or preport.total_hard == 0) and (
        areport is None or areport.total_hard == 0) else 1


ARITHMETIC_SYMBOLS = ("+", "-", "*", "/", "<", "<<", ">>", "&", "|", "^", "/s", "!=", "*hu", ">>s", "*hs", "<=", "==", "<s", "<=s")


def arithmetic_words(f):
    """(x, y, z) of a listed finding as integers; a malformed record's fields do not make words: None."""
    if f["kind"] == "malformed":
        return None
    return tuple(int.from_bytes(bytes(f[k]), "big") for k in ("x", "y", "z"))


def arithmetic_lines(report, basic=True):
    """One line per hard kind of an arithmetic report (the count and the first listed finding of the kind), one per soft kind, then one
    summary line with the counters.  basic: the chips are the BasicMachine's and go by their names."""
    import valida_amd as va

    def chip(f):
        return va.CHIP_NAMES[f["chip"]] if basic else "chip %d" % f["chip"]

    def what(f):
        name = va.ARITHMETIC_OPCODES[f["opcode"] - 100]
        where = "row %d%s, %s" % (f["row"], ", sent" if f["is_send"] else "", name)
        if f["kind"] == "malformed":
            return "%s: fields %s are not bytes" % (where, ", ".join(str(1 + j) for j in range(12) if f["mask"] >> j & 1))
        x, y, z = arithmetic_words(f)
        expr = "%d %s %d = %d" % (x, ARITHMETIC_SYMBOLS[f["opcode"] - 100], y, z)
        if f["kind"] == "undefined":
            return "%s: %s, %s" % (where, expr, ("division by zero", "signed overflow", "shift amount of 32 or more")[f["mask"] - 1])
        return "%s: %s, expected %d" % (where, expr, f["expected"])

    c, lines = report.counters, []
    text = {"malformed": ("malformed record", "malformed records"), "undefined": ("undefined operation", "undefined operations"), "wrong_result": ("wrong result", "wrong results"),
            "shift_quotient": ("signed quotient by a power of two holds the arithmetic shift", "signed quotients by a power of two hold the arithmetic shift"),
            "arithmetic_shr": ("SHR32 record holds the arithmetic shift", "SHR32 records hold the arithmetic shift")}
    for kinds, listed in ((va.ARITHMETIC_HARD_KINDS, report.hard), (va.ARITHMETIC_SOFT_KINDS, report.soft)):
        for kind in kinds:
            if not c[kind]:
                continue
            first = [f for f in listed if f["kind"] == kind]
            head = "%d %s" % (c[kind], text[kind][c[kind] != 1])
            lines.append("%s: %s (%s)" % (chip(first[0]), head, what(first[0])) if first else "alu: " + head)
    ops = ", ".join("%s %d" % (name, n) for name, n in report.opcodes.items() if n)
    lines.append("alu: %d live records in %d slots of %d entries, %d judged (%s), %d other, %d MULHS32 records where the sign matters, %d soft, %s" % (
        c["live"], c["slots"], len(report.entries), c["judged"], ops or "none", c["other"], c["mulhs_sign_matters"], c["soft"],
        "no finding" if not c["hard"] else "%d finding%s" % (c["hard"], "" if c["hard"] == 1 else "s")))
    return lines


PROGRAM_FIELD_NAMES = ("opcode", "operand a", "operand b", "operand c", "operand d", "operand e")


def program_field(j, short=False):
    """Field j of a fetch as the BasicMachine names it (opcode, a..e); beyond those its index."""
    name = PROGRAM_FIELD_NAMES[j] if j < len(PROGRAM_FIELD_NAMES) else "field %d" % j
    return name.split(" ")[-1] if short else name


def program_lines(report):
    """One line per hard kind of a program report (the count and the first listed finding of the kind), one for the wrapped operands, then one
    summary line with the counters and the first unfetched ranges."""
    import valida_amd as va

    c, lines = report.counters, []
    fetcher = va.CHIP_NAMES[report.fetch_chip] if (report.fetch_chip, report.table_chip) == (0, 1) else "chip %d" % report.fetch_chip
    table = va.CHIP_NAMES[report.table_chip] if (report.fetch_chip, report.table_chip) == (0, 1) else "chip %d" % report.table_chip
    text = {"table_key": ("wrong table key", "wrong table keys"), "pc_out_of_rom": ("pc outside the ROM", "pcs outside the ROM"), "wrong_instruction": ("wrong instruction", "wrong instructions"),
            "multiplicity": ("wrong multiplicity", "wrong multiplicities")}
    for kind in va.PROGRAM_HARD_KINDS:
        if not c[kind]:
            continue
        head = "%s: %d %s" % (table if kind in ("table_key", "multiplicity") else fetcher, c[kind], text[kind][c[kind] != 1])
        first = [f for f in report.hard if f["kind"] == kind]
        if not first:
            lines.append(head)
            continue
        f = first[0]
        if kind == "table_key":
            what = "row %d: key %d" % (f["row"], f["found"][0])
        elif kind == "pc_out_of_rom":
            what = "row %d, pc %d, ROM length %d" % (f["row"], f["pc"], c["rom_len"])
        elif kind == "wrong_instruction":
            what = "row %d, pc %d: %s" % (f["row"], f["pc"], ", ".join("%s %d, ROM %d" % (program_field(j), f["found"][j], f["expected"][j]) for j in f["fields"]))
        else:
            what = "word %d: multiplicity %d, fetched %d times" % (f["row"], f["found"][0], f["expected"][1])
        lines.append("%s (%s)" % (head, what))
    if c["wrapped_operand"]:
        head = "%s: %d fetch%s from the ROM only by 2^32 in an immediate" % (fetcher, c["wrapped_operand"], " differs" if c["wrapped_operand"] == 1 else "es differ")
        if report.wrapped:
            f = report.wrapped[0]
            head += " (first row %d, pc %d, fields %s)" % (f["row"], f["pc"], ", ".join(program_field(j, short=True) for j in f["fields"]))
        lines.append(head)
    if c["unfetched_words"]:
        shown = ", ".join("[%d, %d)" % r for r in report.unfetched[:4])
        words = "%d of %d words never fetched%s" % (c["unfetched_words"], c["rom_len"], " (%s%s)" % (shown, ", .." if c["unfetched_ranges"] > min(4, len(report.unfetched)) else "") if shown else "")
    else:
        words = "all words fetched"
    lines.append("%s: %d fetches of a %d-word ROM (%d table rows): %s, hottest pc %d (%d fetches), %d sequential, %d stay, %d jumps, pc %d to %d, %s" % (
        fetcher, c["fetches"], c["rom_len"], c["table_rows"], words, c["hottest_pc"], c["hottest_count"], c["sequential"], c["stay"], c["jumps"], c["first_pc"], c["last_pc"],
        "no finding" if not c["hard"] else "%d finding%s" % (c["hard"], "" if c["hard"] == 1 else "s")))
    return lines


def field_lines(report):
    """One line per (chip, interaction) of a field report with a floating field: the bus, the fields, the most rows one of them floats on."""
    import valida_amd as va

    lines = []
    for c in report.chips:
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        for r in c["records"]:
            fl = [j for j, n in enumerate(r["floating"]) if n]
            if not fl:
                continue
            key = (1 if r["is_global"] else 0, r["bus_index"])
            bus = "the %s bus" % va.BUS_NAMES[key] if key in va.BUS_NAMES else "bus (%s, %d)" % ("global" if key[0] else "local", key[1])
            lines.append("%s: interaction %d (%s on %s): field%s %s float%s on %d of %d live row%s" % (
                name, r["interaction"], "sends" if r["is_send"] else "receives", bus, "" if len(fl) == 1 else "s", index_ranges(fl), "s" if len(fl) == 1 else "",
                max(r["floating"]), r["live_rows"], "" if r["live_rows"] == 1 else "s"))
    return lines


def link_lines(report):
    """One line per bus of a link report with an open tuple (open and total tuples, the open positions), then one per (chip, interaction)
    whose floating fields are not all answered (the open fields, the most open rows of one of them, the most floating rows)."""
    import valida_amd as va

    def bus_name(key):
        return "%s bus" % va.BUS_NAMES[key] if key in va.BUS_NAMES else "bus (%s, %d)" % ("global" if key[0] else "local", key[1])

    lines = []
    for b in report.buses:
        if not b["open_tuples"]:
            continue
        pos = [j for j, n in enumerate(b["open_in"]) if n]
        lines.append("%s: %d of %d tuple%s open; open position%s %s" % (bus_name(tuple(b["bus"])), b["open_tuples"], b["tuples"], "" if b["tuples"] == 1 else "s",
                                                                    "" if len(pos) == 1 else "s", index_ranges(pos)))
    for c in report.chips:
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        for r in c["records"]:
            op = [j for j, n in enumerate(r["open"]) if n]
            if not op:
                continue
            key = (1 if r["is_global"] else 0, r["bus_index"])
            lines.append("%s: interaction %d (%s on the %s): field%s %s open on %d of %d floating row%s" % (
                name, r["interaction"], "sends" if r["is_send"] else "receives", bus_name(key), "" if len(op) == 1 else "s", index_ranges(op), max(r["open"]), max(r["floating"]),
                "" if max(r["floating"]) == 1 else "s"))
    return lines


def coverage_lines(report):
    """One line per chip of a coverage report that has a dead or shadowed detector: the dead constraints / interactions by index, those that
    are never the only detector of a mutation, and how many detectors are essential."""
    import valida_amd as va

    def plural(n, word):
        return "%d %s%s" % (n, word, "" if n == 1 else "s")

    lines = []
    for c in report.chips:
        (dc, di), (sc, si), (ec, ei) = report.dead(c["chip"]), report.shadowed(c["chip"]), report.essential(c["chip"])
        if not (dc or di or sc or si):
            continue
        name = va.CHIP_NAMES[c["chip"]] if c["chip"] < len(va.CHIP_NAMES) else "chip %d" % c["chip"]
        parts = []
        if dc:
            parts.append("dead constraints " + index_ranges(dc))
        if di:
            parts.append("dead interactions " + index_ranges(di))
        if sc or si:
            parts.append("never the only detector: " + " and ".join(([("constraints " + index_ranges(sc))] if sc else []) + ([("interactions " + index_ranges(si))] if si else [])))
        ess = ([plural(len(ec), "constraint")] if ec else []) + ([plural(len(ei), "interaction")] if ei else [])
        parts.append(" and ".join(ess) + " essential" if ess else "no detector essential")
        lines.append("%s: %s" % (name, "; ".join(parts)))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m valida_amd.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("action", choices=["run", "prove", "verify", "check"])
    ap.add_argument("program")
    ap.add_argument("action_file")
    ap.add_argument("advice", nargs="?", default=None)
    ap.add_argument("--stack-height", type=int, default=16777216)
    ap.add_argument("--max-cycles", type=int, default=1 << 22)
    ap.add_argument("--device", type=int, default=None, help="GPU for prove (default 0) / verify (default: the host verifier)")
    ap.add_argument("--host", action="store_true", help="check: host traces and the host audit (no GPU)")
    ap.add_argument("--max-tuples", type=int, default=64)
    ap.add_argument("--max-records", type=int, default=4)
    ap.add_argument("--constraints", action="store_true", help="check: also the constraint audit (which AIR constraints fail on which rows)")
    ap.add_argument("--max-constraints", type=int, default=64)
    ap.add_argument("--mutations", action="store_true", help="check: also the mutation audit (which trace cells no constraint or bus binds)")
    ap.add_argument("--deltas", default="1,-1", help="check --mutations / --coverage / --pairs: 1 to 4 distinct deltas, comma-separated integers mod p (as --deltas=1,-1)")
    ap.add_argument("--coverage", action="store_true", help="check: also the coverage audit (which constraint or bus interaction detects each mutation; "
                    "dead = not reached by this witness, not a fault; never changes the exit status)")
    ap.add_argument("--pairs", action="store_true", help="check: also the pair audit (two cells of one row that can change together unnoticed although one "
                    "alone is noticed; never changes the exit status)")
    ap.add_argument("--rank", action="store_true", help="check: also the rank audit (per row the null space of the Jacobian of all constraints and bus records: "
                    "every first-order degree of freedom; never changes the exit status)")
    ap.add_argument("--fields", action="store_true", help="check: also the field audit (per live bus record the fields the chip's constraints leave undetermined to "
                    "first order on this witness; a floating field on a send usually means the chip delegates; never changes the exit status)")
    ap.add_argument("--links", action="store_true", help="check: also the link audit (the bus tuple positions that float at every record of the tuple, send or receive: "
                    "no chip on the bus pins them; first order, on this witness, each record judged alone; never changes the exit status)")
    ap.add_argument("--steps", action="store_true", help="check: also the step audit (finite steps along each row's null directions: which of the rank audit's "
                    "freedoms are trades every check accepts, which are first-order artefacts; never changes the exit status)")
    ap.add_argument("--invariants", action="store_true", help="check: also the invariant audit (the affine-linear relations every row of a chip keeps on this witness, "
                    "and on how many rows the chip's own constraints and bus records enforce each: never enforced = a candidate missing constraint or a column the "
                    "program never exercises; affine-linear only, one row, this witness, per basis vector, first order; never changes the exit status)")
    ap.add_argument("--transitions", action="store_true", help="check: also the transition audit (the affine-linear relations between a row and its successor that this "
                    "witness keeps on every window or under a boolean gate, and the windows at which the chip's constraints hold each: never held = a candidate missing "
                    "transition constraint; affine-linear only, single gates, this witness, per basis vector, first order, one row at a time; never changes the exit status)")
    ap.add_argument("--products", action="store_true", help="check: also the product audit (the products of two independent columns that are an affine function of the row "
                    "on every row of this witness — b^2 = b, s t = 0, s t = s, s x = y, a b = c — and on how many rows the chip's own constraints and bus records enforce each: "
                    "never enforced = a candidate missing constraint; single products, one row, this witness, first order; never changes the exit status)")
    ap.add_argument("--domains", action="store_true", help="check: also the domain audit (per main column the set of values this witness puts there, and the narrow — byte or "
                    "half-word valued — columns with a non-zero cell on a row where no live bare send to a lookup table guards them: a candidate missing range check; this witness, bare "
                    "fields only; never changes the exit status)")
    ap.add_argument("--max-bits", type=int, default=16, help="check --domains: a column is narrow when its largest value is below 2^N (1 to 16, default 16)")
    ap.add_argument("--lookup-buses", default="", help="check --domains: the buses that count as lookup tables instead of the structural rule, comma-separated (3 or g3: global bus 3, l0: local bus 0)")
    ap.add_argument("--memory", action="store_true", help="check: also the memory audit (the receives of the memory bus replayed as a memory: malformed records, duplicate static "
                    "records, reads that do not return the last write to their address, reads of a non-zero value from an address nobody wrote; definite faults: check exits 1 on a finding)")
    ap.add_argument("--program", dest="program_audit", action="store_true", help="check: also the program audit (every cpu row's instruction held against the program ROM at its pc, the ROM's multiplicities against "
                    "the fetch counts: the reference's commented-out program bus replayed; check exits 1 on a hard finding, fetches that differ only by 2^32 in an immediate are listed apart)")
    ap.add_argument("--arithmetic", action="store_true", help="check: also the arithmetic audit (every live record of the general bus recomputed in 32-bit integer arithmetic: malformed "
                    "records, undefined operations, wrong results; check exits 1 on a hard finding, the reference's two SRA conventions are listed apart)")
    ap.add_argument("--sides", choices=("receives", "sends", "both"), default="receives", help="check --arithmetic: judge the ALU chips' receives (default), the senders' records, or both")
    ap.add_argument("--max-findings", type=int, default=64, help="check --memory, --program, --arithmetic: the findings listed (default 64, at most 2^20; the counts stay exact)")
    ap.add_argument("--min-gate-windows", type=int, default=64, help="check --transitions: a gate that holds on fewer windows is counted but not audited (default 64)")
    ap.add_argument("--max-gates", type=int, default=256, help="check --transitions: the gates listed per chip, the ungated one included (default 256)")
    ap.add_argument("--step-sizes", default="1,-1,2", help="check --steps: 1 to 4 distinct step sizes, comma-separated integers mod p (as --step-sizes=1,-1,2)")
    ap.add_argument("--chips", default="", help="check --pairs / --rank / --fields / --steps / --invariants / --transitions / --products / --domains: audit only these chips, comma-separated names or indices (as --chips=cpu,add)")
    _config_flags(ap)
    args = ap.parse_args(argv)

    if args.action == "verify":
        from valida_amd import verify_cli

        flags = ["--program-file", args.program, "--log-blowup", str(args.log_blowup), "--queries", str(args.queries), "--pow-bits", str(args.pow_bits),
                 "--constants", args.constants] + (["--poseidon-mmcs"] if args.poseidon_mmcs else []) + (
                     ["--device", str(args.device)] if args.device is not None else [])
        return verify_cli.main([args.action_file] + flags)

    import valida_amd as va

    try:
        t0 = time.perf_counter()
        exe = open(args.program, "rb").read()
        advice = open(args.advice, "rb").read() if args.advice else b""
        w = va.Workload.from_executable(exe, advice=advice, stack_height=args.stack_height, max_cycles=args.max_cycles)
        vm_ms = (time.perf_counter() - t0) * 1e3
        if args.action == "run":
            with open(args.action_file, "wb") as f:
                f.write(w.output())
            return 0
        if args.action == "check":
            if args.host:
                report = va.bus_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_tuples=args.max_tuples, max_records_per_tuple=args.max_records)
                creport = va.constraint_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_constraints=args.max_constraints) if args.constraints else None
                mreport = va.mutation_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), deltas=parse_deltas(args.deltas), max_entries=1 << 20) if args.mutations else None
                kreport = va.coverage_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), deltas=parse_deltas(args.deltas), max_cells=1 << 20) if args.coverage else None
                preport = va.pair_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), deltas=parse_deltas(args.deltas), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.pairs else None
                rreport = va.rank_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.rank else None
                freport = va.field_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.fields else None
                lreport = va.link_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_tuples=args.max_tuples, max_records_per_tuple=args.max_records) if args.links else None
                sreport = va.step_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), steps=parse_deltas(args.step_sizes), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.steps else None
                ireport = va.invariant_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_entries=1 << 20, max_terms=256, chips=parse_chips(args.chips)) if args.invariants else None
                treport = va.transition_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_terms=256, min_gate_windows=args.min_gate_windows, max_gates=args.max_gates,
                                                   chips=parse_chips(args.chips)) if args.transitions else None
                qreport = va.product_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_entries=1 << 20, max_terms=256, chips=parse_chips(args.chips)) if args.products else None
                dreport = va.domain_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_entries=1 << 20, chips=parse_chips(args.chips), max_bits=args.max_bits,
                                               lookup_buses=parse_lookup_buses(args.lookup_buses)) if args.domains else None
                memreport = va.memory_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_findings=args.max_findings) if args.memory else None
                progreport = va.program_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), rom_len=w.program_len, max_findings=args.max_findings) if args.program_audit else None
                arreport = va.arithmetic_audit_host(va.Machine.basic(), w.main_traces(), w.preprocessed(), max_findings=args.max_findings, sides=args.sides) if args.arithmetic else None
            else:
                prover = va.Prover(va.Machine.basic(), va.poseidon_round_constants(source=args.constants), device=args.device or 0)
                log = prover.upload_oplog(w.oplog())
                main = [prover.generate_trace(log, chip) for chip in range(va.NUM_CHIPS)]
                prep = [(chip, prover.upload(m)) for chip, m in w.preprocessed()]
                report = prover.bus_audit(main, prep, max_tuples=args.max_tuples, max_records_per_tuple=args.max_records)
                creport = prover.constraint_audit(main, prep, max_constraints=args.max_constraints) if args.constraints else None
                mreport = prover.mutation_audit(main, prep, deltas=parse_deltas(args.deltas), max_entries=1 << 20) if args.mutations else None
                kreport = prover.coverage_audit(main, prep, deltas=parse_deltas(args.deltas), max_cells=1 << 20) if args.coverage else None
                preport = prover.pair_audit(main, prep, deltas=parse_deltas(args.deltas), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.pairs else None
                rreport = prover.rank_audit(main, prep, max_entries=1 << 20, chips=parse_chips(args.chips)) if args.rank else None
                freport = prover.field_audit(main, prep, max_entries=1 << 20, chips=parse_chips(args.chips)) if args.fields else None
                lreport = prover.link_audit(main, prep, max_tuples=args.max_tuples, max_records_per_tuple=args.max_records) if args.links else None
                sreport = prover.step_audit(main, prep, steps=parse_deltas(args.step_sizes), max_entries=1 << 20, chips=parse_chips(args.chips)) if args.steps else None
                ireport = prover.invariant_audit(main, prep, max_entries=1 << 20, max_terms=256, chips=parse_chips(args.chips)) if args.invariants else None
                treport = prover.transition_audit(main, prep, max_terms=256, min_gate_windows=args.min_gate_windows, max_gates=args.max_gates, chips=parse_chips(args.chips)) if args.transitions else None
                qreport = prover.product_audit(main, prep, max_entries=1 << 20, max_terms=256, chips=parse_chips(args.chips)) if args.products else None
                dreport = prover.domain_audit(main, prep, max_entries=1 << 20, chips=parse_chips(args.chips), max_bits=args.max_bits, lookup_buses=parse_lookup_buses(args.lookup_buses)) if args.domains else None
                memreport = prover.memory_audit(main, prep, max_findings=args.max_findings) if args.memory else None
                progreport = prover.program_audit(main, prep, rom_len=w.program_len, max_findings=args.max_findings) if args.program_audit else None
                arreport = prover.arithmetic_audit(main, prep, max_findings=args.max_findings, sides=args.sides) if args.arithmetic else None
            text = report.to_json()
            if creport is not None:
                text = json.dumps(dict(json.loads(text), constraints=creport.to_dict()))
            if mreport is not None:
                text = json.dumps(dict(json.loads(text), mutations=mreport.to_dict()))
            if kreport is not None:
                text = json.dumps(dict(json.loads(text), coverage=kreport.to_dict()))
            if preport is not None:
                text = json.dumps(dict(json.loads(text), pairs=preport.to_dict()))
            if rreport is not None:
                text = json.dumps(dict(json.loads(text), rank=rreport.to_dict()))
            if freport is not None:
                text = json.dumps(dict(json.loads(text), fields=freport.to_dict()))
            if lreport is not None:
                text = json.dumps(dict(json.loads(text), links=lreport.to_dict()))
            if sreport is not None:
                text = json.dumps(dict(json.loads(text), steps=sreport.to_dict()))
            if ireport is not None:
                text = json.dumps(dict(json.loads(text), invariants=ireport.to_dict()))
            if treport is not None:
                text = json.dumps(dict(json.loads(text), transitions=treport.to_dict()))
            if qreport is not None:
                text = json.dumps(dict(json.loads(text), products=qreport.to_dict()))
            if dreport is not None:
                text = json.dumps(dict(json.loads(text), domains=dreport.to_dict()))
            if memreport is not None:
                text = json.dumps(dict(json.loads(text), memory=memreport.to_dict()))
            if progreport is not None:
                text = json.dumps(dict(json.loads(text), program=progreport.to_dict()))
            if arreport is not None:
                text = json.dumps(dict(json.loads(text), arithmetic=arreport.to_dict()))
            with open(args.action_file, "w") as f:
                f.write(text + "\n")
            for line in report_lines(report, w.main_trace(0)) + (constraint_lines(creport, w.main_trace(0)) if creport is not None else []) + (mutation_lines(mreport) if mreport is not None else []) + (
                    coverage_lines(kreport) if kreport is not None else []) + (pair_lines(preport) if preport is not None else []) + (
                    rank_lines(rreport) if rreport is not None else []) + (field_lines(freport) if freport is not None else []) + (
                    link_lines(lreport) if lreport is not None else []) + (step_lines(sreport) if sreport is not None else []) + (
                    invariant_lines(ireport) if ireport is not None else []) + (transition_lines(treport) if treport is not None else []) + (
                    product_lines(qreport) if qreport is not None else []) + (domain_lines(dreport) if dreport is not None else []) + (memory_lines(memreport) if memreport is not None else []) + (
                    program_lines(progreport) if progreport is not None else []) + (arithmetic_lines(arreport) if arreport is not None else []):
                print(line)
            return check_status(report.balanced, creport, memreport, progreport, arreport)
        hash_kind = va.HASH_POSEIDON16 if args.poseidon_mmcs else va.HASH_KECCAK256
        rc = va.poseidon_round_constants(source=args.constants)
        prover = va.Prover(va.Machine.basic(), rc, device=args.device or 0, log_blowup=args.log_blowup, num_queries=args.queries, pow_bits=args.pow_bits,
                           hash_kind=hash_kind)
        proof, _, times = prove_on_device(w, prover)
        t = time.perf_counter()
        with open(args.action_file, "wb") as f:
            f.write(proof.cbor())
        times = dict(vm_ms=vm_ms, **times, write_ms=(time.perf_counter() - t) * 1e3)
        times["total_ms"] = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(cycles=w.cycles, cpu_height=w.cpu_height, proof_words=int(proof.words.size),
                              **{k: round(v, 3) for k, v in times.items()})), file=sys.stderr)
        print("Proof successful")
        return 0
    except (va.VgpuError, OSError) as e:
        print("%s: %s" % (args.action, e), file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
