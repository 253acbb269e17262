// Program audit: do the instruction fetches of a witness match its program ROM?  The reference comments out both halves of the program bus:
// the cpu's send of (pc, opcode, a..e) with count one (cpu/src/lib.rs:138-157) and the program chip's receive of the preprocessed ROM row
// with count `multiplicity` (program/src/lib.rs:50-68); the program chip's AIR is empty, and the transcription follows it
// (chips/basic_machine.hpp, "bus commented out").  So nothing ties a cpu row's instruction to ROM[pc], and nothing ties the multiplicity
// column to how often a word ran: a witness whose cpu rows execute another program, every other record adjusted consistently, passes every
// other audit.  This audit replays the would-be bus exactly and names the fetches and multiplicities that break it.
//
// Contract (include/vgpu.h, "Program audit", states it for the C ABI):
//   inputs    what vgpu_prove and the audits take.  Options name the fetching chip (default 0, the cpu), its pc column (1) and its n_fields
//             (6, 1..8) field columns (3..8: opcode, a..e), the table chip (1, program), its preprocessed key column (0) and word columns
//             (1..6), its main multiplicity column (0) and rom_len (0: the table's height; the table's rows from rom_len on are padding and
//             not fetchable).
//   records   a FETCH is every row r of the fetching chip, padding rows included, count one: pc(r), f(r)[j].  A table row i has key K[i],
//             word W[i][j], multiplicity m[i].  c[i] = the fetches with pc(r) == i, for i below the table height.  Lookups are by row index;
//             values canonical.
//   findings  1 TABLE_KEY (a table row with K[i] != i), 2 PC_OUT_OF_ROM (a fetch with pc >= rom_len), 3 WRONG_INSTRUCTION (pc < rom_len and
//             some field differs from W[pc] by something other than 2^32 mod p), 4 WRAPPED_OPERAND (pc < rom_len, at least one field differs
//             and every differing field has f - W = 2^32 mod p: the unsigned and the signed embedding of one negative i32, cpu/src/lib.rs:
//             356-372 against the ROM's from_i32; counted and listed apart, never a fault), 5 MULTIPLICITY (m[i] != c[i] mod p).  mask: bit j
//             for every differing field, wrapped or not.  A fetch gets at most one of 2, 3, 4.  1, 2, 3, 5 are the HARD findings.  With
//             rom_len = the table's height there is no hard and no wrapped finding exactly when the reference's program bus, uncommented,
//             balances on this witness.
//   counters  exact: fetches, table rows, rom_len, fetched_words (i < rom_len with c[i] > 0), unfetched_words, unfetched_ranges (maximal
//             runs of unfetched words below rom_len), hottest_pc / hottest_count (the largest c[i] over the table's rows, the lowest i on a
//             tie; 0, 0 when no fetch hits the table), first_pc, last_pc, over the windows (r, r + 1): sequential (pc' = pc + 1 in the field),
//             stay (pc' = pc), jumps (the rest); one count per kind.
//   lists     findings: the first max_findings hard findings, TABLE_KEY by i, then the fetch findings by row, then MULTIPLICITY by i;
//             wrapped: the first max_findings WRAPPED_OPERAND rows; unfetched: the first max_ranges ranges [lo, hi), ascending.  Both limits
//             default to 64, are at most 2^20, and 0 lists nothing while every count stays exact.
// What it is not: it judges the fetches against the table of THIS witness only; not whether the opcode flags fit the opcode, not whether the
// step did what the opcode says (for the ALU results: host/arithmetic_audit.hpp), not whether the preprocessed commitment is the verifier's.
// This header holds the options check, the plan, the report with its image "VPG1" and the host twin (plain C++, one thread, no limits beyond
// the refusals).  The device pass is Prover::program_audit (prover_audits.cpp, kernels/program_audit.hip).
#pragma once
#include "bus_audit.hpp"

namespace vhost {

struct ProgramAuditOpts {
    uint32_t fetch_chip = 0, pc_col = 1, n_fields = 6;
    uint32_t field_cols[8] = {3, 4, 5, 6, 7, 8, 0, 0};
    uint32_t table_chip = 1, key_col = 0;
    uint32_t table_cols[8] = {1, 2, 3, 4, 5, 6, 0, 0};
    uint32_t mult_col = 0, rom_len = 0, max_findings = 64, max_ranges = 64, reserved = 0;
};

enum : uint32_t { PG_TABLE_KEY = 1, PG_PC_OUT_OF_ROM = 2, PG_WRONG_INSTRUCTION = 3, PG_WRAPPED_OPERAND = 4, PG_MULTIPLICITY = 5 };
constexpr uint32_t PG_TWO32 = (uint32_t)((1ull << 32) % vg::P);  // 268435454

struct ProgramFinding {
    uint32_t kind = 0, mask = 0, row = 0, pc = 0;  // row: the fetch row, or the table row of kinds 1 and 5 (pc = row there)
    uint32_t found[8] = {0, 0, 0, 0, 0, 0, 0, 0}, expected[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct ProgramReport {
    uint32_t fetch_chip = 0, table_chip = 1, n_fields = 6, max_findings = 64, max_ranges = 64, rom_len = 0;
    uint64_t fetches = 0, table_rows = 0, fetched_words = 0, unfetched_words = 0, unfetched_ranges = 0, hottest_count = 0;
    uint32_t hottest_pc = 0, first_pc = 0, last_pc = 0;
    uint64_t sequential = 0, stay = 0, jumps = 0, kinds[5] = {0, 0, 0, 0, 0};
    std::vector<ProgramFinding> findings, wrapped;
    std::vector<std::pair<uint32_t, uint32_t>> unfetched;
    double device_ms = 0, host_ms = 0, evaluations = 0;  // evaluations: fetches + table rows
    static constexpr uint32_t MAGIC = 0x31475056u;        // "VPG1"
    static constexpr uint32_t HEADER = 48, FINDING_WORDS = 24;
    uint64_t hard() const { return kinds[0] + kinds[1] + kinds[2] + kinds[4]; }
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0); w.push_back(fetch_chip); w.push_back(table_chip); w.push_back(n_fields);
        w.push_back((hard() > findings.size() ? 1u : 0u) | (kinds[3] > wrapped.size() ? 2u : 0u) | (unfetched_ranges > unfetched.size() ? 4u : 0u));
        w.push_back((uint32_t)findings.size()); w.push_back((uint32_t)wrapped.size()); w.push_back((uint32_t)unfetched.size());
        w.push_back(max_findings); w.push_back(max_ranges); w.push_back(rom_len);
        u64(fetches); u64(table_rows); u64(fetched_words); u64(unfetched_words); u64(unfetched_ranges);
        w.push_back(hottest_pc); w.push_back(0); u64(hottest_count); w.push_back(first_pc); w.push_back(last_pc);
        u64(sequential); u64(stay); u64(jumps); u64(hard());
        for (int k = 0; k < 5; k++) u64(kinds[k]);
        u64(0);
        for (const auto* list : {&findings, &wrapped})
            for (auto& f : *list) {
                w.push_back(f.kind); w.push_back(f.mask); w.push_back(f.row); w.push_back(f.pc);
                for (int k = 0; k < 8; k++) w.push_back(f.found[k]);
                for (int k = 0; k < 8; k++) w.push_back(f.expected[k]);
                for (int k = 0; k < 4; k++) w.push_back(0);
            }
        for (auto& r : unfetched) { w.push_back(r.first); w.push_back(r.second); }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

// What the passes read, after the refusals
struct ProgramPlan {
    uint64_t fetches = 0, table_rows = 0;
    uint32_t rom_len = 0;
    int table_prep = -1;  // the table chip's slot among the preprocessed traces
};

// Checks the options against the shapes (every refusal is std::invalid_argument with the reason), then the shapes as the bus audit does.
inline ProgramPlan program_audit_plan(const MachineDesc& machine, const std::vector<BusShape>& main, const std::vector<int>& prep_chips, const std::vector<BusShape>& prep,
                                      const ProgramAuditOpts& o) {
    auto refuse = [](const std::string& m) { throw std::invalid_argument("program_audit: " + m); };
    if (o.reserved) refuse("reserved must be zero");
    if (o.n_fields < 1 || o.n_fields > 8) refuse("n_fields is 1 to 8 (got " + std::to_string(o.n_fields) + ")");
    if (o.max_findings > (1u << 20) || o.max_ranges > (1u << 20)) refuse("max_findings and max_ranges are at most 2^20");
    std::vector<int> prep_slot;
    try {
        (void)bus_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what();
        // a table whose two traces differ in height and a height above 2^30 get this audit's words below; the rest keep the bus audit's
        const bool own = m.find("preprocessed trace shape mismatch") != std::string::npos || m.find("powers of two") != std::string::npos;
        if (!own || o.fetch_chip >= main.size() || o.table_chip >= main.size()) throw std::invalid_argument("program_audit" + (m.rfind("bus_audit", 0) == 0 ? m.substr(9) : ": " + m));
        for (size_t k = 0; k < prep_chips.size(); k++)
            if (prep_chips[k] == (int)o.table_chip && k < prep.size() && prep[k].height != main[o.table_chip].height)
                refuse("the table chip's main trace has " + std::to_string(main[o.table_chip].height) + " rows and its preprocessed trace " + std::to_string(prep[k].height) +
                       ": the multiplicities and the words must be one table");
        if (main[o.fetch_chip].height > (1ull << 30) || main[o.table_chip].height > (1ull << 30))
            refuse("fetch and table heights are at most 2^30 (" + std::to_string(main[o.fetch_chip].height) + ", " + std::to_string(main[o.table_chip].height) + ")");
        throw std::invalid_argument("program_audit" + (m.rfind("bus_audit", 0) == 0 ? m.substr(9) : ": " + m));
    }
    const size_t NC = machine.airs.size();
    if (o.fetch_chip >= NC) refuse("fetch_chip " + std::to_string(o.fetch_chip) + " is not a chip of the machine (" + std::to_string(NC) + " chips)");
    if (o.table_chip >= NC) refuse("table_chip " + std::to_string(o.table_chip) + " is not a chip of the machine (" + std::to_string(NC) + " chips)");
    const AirDesc& fa = machine.airs[o.fetch_chip];
    const AirDesc& ta = machine.airs[o.table_chip];
    if (prep_slot[o.table_chip] < 0) refuse("table chip " + ta.name + " has no preprocessed trace: there is no ROM to compare with");
    const BusShape& tp = prep[(size_t)prep_slot[o.table_chip]];
    if (o.pc_col >= fa.width) refuse("pc_col " + std::to_string(o.pc_col) + " is outside chip " + fa.name + "'s trace (width " + std::to_string(fa.width) + ")");
    for (uint32_t j = 0; j < o.n_fields; j++) {
        if (o.field_cols[j] >= fa.width)
            refuse("field column " + std::to_string(o.field_cols[j]) + " (field " + std::to_string(j) + ") is outside chip " + fa.name + "'s trace (width " + std::to_string(fa.width) + ")");
        if (o.table_cols[j] >= tp.width)
            refuse("table column " + std::to_string(o.table_cols[j]) + " (field " + std::to_string(j) + ") is outside chip " + ta.name + "'s preprocessed trace (width " + std::to_string(tp.width) + ")");
    }
    if (o.key_col >= tp.width) refuse("key_col " + std::to_string(o.key_col) + " is outside chip " + ta.name + "'s preprocessed trace (width " + std::to_string(tp.width) + ")");
    if (o.mult_col >= ta.width) refuse("mult_col " + std::to_string(o.mult_col) + " is outside chip " + ta.name + "'s trace (width " + std::to_string(ta.width) + ")");
    ProgramPlan p;
    p.fetches = main[o.fetch_chip].height; p.table_rows = main[o.table_chip].height; p.table_prep = prep_slot[o.table_chip];
    if (tp.height != p.table_rows) refuse("the table chip's main trace has " + std::to_string(p.table_rows) + " rows and its preprocessed trace " + std::to_string(tp.height));
    if (p.fetches > (1ull << 30) || p.table_rows > (1ull << 30)) refuse("fetch and table heights are at most 2^30");
    if (o.rom_len > p.table_rows) refuse("rom_len " + std::to_string(o.rom_len) + " is above the table's height " + std::to_string(p.table_rows));
    p.rom_len = o.rom_len ? o.rom_len : (uint32_t)p.table_rows;
    return p;
}

inline void program_audit_header(ProgramReport& rep, const ProgramPlan& plan, const ProgramAuditOpts& o) {
    rep.fetch_chip = o.fetch_chip; rep.table_chip = o.table_chip; rep.n_fields = o.n_fields; rep.max_findings = o.max_findings; rep.max_ranges = o.max_ranges;
    rep.rom_len = plan.rom_len; rep.fetches = plan.fetches; rep.table_rows = plan.table_rows; rep.evaluations = (double)(plan.fetches + plan.table_rows);
}

// ---- what the device pass and its emulation share (the layouts are stated in kernels/launch.hpp, program_audit.hip) ----
// tot: the passes' totals (PG_TOT u64); out: the listed records, 20 words each (the hard ones, then the wrapped ones); ranges: (lo, hi) pairs
inline void program_audit_from_device(ProgramReport& rep, const unsigned long long* tot, const uint32_t* out, size_t listed_hard, size_t listed_wrapped, const uint32_t* ranges,
                                      size_t listed_ranges) {
    rep.sequential = tot[0]; rep.stay = tot[1]; rep.jumps = tot[2];
    rep.kinds[1] = tot[3]; rep.kinds[2] = tot[4]; rep.kinds[3] = tot[5]; rep.first_pc = (uint32_t)tot[6]; rep.last_pc = (uint32_t)tot[7];
    rep.kinds[0] = tot[8]; rep.kinds[4] = tot[9]; rep.fetched_words = tot[10]; rep.unfetched_words = rep.rom_len - tot[10]; rep.unfetched_ranges = tot[11];
    if (tot[12]) { rep.hottest_count = tot[12] >> 32; rep.hottest_pc = ~(uint32_t)tot[12]; }
    for (size_t t = 0; t < listed_hard + listed_wrapped; t++) {
        const uint32_t* o = out + 20 * t;
        ProgramFinding f;
        f.kind = o[0]; f.mask = o[1]; f.row = o[2]; f.pc = o[3];
        for (int k = 0; k < 8; k++) { f.found[k] = o[4 + k]; f.expected[k] = o[12 + k]; }
        (t < listed_hard ? rep.findings : rep.wrapped).push_back(f);
    }
    for (size_t t = 0; t < listed_ranges; t++) rep.unfetched.push_back({ranges[2 * t], ranges[2 * t + 1]});
}

// The contract on the host: one walk over the fetches, one over the table.
inline ProgramReport program_audit_host(const MachineDesc& machine, const std::vector<BusHostMatrix>& main, const std::vector<int>& prep_chips, const std::vector<BusHostMatrix>& prep,
                                        const ProgramAuditOpts& o) {
    std::vector<BusShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("program_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("program_audit: null trace"); ps.push_back({m.height, m.width}); }
    const ProgramPlan plan = program_audit_plan(machine, ms, prep_chips, ps, o);
    ProgramReport rep;
    program_audit_header(rep, plan, o);
    const BusHostMatrix& fm = main[o.fetch_chip];
    const BusHostMatrix& tm = main[o.table_chip];
    const BusHostMatrix& tp = prep[(size_t)plan.table_prep];
    const uint64_t H = plan.fetches, T = plan.table_rows;
    auto cell = [](const BusHostMatrix& m, uint64_t r, uint32_t c) { return m.data[r * m.width + c] % vg::P; };
    std::vector<ProgramFinding> keys, fetch, mult;  // the three sections of the hard list, each cut at max_findings
    std::vector<uint64_t> c(T, 0);
    uint32_t prev = 0;
    for (uint64_t r = 0; r < H; r++) {
        const uint32_t pc = cell(fm, r, o.pc_col);
        if (pc < T) c[pc]++;
        if (r == 0) rep.first_pc = pc;
        else if (pc == (prev + 1 == vg::P ? 0u : prev + 1)) rep.sequential++;
        else if (pc == prev) rep.stay++;
        else rep.jumps++;
        prev = pc;
        ProgramFinding f;
        f.row = (uint32_t)r; f.pc = pc;
        bool hard = false;
        for (uint32_t j = 0; j < o.n_fields; j++) f.found[j] = cell(fm, r, o.field_cols[j]);
        if (pc >= plan.rom_len) {
            f.kind = PG_PC_OUT_OF_ROM;
        } else {
            for (uint32_t j = 0; j < o.n_fields; j++) {
                f.expected[j] = cell(tp, pc, o.table_cols[j]);
                if (f.found[j] == f.expected[j]) continue;
                f.mask |= 1u << j;
                if ((f.found[j] + vg::P - f.expected[j]) % vg::P != PG_TWO32) hard = true;
            }
            f.kind = !f.mask ? 0u : hard ? PG_WRONG_INSTRUCTION : PG_WRAPPED_OPERAND;
        }
        if (!f.kind) continue;
        rep.kinds[f.kind - 1]++;
        std::vector<ProgramFinding>& list = f.kind == PG_WRAPPED_OPERAND ? rep.wrapped : fetch;
        if (list.size() < o.max_findings) list.push_back(f);
    }
    rep.last_pc = prev;
    for (uint64_t i = 0; i < T; i++) {
        const uint32_t K = cell(tp, i, o.key_col), m = cell(tm, i, o.mult_col);
        if (c[i] > rep.hottest_count) { rep.hottest_count = c[i]; rep.hottest_pc = (uint32_t)i; }
        if (K != i) {
            rep.kinds[0]++;
            ProgramFinding f;
            f.kind = PG_TABLE_KEY; f.row = f.pc = (uint32_t)i; f.found[0] = K; f.expected[0] = (uint32_t)i;
            if (keys.size() < o.max_findings) keys.push_back(f);
        }
        if (m != c[i] % vg::P) {
            rep.kinds[4]++;
            ProgramFinding f;
            f.kind = PG_MULTIPLICITY; f.row = f.pc = (uint32_t)i; f.found[0] = m; f.expected[0] = (uint32_t)(c[i] % vg::P); f.expected[1] = (uint32_t)c[i];
            if (mult.size() < o.max_findings) mult.push_back(f);
        }
        if (i >= plan.rom_len) continue;
        if (c[i]) { rep.fetched_words++; continue; }
        rep.unfetched_words++;
        if (i == 0 || c[i - 1]) {
            rep.unfetched_ranges++;
            if (rep.unfetched.size() < o.max_ranges) rep.unfetched.push_back({(uint32_t)i, (uint32_t)i});
        }
        // the range this word extends is listed iff it is the newest listed one
        if (rep.unfetched_ranges <= rep.unfetched.size()) rep.unfetched.back().second = (uint32_t)i + 1;
    }
    for (const auto* list : {&keys, &fetch, &mult})
        for (auto& f : *list)
            if (rep.findings.size() < o.max_findings) rep.findings.push_back(f);
    return rep;
}

}  // namespace vhost
