// Mutation audit: WHICH cells of a witness could be changed without any AIR constraint or bus noticing — mutation testing of the AIRs on one
// witness, the converse question to the bus audit (host/bus_audit.hpp) and the constraint audit (host/constraint_audit.hpp).
//   mutation      chip h with main matrix M (height n, width w), a row r, a main column c and a delta d: M' = M except M'[r][c] = M[r][c] + d mod p.
//                 Preprocessed columns are never mutated.
//   AIR-detected  Air::eval of the chip on M' at rows r and (r - 1) mod n, over the constraint audit's domain (next = (row + 1) mod n, is_first /
//                 is_last / is_transition as 0/1 values): some constraint is non-zero there that was zero at the same row on M (newly failing).
//                 For n = 1 the two rows are one row and the mutated cell is seen as `local` and as `next` in one evaluation.  The permutation
//                 constraints are not evaluated; the bus rule is their exact statement.
//   bus-detected  every interaction of the chip on row r in Chip::all_interactions order, for M and for M': an interaction of count 0 is no
//                 record, otherwise the record is (count, fields), canonical; detected when the record of some interaction differs.
//   counts        per (chip, column, delta index), exact over all n rows: air, bus, free (rows that are neither).  A column is UNBOUND when
//                 free = n for every delta.
// Evaluations that the chip's compiled Program proves cannot matter are skipped: a column that no constraint reads as `local` is not evaluated
// at row r, one never read as `next` not at row r - 1, one in no interaction not on the bus (ma_column_flags).  The report is that of the
// definition.  It is a statement about single-cell slack on THIS witness, not a soundness proof.
// This header holds what the host and the device implementation share — options, the column flags, the report and its flat word image — and
// the host implementation over canonical row-major matrices (plain C++, one thread, no device, any number of constraints).  The device pass is
// Prover::mutation_audit (prover_audits.cpp, kernels/mutation_audit.hip).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>
#include "constraint_audit.hpp"

namespace vhost {

constexpr uint32_t MA_MAX_DELTAS = 4;

struct MutationAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t n_deltas = 0;  // 0: the default pair {1, p - 1}
    uint32_t deltas[MA_MAX_DELTAS] = {0, 0, 0, 0};
    uint32_t reserved[2] = {0, 0};
};

struct MutationChipStat {
    uint32_t width = 0, n_constraints = 0, unbound = 0;
    uint64_t height = 0;
    uint64_t free_[MA_MAX_DELTAS] = {0, 0, 0, 0}, air[MA_MAX_DELTAS] = {0, 0, 0, 0}, bus[MA_MAX_DELTAS] = {0, 0, 0, 0};  // sums over the chip's columns
};
struct MutationEntry {
    uint32_t chip = 0, column = 0, delta = 0;  // delta: index into the deltas
    uint64_t free_ = 0, air = 0, bus = 0;
    std::vector<uint32_t> rows;  // the first max_rows_per_entry free rows, ascending
};
struct MutationReport {
    std::vector<uint32_t> deltas;  // canonical
    bool truncated = false;
    uint64_t total_entries = 0;             // (chip, column, delta) with free > 0, exact even when the list is cut
    std::vector<MutationChipStat> chips;    // one per chip of the machine
    std::vector<MutationEntry> entries;     // ascending (chip, column, delta index)
    double device_ms = 0;                   // the device pass (0 for the host implementation); not part of the word image
    double host_ms = 0;                     // wall time of the whole call
    double evaluations = 0;                 // Air::eval row evaluations performed (baselines included); not part of the word image
    static constexpr uint32_t MAGIC = 0x31524d56u;  // "VMR1"
    // Flat image (include/vgpu.h documents it next to vgpu_mutation_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        const uint32_t D = (uint32_t)deltas.size();
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(D); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) w.push_back(i < D ? deltas[i] : 0u);
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); u64(c.height); w.push_back(c.unbound); w.push_back(0);
            for (uint32_t i = 0; i < D; i++) { u64(c.free_[i]); u64(c.air[i]); u64(c.bus[i]); }
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.column); w.push_back(e.delta); w.push_back((uint32_t)e.rows.size());
            u64(e.free_); u64(e.air); u64(e.bus);
            for (uint32_t r : e.rows) w.push_back(r);
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline MutationAuditOpts mutation_audit_checked_opts(const MutationAuditOpts& in) {
    MutationAuditOpts o = in;
    if (o.reserved[0] != 0 || o.reserved[1] != 0) throw std::invalid_argument("mutation_audit: the reserved fields of the options must be zero");
    if (o.max_entries == 0) o.max_entries = 1024;
    if (o.max_rows_per_entry == 0) o.max_rows_per_entry = 4;
    if (o.max_entries > (1ull << 24) || o.max_rows_per_entry > 4096) throw std::invalid_argument("mutation_audit: max_entries is at most 2^24 and max_rows_per_entry at most 4096");
    if (o.n_deltas == 0) { o.n_deltas = 2; o.deltas[0] = 1; o.deltas[1] = vg::P - 1; o.deltas[2] = o.deltas[3] = 0; }
    if (o.n_deltas > MA_MAX_DELTAS) throw std::invalid_argument("mutation_audit: at most " + std::to_string(MA_MAX_DELTAS) + " deltas (got " + std::to_string(o.n_deltas) + ")");
    for (uint32_t i = 0; i < o.n_deltas; i++) {
        if (o.deltas[i] == 0 || o.deltas[i] >= vg::P) throw std::invalid_argument("mutation_audit: a delta must be a canonical value in 1..p-1 (delta " + std::to_string(i) + ": " + std::to_string(o.deltas[i]) + ")");
        for (uint32_t j = 0; j < i; j++)
            if (o.deltas[j] == o.deltas[i]) throw std::invalid_argument("mutation_audit: the deltas must be distinct (" + std::to_string(o.deltas[i]) + " is repeated)");
    }
    return o;
}

// Validates the shapes as the other audits do (their messages, under this audit's name) and that every column an interaction reads lies
// inside its trace.  prep_slot[chip] = index into the preprocessed list or -1.
inline void mutation_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                std::vector<int>& prep_slot) {
    try {
        constraint_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what(), from = "constraint_audit: ";
        throw std::invalid_argument(m.compare(0, from.size(), from) == 0 ? "mutation_audit: " + m.substr(from.size()) : m);
    }
    for (const AirDesc& a : machine.airs)
        for (auto& it : a.interactions) {
            auto check = [&](const vair::VirtualCol& v) {
                for (auto& t : v.terms)
                    if (t.col < 0 || (uint32_t)t.col >= (t.preprocessed ? a.prep_width : a.width)) throw std::invalid_argument("mutation_audit: an interaction of chip " + a.name + " reads a column outside its trace");
            };
            check(it.count);
            for (auto& f : it.fields) check(f);
        }
}

// What the chip's compiled Program and its interactions prove about a main column: bit 0 some constraint reads it as `local`, bit 1 as `next`,
// bit 2 some interaction reads it.  A mutation of a column without bit 0 cannot change Air::eval at its own row, one without bit 1 not at the
// row before, one without bit 2 no bus record.
constexpr uint32_t MA_COL_LOCAL = 1, MA_COL_NEXT = 2, MA_COL_BUS = 4;
inline std::vector<uint32_t> ma_column_flags(const AirDesc& a) {
    std::vector<uint32_t> f(a.width ? a.width : 1, 0);
    for (const vair::Instr& in : a.program.instrs)
        if (in.op == vair::OP_LOAD_MAIN && in.a < a.width) f[in.a] |= in.flag ? MA_COL_NEXT : MA_COL_LOCAL;
    for (auto& it : a.interactions) {
        auto mark = [&](const vair::VirtualCol& v) {
            for (auto& t : v.terms)
                if (!t.preprocessed && t.col >= 0 && (uint32_t)t.col < a.width) f[(size_t)t.col] |= MA_COL_BUS;
        };
        mark(it.count);
        for (auto& v : it.fields) mark(v);
    }
    return f;
}
// What the interactions prove about the bus rule.  A virtual column is affine with constant weights, so adding d != 0 to main column c changes
// its value by d times the sum of c's weights in it: it changes iff that sum is non-zero mod p, on every row alike.  Per column two masks over
// the interactions (bit m = interaction m): [2 c] those whose COUNT changes, [2 c + 1] those with a FIELD that changes.  The mutation of a cell
// of column c is bus-detected iff the first mask is non-zero, or the second meets the interactions that are records (count != 0) on that row.
// Only for at most 32 interactions (`ok`); the device pass evaluates every interaction per mutation otherwise, as the host audit always does.
inline std::vector<uint32_t> ma_bus_masks(const AirDesc& a, bool& ok) {
    std::vector<uint32_t> m(2 * (size_t)(a.width ? a.width : 1), 0);
    ok = a.interactions.size() <= 32;
    if (!ok) return m;
    std::vector<uint64_t> sum(a.width ? a.width : 1);
    for (size_t i = 0; i < a.interactions.size(); i++) {
        auto changed = [&](const vair::VirtualCol& v, uint32_t which) {
            std::fill(sum.begin(), sum.end(), 0);
            for (auto& t : v.terms)
                if (!t.preprocessed && t.col >= 0 && (uint32_t)t.col < a.width) sum[(size_t)t.col] = (sum[(size_t)t.col] + t.weight % vg::P) % vg::P;
            for (uint32_t c = 0; c < a.width; c++)
                if (sum[c]) m[2 * (size_t)c + which] |= 1u << i;
        };
        changed(a.interactions[i].count, 0);
        for (auto& f : a.interactions[i].fields) changed(f, 1);
    }
    return m;
}

// Air::eval row evaluations of the audit of one chip: two baselines per row and, per delta, one per (row, column read as local) and one per
// (row, column read as next); for n = 1 one baseline and one per column read at all.
inline double ma_evaluations(const AirDesc& a, uint64_t n, uint32_t D) {
    if (!a.program.num_asserts) return 0;
    uint64_t per_row = 0;
    for (uint32_t f : ma_column_flags(a)) per_row += n == 1 ? ((f & 3u) ? 1 : 0) : ((f & MA_COL_LOCAL) ? 1 : 0) + ((f & MA_COL_NEXT) ? 1 : 0);
    return (double)n * ((double)per_row * D + (n == 1 ? 1 : 2));
}

// chips[].unbound and the sums, total_entries, truncated from the per-chip counts [(column * D + delta) * 3 + {free, air, bus}]; the entries
// (without rows) of the first max_entries (chip, column, delta) with free > 0
inline void mutation_audit_finish(MutationReport& r, const std::vector<std::vector<uint64_t>>& counts, const MutationAuditOpts& o) {
    const uint32_t D = o.n_deltas;
    r.deltas.assign(o.deltas, o.deltas + D);
    r.total_entries = 0;
    r.entries.clear();
    for (size_t c = 0; c < counts.size(); c++) {
        MutationChipStat& cs = r.chips[c];
        cs.unbound = 0;
        for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) cs.free_[i] = cs.air[i] = cs.bus[i] = 0;
        for (uint32_t col = 0; col < cs.width; col++) {
            bool unbound = true;
            for (uint32_t i = 0; i < D; i++) {
                const uint64_t* k = &counts[c][((size_t)col * D + i) * 3];
                cs.free_[i] += k[0]; cs.air[i] += k[1]; cs.bus[i] += k[2];
                if (k[0] != cs.height) unbound = false;
                if (!k[0]) continue;
                r.total_entries++;
                if (r.entries.size() < o.max_entries) { MutationEntry e; e.chip = (uint32_t)c; e.column = col; e.delta = i; e.free_ = k[0]; e.air = k[1]; e.bus = k[2]; r.entries.push_back(std::move(e)); }
            }
            if (unbound) cs.unbound++;
        }
    }
    r.truncated = r.total_entries > r.entries.size();
}

// The contract on the host: the chip's Program interpreted on the mutated rows, the interactions evaluated before and after; one thread.
inline MutationReport mutation_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                          const std::vector<ConstraintHostMatrix>& prep, const MutationAuditOpts& opts_in) {
    const MutationAuditOpts o = mutation_audit_checked_opts(opts_in);
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("mutation_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("mutation_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    mutation_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t D = o.n_deltas, R = o.max_rows_per_entry;
    MutationReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<uint64_t>> counts(NC);
    std::vector<std::vector<std::vector<uint32_t>>> first(NC);
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    vg::Fp dm[MA_MAX_DELTAS];
    for (uint32_t i = 0; i < D; i++) dm[i] = vg::Fp::from_canonical(o.deltas[i]);
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        const vair::Program& p = air.program;
        const uint32_t K = p.num_asserts, W = air.width, PW = air.prep_width;
        const ConstraintHostMatrix& mm = main[c];
        const uint64_t n = mm.height;
        rep.chips[c].width = W; rep.chips[c].n_constraints = K; rep.chips[c].height = n;
        rep.evaluations += ma_evaluations(air, n, D);
        counts[c].assign((size_t)W * D * 3, 0);
        first[c].resize((size_t)W * D);
        const ConstraintHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        const std::vector<uint32_t> flags = ma_column_flags(air);
        const size_t MW = (K + 63) / 64;
        std::vector<vg::Fp> regs(p.num_regs ? p.num_regs : 1);
        // Air::eval at row q with the given local / next rows (Montgomery).  base == nullptr: writes the fail mask to `out`; otherwise returns
        // whether some constraint is non-zero whose bit in `base` is clear.
        auto eval = [&](uint64_t q, const vg::Fp* ml, const vg::Fp* mn, const vg::Fp* pl, const vg::Fp* pn, const uint64_t* base, uint64_t* out) -> bool {
            uint32_t k = 0;
            for (const vair::Instr& in : p.instrs) {
                switch (in.op) {
                    case vair::OP_CONST: regs[in.dst] = vg::Fp::raw((uint32_t)in.a | ((uint32_t)in.b << 16)); break;
                    case vair::OP_LOAD_MAIN: regs[in.dst] = (in.flag ? mn : ml)[in.a]; break;
                    case vair::OP_LOAD_PREP: regs[in.dst] = (in.flag ? pn : pl)[in.a]; break;
                    case vair::OP_SEL_FIRST: regs[in.dst] = q == 0 ? one : zero; break;
                    case vair::OP_SEL_LAST: regs[in.dst] = q == n - 1 ? one : zero; break;
                    case vair::OP_SEL_TRANS: regs[in.dst] = q == n - 1 ? zero : one; break;
                    case vair::OP_ADD: regs[in.dst] = regs[in.a] + regs[in.b]; break;
                    case vair::OP_SUB: regs[in.dst] = regs[in.a] - regs[in.b]; break;
                    case vair::OP_MUL: regs[in.dst] = regs[in.a] * regs[in.b]; break;
                    case vair::OP_NEG: regs[in.dst] = -regs[in.a]; break;
                    case vair::OP_ASSERT:
                        if (!regs[in.a].is_zero()) {
                            if (!base) out[k >> 6] |= 1ull << (k & 63);
                            else if (!((base[k >> 6] >> (k & 63)) & 1ull)) return true;
                        }
                        k++;
                        break;
                    default: break;
                }
            }
            return false;
        };
        // rows in Montgomery form, row-major
        std::vector<vg::Fp> mont((size_t)n * W), pmont(pm ? (size_t)n * PW : 0);
        for (size_t i = 0; i < mont.size(); i++) mont[i] = vg::Fp::from_canonical(mm.data[i]);
        for (size_t i = 0; i < pmont.size(); i++) pmont[i] = vg::Fp::from_canonical(pm->data[i]);
        auto prow = [&](uint64_t q) -> const vg::Fp* { return pm ? pmont.data() + q * PW : nullptr; };
        std::vector<uint64_t> base(K ? (size_t)n * MW : 0, 0);
        if (K)
            for (uint64_t q = 0; q < n; q++) { const uint64_t nx = (q + 1) & (n - 1); eval(q, mont.data() + q * W, mont.data() + nx * W, prow(q), prow(nx), nullptr, base.data() + q * MW); }
        auto vcol = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* pr) {
            uint64_t acc = v.constant % vg::P;
            for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? pr : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
            return (uint32_t)acc;
        };
        std::vector<vg::Fp> cur(W ? W : 1);
        std::vector<uint32_t> mut(W ? W : 1);
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t rp = (r + n - 1) & (n - 1), nx = (r + 1) & (n - 1);
            const uint32_t* crow = mm.data + r * W;
            const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
            for (uint32_t col = 0; col < W; col++) cur[col] = mont[r * W + col];
            for (uint32_t col = 0; col < W; col++) {
                const uint32_t fl = flags[col];
                for (uint32_t i = 0; i < D; i++) {
                    bool a_det = false, b_det = false;
                    if (K && (fl & (MA_COL_LOCAL | MA_COL_NEXT))) {
                        cur[col] = mont[r * W + col] + dm[i];
                        if (n == 1) a_det = eval(0, cur.data(), cur.data(), prow(0), prow(0), base.data(), nullptr);
                        else {
                            if (fl & MA_COL_LOCAL) a_det = eval(r, cur.data(), mont.data() + nx * W, prow(r), prow(nx), base.data() + r * MW, nullptr);
                            if (!a_det && (fl & MA_COL_NEXT)) a_det = eval(rp, mont.data() + rp * W, cur.data(), prow(rp), prow(r), base.data() + rp * MW, nullptr);
                        }
                        cur[col] = mont[r * W + col];
                    }
                    if (fl & MA_COL_BUS) {
                        for (uint32_t k = 0; k < W; k++) mut[k] = crow[k];
                        mut[col] = (uint32_t)(((uint64_t)crow[col] % vg::P + o.deltas[i]) % vg::P);
                        for (auto& it : air.interactions) {
                            const uint32_t c0 = vcol(it.count, crow, cprow), c1 = vcol(it.count, mut.data(), cprow);
                            if (c0 != c1) { b_det = true; break; }
                            if (!c0) continue;
                            for (auto& f : it.fields)
                                if (vcol(f, crow, cprow) != vcol(f, mut.data(), cprow)) { b_det = true; break; }
                            if (b_det) break;
                        }
                    }
                    uint64_t* k = &counts[c][((size_t)col * D + i) * 3];
                    if (a_det) k[1]++;
                    if (b_det) k[2]++;
                    if (!a_det && !b_det && k[0]++ < R) first[c][(size_t)col * D + i].push_back((uint32_t)r);
                }
            }
        }
    }
    mutation_audit_finish(rep, counts, o);
    for (auto& e : rep.entries) e.rows = std::move(first[e.chip][(size_t)e.column * o.n_deltas + e.delta]);
    return rep;
}

}  // namespace vhost
