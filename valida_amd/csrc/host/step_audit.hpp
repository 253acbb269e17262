// Step audit: finite steps along the null directions the rank audit (host/rank_audit.hpp) finds — the link between its first-order answer and
// the mutation audit's finite one (host/mutation_audit.hpp).  At row r of chip h every loose column c has a canonical null vector v of the
// row's Jacobian; the audit makes the finite move M[r] + t v for a few steps t and asks the mutation audit's question of it.
//   directions   exactly the rank audit's: J_r, its RREF, loose / pinned / zero / coupled and the canonical null vector of a loose column.  The
//                vector of a ZERO loose column is e_c (a zero column is a non-pivot column whose basis vector has no pivot entry).  Several
//                columns may share a vector (a pivot column takes the vector of its smallest non-pivot partner); results are per column.
//   move         step index s, t = steps[s]: M' = M except M'[r][j] = M[r][j] + t v_j mod p for every main column j.  Preprocessed columns never move.
//   detected     the mutation audit's two rules on M'.  AIR: Air::eval at q = r and q = (r - 1) mod n on the constraint audit's domain; some
//                constraint is non-zero there that was zero at the same row on M (n = 1: one evaluation, the row local and next at once;
//                permutation constraints are not evaluated).  Bus: the record of some interaction on row r differs.  v annihilates the count
//                row of every interaction and, on live rows, every field row, so the bus rule can never detect: this implementation
//                evaluates it all the same and counts it (bus_detected, per (row, loose column, step)); the device pass writes 0.
//   per cell     (row, loose column): pass mask, bit s = step s goes undetected.  EXACT: every step passes.  CURVED: some step is caught — a
//                first-order artefact (x^2 = 0 at x = 0).
//   per chip     max_degree (the machine's max_constraint_degree) and line_exact = [n_steps >= max_degree]: along the line t -> M[r] + t v
//                every constraint (at q = r and at q = r - 1) is a polynomial in t of degree <= max_degree; one that held on M is zero at
//                t = 0, so n_steps further zeros make max_degree + 1 zeros or more: it vanishes identically.  With line_exact an exact cell
//                is a whole line of witnesses on which no constraint that holds now fails, and no bus record changes.
// What it is not: one row, THIS witness, the canonical vectors only (not the whole null space); line_exact speaks of constraints that held;
// cross-row combinations are not looked for.
// This header holds what host and device share — options, report, word image — and the host implementation (plain C++, one thread, no limits):
// the directions through rank_audit_host's per-row callback, the moves judged by the chip's Program before / after and the interactions
// before / after as mutation_audit_host judges its own.  The device pass is Prover::step_audit (prover_audits.cpp, kernels/step_audit.hip).
#pragma once
#include "rank_audit.hpp"

namespace vhost {

constexpr uint32_t SA_MAX_STEPS = 4;
constexpr uint32_t SA_ROW_WORDS = 4 + 2 * RA_TERMS;  // row, pass mask, zero flag, n_support, terms

struct StepAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t chip_mask = 0;  // bit h: audit chip h; 0: all chips
    uint32_t n_steps = 0;    // 0: the default {1, p - 1, 2}
    uint32_t steps[SA_MAX_STEPS] = {0, 0, 0, 0};
    uint32_t reserved[3] = {0, 0, 0};
};

struct StepChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t max_degree = 0, line_exact = 0;
    uint64_t loose_cells = 0, zero_cells = 0, exact_cells = 0, coupled_exact_cells = 0;  // sums over rows and columns
    uint64_t confirmed_rows = 0, refuted_rows = 0;  // rows with a coupled-and-exact column / with a curved column
    uint64_t passes[SA_MAX_STEPS] = {0, 0, 0, 0};   // (row, loose column) cells whose step s goes undetected
    uint64_t bus_detected = 0;
    std::vector<uint64_t> loose, zeros, exact, coupled_exact;  // per column: rows
};
struct StepListedRow {
    uint32_t row = 0, pass_mask = 0, zero = 0, n_support = 0;
    uint32_t terms[2 * RA_TERMS] = {};
};
struct StepEntry {
    uint32_t chip = 0, column = 0;
    uint64_t coupled_exact = 0, curved = 0;
    std::vector<StepListedRow> rows;  // the first max_rows_per_entry rows where the column is loose and (not zero, or curved), ascending
};
struct StepReport {
    std::vector<uint32_t> steps;  // canonical
    bool truncated = false;
    uint64_t total_entries = 0;  // (chip, column) with a coupled-and-exact or a curved row, exact even when the list is cut
    std::vector<StepChipStat> chips;
    std::vector<StepEntry> entries;  // ascending (chip, column)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31525356u;  // "VSR1"
    // Flat image (include/vgpu.h documents it next to vgpu_step_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(RA_TERMS); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        w.push_back((uint32_t)steps.size()); w.push_back(0);
        for (uint32_t i = 0; i < SA_MAX_STEPS; i++) w.push_back(i < steps.size() ? steps[i] : 0u);
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height);
            w.push_back(c.max_degree); w.push_back(c.line_exact);
            u64(c.loose_cells); u64(c.zero_cells); u64(c.exact_cells); u64(c.coupled_exact_cells); u64(c.confirmed_rows); u64(c.refuted_rows);
            for (uint32_t i = 0; i < SA_MAX_STEPS; i++) u64(c.passes[i]);
            u64(c.bus_detected);
            for (uint32_t k = 0; k < c.width; k++) {
                u64(k < c.loose.size() ? c.loose[k] : 0); u64(k < c.zeros.size() ? c.zeros[k] : 0);
                u64(k < c.exact.size() ? c.exact[k] : 0); u64(k < c.coupled_exact.size() ? c.coupled_exact[k] : 0);
            }
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.column); w.push_back((uint32_t)e.rows.size()); w.push_back(0);
            u64(e.coupled_exact); u64(e.curved);
            for (auto& r : e.rows) {
                w.push_back(r.row); w.push_back(r.pass_mask); w.push_back(r.zero); w.push_back(r.n_support);
                for (uint32_t t = 0; t < 2 * RA_TERMS; t++) w.push_back(r.terms[t]);
            }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string sa_renamed(const std::invalid_argument& e) {
    const std::string m = e.what(), from = "rank_audit: ";
    return m.compare(0, from.size(), from) == 0 ? "step_audit: " + m.substr(from.size()) : m;
}

inline StepAuditOpts step_audit_checked_opts(const StepAuditOpts& in, size_t n_chips) {
    if (in.reserved[0] != 0 || in.reserved[1] != 0 || in.reserved[2] != 0) throw std::invalid_argument("step_audit: the reserved fields of the options must be zero");
    StepAuditOpts o = in;
    RankAuditOpts ro;
    ro.max_entries = in.max_entries; ro.max_rows_per_entry = in.max_rows_per_entry; ro.chip_mask = in.chip_mask;
    try {
        ro = rank_audit_checked_opts(ro, n_chips);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(sa_renamed(e));
    }
    o.max_entries = ro.max_entries; o.max_rows_per_entry = ro.max_rows_per_entry;
    if (o.n_steps == 0) { o.n_steps = 3; o.steps[0] = 1; o.steps[1] = vg::P - 1; o.steps[2] = 2; o.steps[3] = 0; }
    if (o.n_steps > SA_MAX_STEPS) throw std::invalid_argument("step_audit: at most " + std::to_string(SA_MAX_STEPS) + " steps (got " + std::to_string(o.n_steps) + ")");
    for (uint32_t i = 0; i < o.n_steps; i++) {
        if (o.steps[i] == 0 || o.steps[i] >= vg::P) throw std::invalid_argument("step_audit: a step must be a canonical value in 1..p-1 (step " + std::to_string(i) + ": " + std::to_string(o.steps[i]) + ")");
        for (uint32_t j = 0; j < i; j++)
            if (o.steps[j] == o.steps[i]) throw std::invalid_argument("step_audit: the steps must be distinct (" + std::to_string(o.steps[i]) + " is repeated)");
    }
    for (uint32_t i = o.n_steps; i < SA_MAX_STEPS; i++) o.steps[i] = 0;
    return o;
}
inline bool step_audit_selected(const StepAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void step_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                            std::vector<int>& prep_slot) {
    try {
        rank_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(sa_renamed(e));
    }
}

// The static part of a chip's block
inline void step_audit_chip_block(StepChipStat& cs, const AirDesc& air, uint64_t height, bool audited, uint32_t n_steps) {
    cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = height;
    cs.audited = audited ? 1u : 0u;
    cs.max_degree = (uint32_t)std::max(air.max_constraint_degree, 0);
    cs.line_exact = audited && n_steps >= cs.max_degree ? 1u : 0u;
    cs.loose.assign(air.width, 0); cs.zeros.assign(air.width, 0); cs.exact.assign(air.width, 0); cs.coupled_exact.assign(air.width, 0);
}

// The sums over a chip's columns, total_entries, truncated and the entries (without rows) from the per-column counts
inline void step_audit_finish(StepReport& r, const StepAuditOpts& o) {
    r.steps.assign(o.steps, o.steps + o.n_steps);
    r.total_entries = 0;
    r.entries.clear();
    for (size_t c = 0; c < r.chips.size(); c++) {
        StepChipStat& cs = r.chips[c];
        cs.loose_cells = cs.zero_cells = cs.exact_cells = cs.coupled_exact_cells = 0;
        if (!cs.audited) continue;
        for (uint32_t k = 0; k < cs.width; k++) {
            cs.loose_cells += cs.loose[k]; cs.zero_cells += cs.zeros[k]; cs.exact_cells += cs.exact[k]; cs.coupled_exact_cells += cs.coupled_exact[k];
            const uint64_t curved = cs.loose[k] - cs.exact[k];
            if (!cs.coupled_exact[k] && !curved) continue;
            r.total_entries++;
            if (r.entries.size() < o.max_entries) {
                StepEntry e;
                e.chip = (uint32_t)c; e.column = k; e.coupled_exact = cs.coupled_exact[k]; e.curved = curved;
                r.entries.push_back(std::move(e));
            }
        }
    }
    r.truncated = r.total_entries > r.entries.size();
}

inline StepReport step_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                  const std::vector<ConstraintHostMatrix>& prep, const StepAuditOpts& opts_in) {
    const StepAuditOpts o = step_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("step_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("step_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    step_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t S = o.n_steps, R = o.max_rows_per_entry, ALL = (1u << S) - 1u;
    StepReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<std::vector<StepListedRow>>> first(NC);
    for (size_t c = 0; c < NC; c++) {
        step_audit_chip_block(rep.chips[c], machine.airs[c], main[c].height, step_audit_selected(o, c), S);
        first[c].resize(machine.airs[c].width);
    }
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    vg::Fp tm[SA_MAX_STEPS];
    for (uint32_t i = 0; i < S; i++) tm[i] = vg::Fp::from_canonical(o.steps[i]);

    // the state of the chip the callback is in
    size_t cur_chip = (size_t)-1;
    std::vector<vg::Fp> mont, pmont, regs, moved, vec;
    std::vector<uint64_t> base;
    std::vector<uint32_t> mut, mask_of;
    const AirDesc* air = nullptr;
    const ConstraintHostMatrix* pm = nullptr;
    uint64_t n = 0;
    uint32_t K = 0, W = 0, PW = 0;
    size_t MW = 0;
    auto prow = [&](uint64_t q) -> const vg::Fp* { return pm ? pmont.data() + q * PW : nullptr; };
    // Air::eval at row q on the given local / next rows; base == nullptr: the fail mask to `out`, otherwise: some constraint is non-zero whose bit in `base` is clear
    auto eval = [&](uint64_t q, const vg::Fp* ml, const vg::Fp* mn, const vg::Fp* pl, const vg::Fp* pn, const uint64_t* b, uint64_t* out) -> bool {
        uint32_t k = 0;
        rep.evaluations += 1;
        for (const vair::Instr& in : air->program.instrs) {
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
                        if (!b) out[k >> 6] |= 1ull << (k & 63);
                        else if (!((b[k >> 6] >> (k & 63)) & 1ull)) return true;
                    }
                    k++;
                    break;
                default: break;
            }
        }
        return false;
    };
    auto vcol = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* pr) {
        uint64_t acc = v.constant % vg::P;
        for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? pr : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
        return (uint32_t)acc;
    };
    auto enter = [&](size_t c) {
        cur_chip = c;
        air = &machine.airs[c];
        K = air->program.num_asserts; W = air->width; PW = air->prep_width;
        n = main[c].height;
        pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        MW = (K + 63) / 64;
        regs.assign(air->program.num_regs ? air->program.num_regs : 1, zero);
        mont.resize((size_t)n * W); pmont.resize(pm ? (size_t)n * PW : 0);
        for (size_t i = 0; i < mont.size(); i++) mont[i] = vg::Fp::from_canonical(main[c].data[i]);
        for (size_t i = 0; i < pmont.size(); i++) pmont[i] = vg::Fp::from_canonical(pm->data[i]);
        base.assign(K ? (size_t)n * MW : 0, 0);
        if (K)
            for (uint64_t q = 0; q < n; q++) { const uint64_t nx = (q + 1) & (n - 1); eval(q, mont.data() + q * W, mont.data() + nx * W, prow(q), prow(nx), nullptr, base.data() + q * MW); }
        moved.assign(W, zero); vec.assign(W, zero); mut.assign(W, 0); mask_of.assign(W, 0);
    };
    auto per_row = [&](size_t c, uint64_t r, const RankBasis& B) {
        if (c != cur_chip) enter(c);
        StepChipStat& cs = rep.chips[c];
        const uint64_t rp = (r + n - 1) & (n - 1), nx = (r + 1) & (n - 1);
        const uint32_t* crow = main[c].data + r * W;
        const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
        constexpr uint32_t UNSET = 0xffffffffu;
        std::fill(mask_of.begin(), mask_of.end(), UNSET);  // per non-pivot column f: the pass mask of its basis vector, made once per row
        bool confirmed = false, refuted = false;
        for (uint32_t col = 0; col < W; col++) {
            if (B.pinned(col)) continue;
            uint32_t f = col;
            if (B.row_of[col] >= 0) {
                const vg::Fp* b = &B.rows[(size_t)B.row_of[col] * W];
                for (f = 0; f < W; f++) if (B.row_of[f] < 0 && !b[f].is_zero()) break;
            }
            if (mask_of[f] == UNSET) {
                for (uint32_t k = 0; k < W; k++) vec[k] = k == f ? one : (B.row_of[k] >= 0 ? -B.rows[(size_t)B.row_of[k] * W + f] : zero);
                uint32_t mask = 0;
                for (uint32_t s = 0; s < S; s++) {
                    for (uint32_t k = 0; k < W; k++) { moved[k] = mont[r * W + k] + tm[s] * vec[k]; mut[k] = moved[k].canonical(); }
                    bool a_det = false, b_det = false;
                    if (K) {
                        if (n == 1) a_det = eval(0, moved.data(), moved.data(), prow(0), prow(0), base.data(), nullptr);
                        else {
                            a_det = eval(r, moved.data(), mont.data() + nx * W, prow(r), prow(nx), base.data() + r * MW, nullptr);
                            if (!a_det) a_det = eval(rp, mont.data() + rp * W, moved.data(), prow(rp), prow(r), base.data() + rp * MW, nullptr);
                        }
                    }
                    for (auto& it : air->interactions) {
                        const uint32_t c0 = vcol(it.count, crow, cprow), c1 = vcol(it.count, mut.data(), cprow);
                        if (c0 != c1) { b_det = true; break; }
                        if (!c0) continue;
                        for (auto& fl : it.fields)
                            if (vcol(fl, crow, cprow) != vcol(fl, mut.data(), cprow)) { b_det = true; break; }
                        if (b_det) break;
                    }
                    if (!a_det && !b_det) mask |= 1u << s;
                    if (b_det) mask |= 0x100u << s;
                }
                mask_of[f] = mask;
            }
            const uint32_t mask = mask_of[f] & 0xffu, isz = B.nonzero[col] ? 0u : 1u;
            const bool exact = mask == ALL;
            cs.loose[col]++;
            if (isz) cs.zeros[col]++;
            if (exact) cs.exact[col]++;
            if (exact && !isz) { cs.coupled_exact[col]++; confirmed = true; }
            if (!exact) refuted = true;
            for (uint32_t s = 0; s < S; s++) { cs.passes[s] += (mask >> s) & 1u; cs.bus_detected += (mask_of[f] >> (8 + s)) & 1u; }
            if ((!isz || !exact) && first[c][col].size() < R) {
                const RankListedRow v = B.null_vector(col, (uint32_t)r);
                StepListedRow lr;
                lr.row = (uint32_t)r; lr.pass_mask = mask; lr.zero = isz; lr.n_support = v.n_support;
                std::copy(v.terms, v.terms + 2 * RA_TERMS, lr.terms);
                first[c][col].push_back(lr);
            }
        }
        if (confirmed) cs.confirmed_rows++;
        if (refuted) cs.refuted_rows++;
    };
    RankAuditOpts ro;
    ro.max_entries = 1; ro.max_rows_per_entry = 1; ro.chip_mask = o.chip_mask;
    try {
        const RankReport rr = rank_audit_host(machine, main, prep_chips, prep, ro, per_row);
        rep.evaluations += rr.evaluations;
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(sa_renamed(e));
    }
    step_audit_finish(rep, o);
    for (auto& e : rep.entries) e.rows = std::move(first[e.chip][e.column]);
    return rep;
}

}  // namespace vhost
