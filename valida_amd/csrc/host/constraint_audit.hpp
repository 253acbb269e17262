// Constraint audit: WHICH AIR constraints of a witness fail, on which rows, with which value — the exact form of check_constraints
// (machine/src/check_constraints.rs:14-84, called per chip from basic/src/lib.rs:270-277) over a full witness; the other half of the debug
// self-check next to the bus audit (host/bus_audit.hpp).  The domain is the trace itself: row r of a chip of height n has next = (r + 1) mod n,
// is_first_row = [r == 0], is_last_row = [r == n - 1], is_transition = [r != n - 1] as 0/1 field values; constraint k of a chip is the k-th
// assert_zero of its Air::eval in call order (Dag::constraints / OP_ASSERT of air/symbolic.hpp); it fails on a row when its value there is
// non-zero.  Only Air::eval is audited (the permutation constraints depend on sampled challenges; their exact statement is the bus audit).
// This header holds what the host and the device implementation share — options, shape validation, the report and its flat word image — and the
// host implementation over canonical row-major matrices (plain C++, one thread, no device).  The device pass is Prover::constraint_audit
// (prover_audits.cpp, kernels/constraint_audit.hip).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "machine.hpp"

namespace vhost {

struct ConstraintAuditOpts {
    uint64_t max_constraints = 64;
    uint32_t max_rows_per_constraint = 4;
    uint32_t reserved = 0;
};

struct ConstraintChipStat { uint32_t n_constraints = 0, failing_constraints = 0; uint64_t height = 0, failing_rows = 0; };
struct ConstraintEntry {
    uint32_t chip = 0, constraint = 0;
    uint64_t failing_rows = 0;
    std::vector<std::pair<uint32_t, uint32_t>> rows;  // the first max_rows_per_constraint failing rows, ascending: (row, canonical value)
};
struct ConstraintReport {
    bool satisfied = true, truncated = false;
    uint64_t total_failing = 0;             // failing (chip, constraint) pairs, exact even when the list is cut
    std::vector<ConstraintChipStat> chips;  // one per chip of the machine
    std::vector<ConstraintEntry> constraints;  // ascending (chip, constraint)
    double device_ms = 0;                   // the device pass (0 for the host implementation); not part of the word image
    double host_ms = 0;                     // wall time of the whole call
    static constexpr uint32_t MAGIC = 0x31524356u;  // "VCR1"
    // Flat image (include/vgpu.h documents it next to vgpu_constraint_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(satisfied ? 1u : 0u); w.push_back(truncated ? 1u : 0u);
        u64(total_failing);
        w.push_back((uint32_t)constraints.size()); w.push_back((uint32_t)chips.size());
        for (auto& c : chips) { w.push_back(c.n_constraints); w.push_back(c.failing_constraints); u64(c.height); u64(c.failing_rows); }
        for (auto& e : constraints) {
            w.push_back(e.chip); w.push_back(e.constraint); u64(e.failing_rows); w.push_back((uint32_t)e.rows.size());
            for (auto& r : e.rows) { w.push_back(r.first); w.push_back(r.second); }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline ConstraintAuditOpts constraint_audit_checked_opts(const ConstraintAuditOpts& in) {
    ConstraintAuditOpts o = in;
    if (o.reserved != 0) throw std::invalid_argument("constraint_audit: the reserved field of the options must be zero");
    if (o.max_constraints == 0) o.max_constraints = 64;
    if (o.max_rows_per_constraint == 0) o.max_rows_per_constraint = 4;
    if (o.max_constraints > (1ull << 24) || o.max_rows_per_constraint > 4096) throw std::invalid_argument("constraint_audit: max_constraints is at most 2^24 and max_rows_per_constraint at most 4096");
    return o;
}

struct ConstraintShape { uint64_t height, width; };

// Validates the shapes exactly as prove and the bus audit do (one main trace per chip, widths, power-of-two heights, preprocessed traces for
// exactly the chips that have preprocessed columns) and that every column a constraint program loads lies inside its trace.
// prep_slot[chip] = index into the preprocessed list or -1.
inline void constraint_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                  std::vector<int>& prep_slot) {
    const size_t NC = machine.airs.size();
    if (main.size() != NC) throw std::invalid_argument("constraint_audit: need one main trace per chip (" + std::to_string(NC) + "), got " + std::to_string(main.size()));
    prep_slot.assign(NC, -1);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& a = machine.airs[i];
        if (main[i].width != a.width) throw std::invalid_argument("constraint_audit: trace width mismatch for chip " + a.name + " (" + std::to_string(main[i].width) + ", expected " + std::to_string(a.width) + ")");
        const uint64_t h = main[i].height;
        if (h == 0 || (h & (h - 1)) || h > (1ull << 27)) throw std::invalid_argument("constraint_audit: trace heights must be powers of two up to 2^27 (chip " + a.name + ": " + std::to_string(h) + ")");
    }
    for (size_t k = 0; k < prep_chips.size(); k++) {
        const int chip = prep_chips[k];
        if (chip < 0 || (size_t)chip >= NC || prep_slot[chip] >= 0) throw std::invalid_argument("constraint_audit: bad or repeated preprocessed chip index");
        if (machine.airs[chip].prep_width == 0) throw std::invalid_argument("constraint_audit: chip " + machine.airs[chip].name + " has no preprocessed columns");
        if (prep[k].width != machine.airs[chip].prep_width || prep[k].height != main[chip].height) throw std::invalid_argument("constraint_audit: preprocessed trace shape mismatch for chip " + machine.airs[chip].name);
        prep_slot[chip] = (int)k;
    }
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& a = machine.airs[i];
        if (a.prep_width && prep_slot[i] < 0) throw std::invalid_argument("constraint_audit: chip " + a.name + " needs its preprocessed trace");
        for (const vair::Instr& in : a.program.instrs) {
            if ((in.op == vair::OP_LOAD_MAIN && in.a >= a.width) || (in.op == vair::OP_LOAD_PREP && in.a >= a.prep_width)) throw std::invalid_argument("constraint_audit: a constraint of chip " + a.name + " reads a column outside its trace");
            if (in.op != vair::OP_ASSERT && in.op != vair::OP_NOP && in.dst >= a.program.num_regs) throw std::invalid_argument("constraint_audit: the constraint program of chip " + a.name + " is malformed");
        }
    }
}

// chips[].failing_constraints, total_failing, satisfied, truncated from the per-chip per-constraint counts; the entries (without rows) of the
// first max_constraints failing pairs in ascending (chip, constraint) order
inline void constraint_audit_finish(ConstraintReport& r, const std::vector<std::vector<uint64_t>>& counts, const ConstraintAuditOpts& o) {
    r.total_failing = 0;
    r.constraints.clear();
    for (size_t c = 0; c < counts.size(); c++) {
        r.chips[c].failing_constraints = 0;
        for (size_t k = 0; k < counts[c].size(); k++) {
            if (!counts[c][k]) continue;
            r.chips[c].failing_constraints++;
            r.total_failing++;
            if (r.constraints.size() < o.max_constraints) { ConstraintEntry e; e.chip = (uint32_t)c; e.constraint = (uint32_t)k; e.failing_rows = counts[c][k]; r.constraints.push_back(std::move(e)); }
        }
    }
    r.satisfied = r.total_failing == 0;
    r.truncated = r.total_failing > r.constraints.size();
}

struct ConstraintHostMatrix { const uint32_t* data; uint64_t height, width; };  // canonical row-major (the reference's RowMajorMatrix<Val>)

// The contract on the host: the chip's Program (what vair::HostEval runs) interpreted on every row; one thread.
inline ConstraintReport constraint_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                              const std::vector<ConstraintHostMatrix>& prep, const ConstraintAuditOpts& opts_in) {
    const ConstraintAuditOpts o = constraint_audit_checked_opts(opts_in);
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("constraint_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("constraint_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    constraint_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    ConstraintReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<uint64_t>> counts(NC);
    std::vector<std::vector<std::vector<std::pair<uint32_t, uint32_t>>>> first(NC);
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    for (size_t c = 0; c < NC; c++) {
        const vair::Program& p = machine.airs[c].program;
        const uint32_t K = p.num_asserts;
        const ConstraintHostMatrix& mm = main[c];
        rep.chips[c].n_constraints = K; rep.chips[c].height = mm.height;
        counts[c].assign(K, 0);
        first[c].resize(K);
        if (!K) continue;
        const ConstraintHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        std::vector<vg::Fp> regs(p.num_regs ? p.num_regs : 1);
        const uint64_t n = mm.height;
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t nx = (r + 1) & (n - 1);
            const uint32_t *ml = mm.data + r * mm.width, *mn = mm.data + nx * mm.width;
            const uint32_t *pl = pm ? pm->data + r * pm->width : nullptr, *pn = pm ? pm->data + nx * pm->width : nullptr;
            uint32_t k = 0;
            bool any = false;
            for (const vair::Instr& in : p.instrs) {
                switch (in.op) {
                    case vair::OP_CONST: regs[in.dst] = vg::Fp::raw((uint32_t)in.a | ((uint32_t)in.b << 16)); break;
                    case vair::OP_LOAD_MAIN: regs[in.dst] = vg::Fp::from_canonical((in.flag ? mn : ml)[in.a]); break;
                    case vair::OP_LOAD_PREP: regs[in.dst] = vg::Fp::from_canonical((in.flag ? pn : pl)[in.a]); break;
                    case vair::OP_SEL_FIRST: regs[in.dst] = r == 0 ? one : zero; break;
                    case vair::OP_SEL_LAST: regs[in.dst] = r == n - 1 ? one : zero; break;
                    case vair::OP_SEL_TRANS: regs[in.dst] = r == n - 1 ? zero : one; break;
                    case vair::OP_ADD: regs[in.dst] = regs[in.a] + regs[in.b]; break;
                    case vair::OP_SUB: regs[in.dst] = regs[in.a] - regs[in.b]; break;
                    case vair::OP_MUL: regs[in.dst] = regs[in.a] * regs[in.b]; break;
                    case vair::OP_NEG: regs[in.dst] = -regs[in.a]; break;
                    case vair::OP_ASSERT: {
                        const uint32_t v = regs[in.a].canonical();
                        if (v) {
                            any = true;
                            if (counts[c][k]++ < o.max_rows_per_constraint) first[c][k].push_back({(uint32_t)r, v});
                        }
                        k++;
                        break;
                    }
                    default: break;
                }
            }
            if (any) rep.chips[c].failing_rows++;
        }
    }
    constraint_audit_finish(rep, counts, o);
    for (auto& e : rep.constraints) e.rows = std::move(first[e.chip][e.constraint]);
    return rep;
}

}  // namespace vhost
