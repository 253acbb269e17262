// Field audit: which FIELDS of a chip's bus records its constraints leave undetermined.  The five row audits count a cell that feeds a record
// as bound, because a changed record detects.  That makes them blind to a chip that receives (opcode, a, b, c) and never ties c to a and b: the
// field audit asks the rank audit's Jacobian per record field instead of per cell.
//   rows           of the rank audit's Jacobian J_r of chip h at row r (host/rank_audit.hpp: the same domain, the same n = 1 rule, derivatives at
//                  the witness as it is): C, the constraint rows dC_k / dM[r][c] at q = r and q = (r - 1) mod n; psi_m, the main-column weights
//                  of the count of every interaction m, live or not; phi_{m,j}, the main-column weights of field j of interaction m, which
//                  exist only when m is LIVE at r (its count is non-zero on M).
//   per field      of a live interaction m: CONSTANT when phi_{m,j} = 0 (it reads only constants or preprocessed columns): never audited,
//                  never floats.  Otherwise S_{m,j} = C + {psi_*} + {phi_{m,i} : i != j}; the field is DETERMINED at r iff phi_{m,j} lies in
//                  the row space of S_{m,j}, otherwise it FLOATS: some direction v in the row's cells leaves every constraint, every count and
//                  every other field of that record unchanged to first order, and moves this field.
//   not held fixed the records of the chip's OTHER interactions.  The same cell often also goes to the range bus (the output bytes of add and
//                  sub) or to a sister record (cpu's channel values, shift's two records); holding that copy fixed would hide exactly the holes
//                  this audit is for.
//   witness        of a floating field: R = RREF(S_{m,j}), b_f the null-space basis vector of non-pivot column f (the rank audit's definition),
//                  f the smallest with phi_{m,j} . b_f != 0, v = b_f / (phi_{m,j} . b_f): S v = 0 and phi v = 1.  The RREF is unique, so no
//                  elimination order changes a word.
// It is first order, on this witness, with the other rows' cells held fixed: b (b - 1) = 0 pins b (add's carries count as bound), x^2 = 0 at
// x = 0 makes x look free, a field determined only for y != 0 (z = x y, field x) floats on the rows where y = 0.  A floating field on a SEND
// usually means "this chip delegates" (cpu's read values, shift's output): the finding is a field that also floats on the receiving chip.
// Inputs are not functions of outputs: lt's operands are expected to float.
// This header holds what host and device share — the report and its word image — and the host implementation (plain C++, one thread, no
// limits).  Options are the rank audit's.  The device pass is Prover::field_audit (prover_audits.cpp, kernels/field_audit.hip).
#pragma once
#include <functional>
#include "rank_audit.hpp"

namespace vhost {

struct FieldInteractionStat {
    uint32_t is_send = 0, is_global = 0, bus_index = 0, n_fields = 0;
    uint64_t live_rows = 0;
    std::vector<uint32_t> constant;   // per field: 1 when it has no main-column weight
    std::vector<uint64_t> floating;   // per field: rows where it floats
};
struct FieldChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0, live_records = 0, floating_fields = 0, floating_rows = 0;
    std::vector<FieldInteractionStat> interactions;
};
struct FieldEntry {
    uint32_t chip = 0, interaction = 0, field = 0;
    uint64_t floating = 0;
    std::vector<RankListedRow> rows;  // the first max_rows_per_entry floating rows, ascending, each with the witness direction
};
struct FieldReport {
    bool truncated = false;
    uint64_t total_entries = 0;  // (chip, interaction, field) with a floating row, exact even when the list is cut
    std::vector<FieldChipStat> chips;
    std::vector<FieldEntry> entries;  // ascending (chip, interaction, field)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31414656u;  // "VFA1"
    // Flat image (include/vgpu.h documents it next to vgpu_field_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(RA_TERMS); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height); u64(c.live_records); u64(c.floating_fields); u64(c.floating_rows);
            for (auto& it : c.interactions) {
                w.push_back(it.is_send); w.push_back(it.is_global); w.push_back(it.bus_index); w.push_back(it.n_fields);
                u64(it.live_rows);
                for (uint32_t j = 0; j < it.n_fields; j++) { w.push_back(it.constant[j]); u64(it.floating[j]); }
            }
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.interaction); w.push_back(e.field); w.push_back((uint32_t)e.rows.size());
            u64(e.floating);
            for (auto& r : e.rows) {
                w.push_back(r.row); w.push_back(r.n_support);
                for (uint32_t t = 0; t < 2 * RA_TERMS; t++) w.push_back(r.terms[t]);
            }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string field_audit_renamed(const std::string& m) {
    const std::string from = "rank_audit: ";
    return m.compare(0, from.size(), from) == 0 ? "field_audit: " + m.substr(from.size()) : m;
}
inline RankAuditOpts field_audit_checked_opts(const RankAuditOpts& in, size_t n_chips) {
    try {
        return rank_audit_checked_opts(in, n_chips);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(field_audit_renamed(e.what()));
    }
}
inline void field_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                             std::vector<int>& prep_slot) {
    try {
        rank_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(field_audit_renamed(e.what()));
    }
}

// The chip's block of the report before any row is looked at: shapes, bus names and the constant flags (from the weight rows: ra_weight_rows)
inline void field_audit_chip_block(FieldChipStat& cs, const AirDesc& air, uint64_t height, bool audited, const std::vector<uint32_t>& wr) {
    cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = height;
    cs.audited = audited ? 1u : 0u;
    cs.interactions.resize(air.interactions.size());
    for (size_t m = 0; m < air.interactions.size(); m++) {
        const auto& it = air.interactions[m];
        FieldInteractionStat& s = cs.interactions[m];
        s.is_send = it.is_send() ? 1u : 0u; s.is_global = it.is_local() ? 0u : 1u; s.bus_index = (uint32_t)it.bus_index; s.n_fields = (uint32_t)it.fields.size();
        s.constant.assign(s.n_fields, 0); s.floating.assign(s.n_fields, 0);
        const uint32_t at = wr[2 + m];
        for (uint32_t j = 0; j < s.n_fields; j++) {
            uint32_t any = 0;
            for (uint32_t k = 0; k < air.width; k++) any |= wr[at + 1 + (size_t)(1 + j) * air.width + k];
            s.constant[j] = any ? 0u : 1u;
        }
    }
}

// total_entries, truncated and the entries (without rows) from the per-field counts
inline void field_audit_finish(FieldReport& r, const RankAuditOpts& o) {
    r.total_entries = 0;
    r.entries.clear();
    for (size_t c = 0; c < r.chips.size(); c++) {
        const FieldChipStat& cs = r.chips[c];
        if (!cs.audited) continue;
        for (size_t m = 0; m < cs.interactions.size(); m++)
            for (uint32_t j = 0; j < cs.interactions[m].n_fields; j++) {
                const uint64_t fl = cs.interactions[m].floating[j];
                if (!fl) continue;
                r.total_entries++;
                if (r.entries.size() < o.max_entries) {
                    FieldEntry e;
                    e.chip = (uint32_t)c; e.interaction = (uint32_t)m; e.field = j; e.floating = fl;
                    r.entries.push_back(std::move(e));
                }
            }
    }
    r.truncated = r.total_entries > r.entries.size();
}

// x modulo the reduced basis B (x is left on B's non-pivot columns)
inline void field_audit_reduce(const RankBasis& B, std::vector<vg::Fp>& x) {
    for (uint32_t p = 0; p < B.w; p++) {
        if (B.row_of[p] < 0 || x[p].is_zero()) continue;
        const vg::Fp coef = x[p];
        const vg::Fp* b = &B.rows[(size_t)B.row_of[p] * B.w];
        for (uint32_t c = 0; c < B.w; c++) x[c] -= coef * b[c];
    }
}

// The contract on the host, literally: per row the base basis of C and the counts; per live record and field a copy of it with the other
// fields inserted, and the field reduced against it.  A chip without constraints depends on the row only through its live set: the row before's
// answer is kept while the live set repeats.  on_record, when given, is called once per audited live record in record order with the
// record's float mask (bit j: field j floats; fields from 32 on are not in it): what the link audit joins (host/link_audit.hpp).
using FieldRecordFn = std::function<void(uint32_t chip, uint64_t row, uint32_t interaction, uint32_t float_mask)>;
inline FieldReport field_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                    const std::vector<ConstraintHostMatrix>& prep, const RankAuditOpts& opts_in, const FieldRecordFn* on_record = nullptr) {
    const RankAuditOpts o = field_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("field_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("field_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    field_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    FieldReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<std::vector<std::vector<RankListedRow>>>> first(NC);
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        const vair::Program& p = air.program;
        const uint32_t K = p.num_asserts, W = air.width, PW = air.prep_width;
        const ConstraintHostMatrix& mm = main[c];
        const uint64_t n = mm.height;
        const std::vector<uint32_t> wr = ra_weight_rows(air);
        FieldChipStat& cs = rep.chips[c];
        field_audit_chip_block(cs, air, n, rank_audit_selected(o, c), wr);
        const size_t M = air.interactions.size();
        first[c].resize(M);
        for (size_t m = 0; m < M; m++) first[c][m].resize(cs.interactions[m].n_fields);
        if (!cs.audited || !W || !M) continue;  // no interaction, no record
        const ConstraintHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        std::vector<vg::Fp> mont((size_t)n * W), pmont(pm ? (size_t)n * PW : 0);
        for (size_t i = 0; i < mont.size(); i++) mont[i] = vg::Fp::from_canonical(mm.data[i]);
        for (size_t i = 0; i < pmont.size(); i++) pmont[i] = vg::Fp::from_canonical(pm->data[i]);
        auto prow = [&](uint64_t q) -> const vg::Fp* { return pm ? pmont.data() + q * PW : nullptr; };
        std::vector<vg::Fp> rv(p.num_regs ? p.num_regs : 1), rd(p.num_regs ? p.num_regs : 1);
        // one dual evaluation at row q: the derivative of every constraint by main column `col` in the seeded roles -> out[k * W + col]
        auto eval = [&](uint64_t q, uint32_t col, bool seed_local, bool seed_next, vg::Fp* out) {
            const uint64_t nx = (q + 1) & (n - 1);
            const vg::Fp *ml = mont.data() + q * W, *mn = mont.data() + nx * W, *pl = prow(q), *pn = prow(nx);
            uint32_t k = 0;
            rep.evaluations += 1;
            for (const vair::Instr& in : p.instrs) {
                switch (in.op) {
                    case vair::OP_CONST: rv[in.dst] = vg::Fp::raw((uint32_t)in.a | ((uint32_t)in.b << 16)); rd[in.dst] = zero; break;
                    case vair::OP_LOAD_MAIN: rv[in.dst] = (in.flag ? mn : ml)[in.a]; rd[in.dst] = (in.a == col && (in.flag ? seed_next : seed_local)) ? one : zero; break;
                    case vair::OP_LOAD_PREP: rv[in.dst] = (in.flag ? pn : pl)[in.a]; rd[in.dst] = zero; break;
                    case vair::OP_SEL_FIRST: rv[in.dst] = q == 0 ? one : zero; rd[in.dst] = zero; break;
                    case vair::OP_SEL_LAST: rv[in.dst] = q == n - 1 ? one : zero; rd[in.dst] = zero; break;
                    case vair::OP_SEL_TRANS: rv[in.dst] = q == n - 1 ? zero : one; rd[in.dst] = zero; break;
                    case vair::OP_ADD: { const vg::Fp v = rv[in.a] + rv[in.b], d = rd[in.a] + rd[in.b]; rv[in.dst] = v; rd[in.dst] = d; } break;
                    case vair::OP_SUB: { const vg::Fp v = rv[in.a] - rv[in.b], d = rd[in.a] - rd[in.b]; rv[in.dst] = v; rd[in.dst] = d; } break;
                    case vair::OP_MUL: { const vg::Fp v = rv[in.a] * rv[in.b], d = rv[in.a] * rd[in.b] + rd[in.a] * rv[in.b]; rv[in.dst] = v; rd[in.dst] = d; } break;
                    case vair::OP_NEG: { const vg::Fp v = -rv[in.a], d = -rd[in.a]; rv[in.dst] = v; rd[in.dst] = d; } break;
                    case vair::OP_ASSERT: out[(size_t)k * W + col] = rd[in.a]; k++; break;
                    default: break;
                }
            }
        };
        auto vcol = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* pr) {
            uint64_t acc = v.constant % vg::P;
            for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? pr : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
            return (uint32_t)acc;
        };
        auto wrow = [&](size_t m, uint32_t x, std::vector<vg::Fp>& out) {  // x = 0: the count, 1 + j: field j
            const uint32_t at = wr[2 + m];
            for (uint32_t k = 0; k < W; k++) out[k] = vg::Fp::raw(wr[at + 1 + (size_t)x * W + k]);
        };
        std::vector<vg::Fp> jl((size_t)K * W ? (size_t)K * W : 1), jn(jl.size()), x(W);
        RankBasis B, S;
        // the row's answer: per interaction its liveness, per field whether it floats and the direction (row filled in when listed)
        std::vector<uint8_t> live(M, 0), live_prev;
        std::vector<std::vector<uint8_t>> fl(M);
        std::vector<std::vector<RankListedRow>> dir(M);
        for (size_t m = 0; m < M; m++) { fl[m].assign(cs.interactions[m].n_fields, 0); dir[m].resize(cs.interactions[m].n_fields); }
        bool have_prev = false;
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t rp = (r + n - 1) & (n - 1);
            const uint32_t* crow = mm.data + r * W;
            const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
            for (size_t m = 0; m < M; m++) live[m] = vcol(air.interactions[m].count, crow, cprow) != 0 ? 1 : 0;
            const bool reuse = !K && have_prev && live == live_prev;
            live_prev = live; have_prev = true;
            if (!reuse) {
                B.reset(W);
                if (K) {
                    for (uint32_t col = 0; col < W; col++) {
                        eval(r, col, true, n == 1, jl.data());
                        if (n > 1) eval(rp, col, false, true, jn.data());
                    }
                    for (uint32_t k = 0; k < K; k++) { x.assign(jl.begin() + (size_t)k * W, jl.begin() + (size_t)(k + 1) * W); B.insert(x); }
                    if (n > 1)
                        for (uint32_t k = 0; k < K; k++) { x.assign(jn.begin() + (size_t)k * W, jn.begin() + (size_t)(k + 1) * W); B.insert(x); }
                }
                for (size_t m = 0; m < M; m++) { wrow(m, 0, x); B.insert(x); }
                for (size_t m = 0; m < M; m++) {
                    const uint32_t nf = cs.interactions[m].n_fields;
                    for (uint32_t j = 0; j < nf; j++) {
                        fl[m][j] = 0;
                        if (!live[m] || cs.interactions[m].constant[j]) continue;
                        S = B;
                        for (uint32_t i = 0; i < nf; i++) if (i != j) { wrow(m, 1 + i, x); S.insert(x); }
                        wrow(m, 1 + j, x);
                        field_audit_reduce(S, x);
                        uint32_t f = 0;
                        while (f < W && x[f].is_zero()) f++;
                        if (f == W) continue;  // determined
                        fl[m][j] = 1;
                        const vg::Fp inv = x[f].inv();
                        RankListedRow out;
                        for (uint32_t k = 0; k < W; k++) {
                            vg::Fp v = zero;
                            if (k == f) v = inv;
                            else if (S.row_of[k] >= 0) v = -S.rows[(size_t)S.row_of[k] * W + f] * inv;
                            if (v.is_zero()) continue;
                            if (out.n_support < RA_TERMS) { out.terms[2 * out.n_support] = k; out.terms[2 * out.n_support + 1] = v.canonical(); }
                            out.n_support++;
                        }
                        dir[m][j] = out;
                    }
                }
            }
            bool any = false;
            for (size_t m = 0; m < M; m++) {
                if (!live[m]) continue;
                FieldInteractionStat& s = cs.interactions[m];
                s.live_rows++; cs.live_records++;
                if (on_record) {
                    uint32_t mask = 0;
                    for (uint32_t j = 0; j < s.n_fields && j < 32u; j++) mask |= fl[m][j] ? 1u << j : 0u;
                    (*on_record)((uint32_t)c, r, (uint32_t)m, mask);
                }
                for (uint32_t j = 0; j < s.n_fields; j++) {
                    if (!fl[m][j]) continue;
                    any = true;
                    s.floating[j]++; cs.floating_fields++;
                    if (first[c][m][j].size() < R) { first[c][m][j].push_back(dir[m][j]); first[c][m][j].back().row = (uint32_t)r; }
                }
            }
            if (any) cs.floating_rows++;
        }
    }
    field_audit_finish(rep, o);
    for (auto& e : rep.entries) e.rows = std::move(first[e.chip][e.interaction][e.field]);
    return rep;
}

}  // namespace vhost
