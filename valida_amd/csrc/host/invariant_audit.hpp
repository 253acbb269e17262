// Invariant audit: the converse of the other audits.  They ask what the constraints and bus records bind; this one asks which affine-linear
// relations among a chip's main columns the WITNESS keeps on every row, and then on how many rows the chip's own constraints and records
// enforce each of them to first order.
//   invariants     chip h, main matrix M (n x w, canonical): the augmented row a_r = (1, M[r][0], .., M[r][w - 1]); I_h = { l in F_p^(w + 1) :
//                  l . a_r = 0 for every r }.  R = the reduced row echelon form of the n x (w + 1) matrix of the a_r, columns in that order
//                  (the constant first): unique, so no elimination order, grid or row order changes a word.  Column 0 is always a pivot.
//                  rho_A = rank, d = w + 1 - rho_A.
//   basis          one invariant per non-pivot main column f: l_f = 1, l_p = -R[row of p][f] for every pivot column p (only pivots left of f
//                  occur), 0 elsewhere: "column f is this affine function of earlier columns".  CONSTANT when no main column other than f has
//                  a non-zero coefficient (M[r][f] = -l_0 on every row), otherwise a RELATION.
//   enforcement    c = (l_1 .. l_w) against the rank audit's Jacobian J_r (host/rank_audit.hpp, the same matrix word for word; n = 1 by its
//                  rule): l is ENFORCED at r iff c lies in the row space of J_r (c . v = 0 for every v with J_r v = 0), otherwise FREE at r:
//                  some first-order-unnoticed move of the row's cells breaks the relation.  Each invariant is judged against J_r alone.
// What it is not: affine-linear only (b (b - 1) = 0 is not found); one row (no relation between a row and its successor); THIS witness (a
// short program has accidental relations); the verdict is per basis vector (a sum of two free invariants can be enforced); first order, with
// the rank audit's caveats.  `check`'s exit status never depends on it.
// This header holds what the host and the device implementation share — options, the report and its word image, the entries from the basis —
// and the host implementation (plain C++, one thread, no limits).  The device pass is Prover::invariant_audit (prover_audits.cpp,
// kernels/invariant_audit.hip).
#pragma once
#include "rank_audit.hpp"

namespace vhost {

struct InvariantAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t chip_mask = 0;  // bit h: audit chip h; 0: all chips
    uint32_t max_terms = 8;  // (column, coefficient) terms listed per invariant
    uint32_t reserved[3] = {0, 0, 0};
};

struct InvariantChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t rank = 0, dim = 0, constants = 0, relations = 0;  // rho_A, d, and d split by kind
    uint32_t every = 0, some = 0, never = 0;                   // invariants enforced on every row, on some rows, on no row
};
struct InvariantEntry {
    uint32_t chip = 0, column = 0, kind = 0;  // kind 0: constant, 1: relation
    uint32_t l0 = 0, n_support = 0;           // canonical constant term; main columns with a non-zero coefficient, f included
    std::vector<uint32_t> terms;              // the first max_terms (column, coefficient), ascending column
    uint64_t enforced = 0, free_rows = 0;
    std::vector<uint32_t> rows;               // the first max_rows_per_entry free rows, ascending
};
struct InvariantReport {
    bool truncated = false;
    uint32_t max_terms = 8;
    uint64_t total_entries = 0;  // the sum of d over the audited chips, exact even when the list is cut
    std::vector<InvariantChipStat> chips;
    std::vector<InvariantEntry> entries;  // ascending (chip, column)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31524956u;  // "VIR1"
    // Flat image (include/vgpu.h documents it next to vgpu_invariant_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(max_terms); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height);
            w.push_back(c.rank); w.push_back(c.dim); w.push_back(c.constants); w.push_back(c.relations);
            w.push_back(c.every); w.push_back(c.some); w.push_back(c.never); w.push_back(0);
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.column); w.push_back(e.kind); w.push_back(e.l0);
            w.push_back(e.n_support); w.push_back((uint32_t)(e.terms.size() / 2)); w.push_back((uint32_t)e.rows.size()); w.push_back(0);
            u64(e.enforced); u64(e.free_rows);
            w.insert(w.end(), e.terms.begin(), e.terms.end());
            w.insert(w.end(), e.rows.begin(), e.rows.end());
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string ia_renamed(const std::invalid_argument& e) {
    const std::string m = e.what(), from = "rank_audit: ";
    return m.compare(0, from.size(), from) == 0 ? "invariant_audit: " + m.substr(from.size()) : m;
}

inline InvariantAuditOpts invariant_audit_checked_opts(const InvariantAuditOpts& in, size_t n_chips) {
    if (in.reserved[0] != 0 || in.reserved[1] != 0 || in.reserved[2] != 0) throw std::invalid_argument("invariant_audit: the reserved fields of the options must be zero");
    InvariantAuditOpts o = in;
    RankAuditOpts ro;
    ro.max_entries = in.max_entries; ro.max_rows_per_entry = in.max_rows_per_entry; ro.chip_mask = in.chip_mask;
    try {
        ro = rank_audit_checked_opts(ro, n_chips);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(ia_renamed(e));
    }
    o.max_entries = ro.max_entries; o.max_rows_per_entry = ro.max_rows_per_entry;
    if (o.max_terms == 0) o.max_terms = 8;
    if (o.max_terms > 4096) throw std::invalid_argument("invariant_audit: max_terms is at most 4096");
    return o;
}
inline bool invariant_audit_selected(const InvariantAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void invariant_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                 std::vector<int>& prep_slot) {
    try {
        rank_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(ia_renamed(e));
    }
}

// The static part of a chip's block
inline void invariant_audit_chip_block(InvariantChipStat& cs, const AirDesc& air, uint64_t height, bool audited) {
    cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = height;
    cs.audited = audited ? 1u : 0u;
}

// One chip's invariants from the reduced basis of its augmented rows: pivot[c] (c = 0 .. w: c is a pivot column) and vec (d rows of w + 1
// Montgomery words, row i the canonical vector of the i-th non-pivot column) -> rank, dim, constants, relations of the chip's block and one entry
// per non-pivot column (counts and rows are filled in later); all of them, the caller cuts the list.
inline void invariant_audit_entries(InvariantChipStat& cs, uint32_t chip, const std::vector<uint8_t>& pivot, const std::vector<vg::Fp>& vec, uint32_t max_terms,
                                    std::vector<InvariantEntry>& out) {
    const uint32_t AW = cs.width + 1;
    cs.rank = 0;
    for (uint32_t c = 0; c < AW; c++) cs.rank += pivot[c] ? 1u : 0u;
    cs.dim = AW - cs.rank; cs.constants = cs.relations = 0;
    uint32_t i = 0;
    for (uint32_t f = 1; f < AW; f++) {
        if (pivot[f]) continue;
        const vg::Fp* l = vec.data() + (size_t)i++ * AW;
        InvariantEntry e;
        e.chip = chip; e.column = f - 1; e.l0 = l[0].canonical();
        for (uint32_t c = 1; c < AW; c++) {
            if (l[c].is_zero()) continue;
            if (e.n_support < max_terms) { e.terms.push_back(c - 1); e.terms.push_back(l[c].canonical()); }
            e.n_support++;
        }
        e.kind = e.n_support > 1 ? 1u : 0u;
        if (e.kind) cs.relations++; else cs.constants++;
        out.push_back(std::move(e));
    }
}

// every / some / never of the chips' blocks from the entries' counts (all entries of every audited chip), then the cut at max_entries
inline void invariant_audit_finish(InvariantReport& r, const InvariantAuditOpts& o) {
    r.max_terms = o.max_terms;
    for (auto& cs : r.chips) cs.every = cs.some = cs.never = 0;
    for (auto& e : r.entries) {
        InvariantChipStat& cs = r.chips[e.chip];
        if (!e.free_rows) cs.every++; else if (!e.enforced) cs.never++; else cs.some++;
    }
    r.total_entries = r.entries.size();
    if (r.entries.size() > o.max_entries) r.entries.resize((size_t)o.max_entries);
    r.truncated = r.total_entries > r.entries.size();
}

// The contract on the host: RREF of the augmented rows by insertion (RankBasis of width w + 1), then the rank audit's host Jacobian and RREF
// per row (rank_audit_host's per_row), each c reduced against it; one thread.
inline InvariantReport invariant_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                            const std::vector<ConstraintHostMatrix>& prep, const InvariantAuditOpts& opts_in) {
    const InvariantAuditOpts o = invariant_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("invariant_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("invariant_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    invariant_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    InvariantReport rep;
    rep.chips.resize(NC);
    std::vector<size_t> e_at(NC + 1, 0);            // chip c's entries are [e_at[c], e_at[c + 1])
    std::vector<std::vector<vg::Fp>> cvec(NC);      // per chip d rows of w Montgomery words: c = (l_1 .. l_w)
    uint32_t need_mask = 0;
    bool need = false;
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        InvariantChipStat& cs = rep.chips[c];
        invariant_audit_chip_block(cs, air, main[c].height, invariant_audit_selected(o, c));
        e_at[c] = rep.entries.size();
        if (!cs.audited || !air.width) continue;
        const uint32_t W = air.width, AW = W + 1;
        RankBasis B;
        B.reset(AW);
        std::vector<vg::Fp> x(AW);
        for (uint64_t r = 0; r < main[c].height && B.rho < AW; r++) {
            x[0] = vg::Fp::one();
            for (uint32_t k = 0; k < W; k++) x[1 + k] = vg::Fp::from_canonical(main[c].data[r * W + k]);
            B.insert(x);
        }
        std::vector<uint8_t> pivot(AW);
        std::vector<vg::Fp> vec;
        for (uint32_t f = 0; f < AW; f++) pivot[f] = B.row_of[f] >= 0;
        for (uint32_t f = 0; f < AW; f++) {
            if (pivot[f]) continue;
            for (uint32_t k = 0; k < AW; k++) {
                vec.push_back(k == f ? vg::Fp::one() : (pivot[k] ? -B.rows[(size_t)B.row_of[k] * AW + f] : vg::Fp::zero()));
                if (k) cvec[c].push_back(vec.back());
            }
        }
        invariant_audit_entries(cs, (uint32_t)c, pivot, vec, o.max_terms, rep.entries);
        if (cs.dim) { need = true; if (c < 32) need_mask |= 1u << c; }
    }
    e_at[NC] = rep.entries.size();
    if (need) {
        std::vector<vg::Fp> x;
        auto per_row = [&](size_t c, uint64_t r, const RankBasis& B) {
            const uint32_t W = B.w, d = rep.chips[c].dim;
            for (uint32_t i = 0; i < d; i++) {
                InvariantEntry& e = rep.entries[e_at[c] + i];
                const vg::Fp* cv = cvec[c].data() + (size_t)i * W;
                x.assign(cv, cv + W);
                // the basis is reduced: the coefficients can all be read before any update
                for (uint32_t p = 0; p < W; p++) {
                    if (B.row_of[p] < 0 || cv[p].is_zero()) continue;
                    const vg::Fp* b = &B.rows[(size_t)B.row_of[p] * W];
                    for (uint32_t k = 0; k < W; k++) x[k] -= cv[p] * b[k];
                }
                bool left = false;
                for (uint32_t k = 0; k < W; k++) left |= !x[k].is_zero();
                if (!left) { e.enforced++; continue; }
                e.free_rows++;
                if (e.rows.size() < R) e.rows.push_back((uint32_t)r);
            }
        };
        RankAuditOpts ro;
        ro.max_entries = 1; ro.max_rows_per_entry = 1;
        ro.chip_mask = NC <= 32 ? need_mask : 0;  // chips without an invariant have nothing to judge
        try {
            const RankReport rr = rank_audit_host(machine, main, prep_chips, prep, ro, per_row);
            rep.evaluations = rr.evaluations;
        } catch (const std::invalid_argument& e) {
            throw std::invalid_argument(ia_renamed(e));
        }
    }
    invariant_audit_finish(rep, o);
    return rep;
}

}  // namespace vhost
