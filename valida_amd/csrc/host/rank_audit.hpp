// Rank audit: every first-order degree of freedom of one trace row — the general form of what the mutation audit (single cells) and the pair
// audit (two cells, given deltas) look for.  At row r of chip h, which directions v in the space F_p^w of the row's w main cells leave every
// constraint and every bus record unchanged to first order?  That is the null space of the Jacobian J_r of everything that reads the row.
//   Jacobian       w columns, one per main cell M[r][c] (preprocessed columns are never varied).  Rows: for every constraint k the partial
//                  derivatives dC_k / dM[r][c] of Air::eval at evaluation q = r (the cell read as `local`) and the same at q = (r - 1) mod n (the
//                  cell read as `next`), on the constraint audit's domain (next = (q + 1) mod n, is_first_row = [q = 0], is_last_row =
//                  [q = n - 1], is_transition = [q != n - 1]); for n = 1 one evaluation, the cell local and next at once, the derivative the
//                  sum over both roles.  Derivatives are taken at the witness as it is.  Permutation constraints are not evaluated: for every
//                  interaction m (Chip::all_interactions order) one row holds the main-column weights of its count and, when the count is
//                  non-zero at row r, one further row per field holds that field's main-column weights — v is orthogonal to those rows iff
//                  the record of m is unchanged along M[r] + t v for every t (exact, the virtual columns are affine).
//   per row        from the reduced row echelon form R of J_r (unique: no elimination order changes a word): rank rho, nullity nu = w - rho,
//                  z = zero columns of J_r; the row is COUPLED when nu > z.  Column c is PINNED iff e_c is in the row space (c is a pivot
//                  column whose row of R has no other non-zero entry), otherwise LOOSE; ZERO when column c of J_r is zero (a zero column is
//                  loose); COUPLED at r when loose and not zero: bound alone, slack together — the finding.
//   null vector    of a loose column c: if c is a non-pivot column the basis vector of c (v_c = 1, v_p = -R[row of p][c] for every pivot
//                  column p, 0 on the other non-pivot columns); if c is a pivot column with row i, the basis vector of the smallest non-pivot
//                  column f with R[i][f] != 0.
// It is first order: for a constraint of degree >= 2 in the row's cells a tangent-free direction is necessary for a CURVE of unnoticed changes
// and says nothing about a finite jump (b (b - 1) = 0 pins b although b -> 1 - b passes; x^2 = 0 at x = 0 reports x zero / loose although it is
// bound): finite flips stay with the mutation and pair audits.  It covers the cells of one row; cross-row combinations are not looked for.  It
// is a statement about THIS witness, not a soundness proof.
// This header holds what the host and the device implementation share — options, the report and its word image, the row analysis — and the
// host implementation (plain C++, one thread, no limits).  The device pass is Prover::rank_audit (prover_audits.cpp, kernels/rank_audit.hip).
#pragma once
#include <chrono>
#include <functional>
#include "mutation_audit.hpp"

namespace vhost {

constexpr uint32_t RA_TERMS = 8;                      // (column, coefficient) terms of a listed null vector
constexpr uint32_t RA_ROW_WORDS = 2 + 2 * RA_TERMS;   // row, n_support, terms

struct RankAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t chip_mask = 0;  // bit h: audit chip h; 0: all chips
    uint32_t reserved[2] = {0, 0};
};

struct RankChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0, nullity = 0, zero = 0, coupled_rows = 0;  // sums over the rows; rows with nu > z
    uint32_t max_nullity = 0, loose_cols = 0, pinned_cols = 0, coupled_cols = 0;
    std::vector<uint64_t> loose, zeros;  // per column: rows where it is loose / zero (coupled = loose - zero)
};
struct RankListedRow {
    uint32_t row = 0, n_support = 0;
    uint32_t terms[2 * RA_TERMS] = {};  // (column, canonical coefficient), ascending column, unused slots 0
};
struct RankEntry {
    uint32_t chip = 0, column = 0;
    uint64_t coupled = 0;
    std::vector<RankListedRow> rows;  // the first max_rows_per_entry coupled rows, ascending
};
struct RankReport {
    bool truncated = false;
    uint64_t total_entries = 0;  // (chip, column) with a coupled row, exact even when the list is cut
    std::vector<RankChipStat> chips;
    std::vector<RankEntry> entries;  // ascending (chip, column)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31525256u;  // "VRR1"
    // Flat image (include/vgpu.h documents it next to vgpu_rank_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(RA_TERMS); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height); u64(c.nullity); u64(c.zero); u64(c.coupled_rows);
            w.push_back(c.max_nullity); w.push_back(c.loose_cols); w.push_back(c.pinned_cols); w.push_back(c.coupled_cols);
            for (uint32_t k = 0; k < c.width; k++) { u64(k < c.loose.size() ? c.loose[k] : 0); u64(k < c.zeros.size() ? c.zeros[k] : 0); }
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.column); w.push_back((uint32_t)e.rows.size()); w.push_back(0);
            u64(e.coupled);
            for (auto& r : e.rows) {
                w.push_back(r.row); w.push_back(r.n_support);
                for (uint32_t t = 0; t < 2 * RA_TERMS; t++) w.push_back(r.terms[t]);
            }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline RankAuditOpts rank_audit_checked_opts(const RankAuditOpts& in, size_t n_chips) {
    if (in.reserved[0] != 0 || in.reserved[1] != 0) throw std::invalid_argument("rank_audit: the reserved fields of the options must be zero");
    RankAuditOpts o = in;
    if (o.max_entries == 0) o.max_entries = 1024;
    if (o.max_rows_per_entry == 0) o.max_rows_per_entry = 4;
    if (o.max_entries > (1ull << 24)) throw std::invalid_argument("rank_audit: max_entries is at most 2^24");
    if (o.max_rows_per_entry > 4096) throw std::invalid_argument("rank_audit: max_rows_per_entry is at most 4096");
    if (n_chips < 32 && (o.chip_mask >> n_chips) != 0) throw std::invalid_argument("rank_audit: chip_mask names a chip the machine does not have (" + std::to_string(n_chips) + " chips)");
    if (n_chips > 32 && o.chip_mask != 0) throw std::invalid_argument("rank_audit: chip_mask selects among at most 32 chips");
    return o;
}
inline bool rank_audit_selected(const RankAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void rank_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                            std::vector<int>& prep_slot) {
    try {
        mutation_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what(), from = "mutation_audit: ";
        throw std::invalid_argument(m.compare(0, from.size(), from) == 0 ? "rank_audit: " + m.substr(from.size()) : m);
    }
}

// The interaction rows of the Jacobian as the device pass reads them (u32 words): [0] M, then per interaction m [2 + m] its offset; at the
// offset: n_fields, then 1 + n_fields weight rows of `width` Montgomery words each (the count first): the sum of the main-column weights per
// column.  The liveness of an interaction (count != 0 on the row) comes from the interaction words of the permutation kernels.
inline std::vector<uint32_t> ra_weight_rows(const AirDesc& a) {
    std::vector<uint32_t> w;
    const uint32_t M = (uint32_t)a.interactions.size();
    w.push_back(M); w.push_back(a.width);
    w.resize(2 + M);
    auto row = [&](const vair::VirtualCol& v) {
        const size_t at = w.size();
        w.resize(at + a.width, 0);
        for (auto& t : v.terms)
            if (!t.preprocessed && t.col >= 0 && (uint32_t)t.col < a.width) w[at + t.col] = (vg::Fp::raw(w[at + t.col]) + vg::Fp::from_canonical(t.weight % vg::P)).v;
    };
    for (uint32_t m = 0; m < M; m++) {
        w[2 + m] = (uint32_t)w.size();
        w.push_back((uint32_t)a.interactions[m].fields.size());
        row(a.interactions[m].count);
        for (auto& f : a.interactions[m].fields) row(f);
    }
    return w;
}

// Row insertion into a reduced row echelon basis over F_p: the elimination both passes perform (the device one lane per column).
struct RankBasis {
    uint32_t w = 0, rho = 0;
    std::vector<vg::Fp> rows;       // [rho][w], reduced: a pivot column holds 1 in its row and 0 elsewhere
    std::vector<int32_t> row_of;    // [w] the row whose pivot the column is, or -1
    std::vector<uint8_t> nonzero;   // [w] some inserted row had a non-zero entry here
    void reset(uint32_t width) { w = width; rho = 0; rows.assign((size_t)w * w, vg::Fp::zero()); row_of.assign(w, -1); nonzero.assign(w, 0); }
    void insert(std::vector<vg::Fp>& x) {  // x is consumed
        for (uint32_t c = 0; c < w; c++) if (!x[c].is_zero()) nonzero[c] = 1;
        if (rho == w) return;
        // the pivot columns of the other rows are zero in every basis row, so the coefficients can all be read before any update
        for (uint32_t p = 0; p < w; p++) {
            if (row_of[p] < 0 || x[p].is_zero()) continue;
            const vg::Fp coef = x[p];
            const vg::Fp* b = &rows[(size_t)row_of[p] * w];
            for (uint32_t c = 0; c < w; c++) x[c] -= coef * b[c];
        }
        uint32_t pc = 0;
        while (pc < w && x[pc].is_zero()) pc++;
        if (pc == w) return;
        const vg::Fp inv = x[pc].inv();
        for (uint32_t c = 0; c < w; c++) x[c] *= inv;
        for (uint32_t i = 0; i < rho; i++) {
            vg::Fp* b = &rows[(size_t)i * w];
            const vg::Fp coef = b[pc];
            if (coef.is_zero()) continue;
            for (uint32_t c = 0; c < w; c++) b[c] -= coef * x[c];
        }
        std::copy(x.begin(), x.end(), rows.begin() + (size_t)rho * w);
        row_of[pc] = (int32_t)rho++;
    }
    uint32_t zero_columns() const { uint32_t z = 0; for (uint32_t c = 0; c < w; c++) z += nonzero[c] ? 0 : 1; return z; }
    // pinned: a pivot column whose row has no other non-zero entry
    bool pinned(uint32_t c) const {
        if (row_of[c] < 0) return false;
        const vg::Fp* b = &rows[(size_t)row_of[c] * w];
        for (uint32_t k = 0; k < w; k++) if (k != c && !b[k].is_zero()) return false;
        return true;
    }
    // the canonical null vector of a loose column
    RankListedRow null_vector(uint32_t c, uint32_t row) const {
        uint32_t f = c;
        if (row_of[c] >= 0) {
            const vg::Fp* b = &rows[(size_t)row_of[c] * w];
            for (f = 0; f < w; f++) if (row_of[f] < 0 && !b[f].is_zero()) break;
        }
        RankListedRow out;
        out.row = row;
        for (uint32_t k = 0; k < w; k++) {
            vg::Fp v = vg::Fp::zero();
            if (k == f) v = vg::Fp::one();
            else if (row_of[k] >= 0) v = -rows[(size_t)row_of[k] * w + f];
            if (v.is_zero()) continue;
            if (out.n_support < RA_TERMS) { out.terms[2 * out.n_support] = k; out.terms[2 * out.n_support + 1] = v.canonical(); }
            out.n_support++;
        }
        return out;
    }
};

// chips[].{loose_cols, pinned_cols, coupled_cols}, total_entries, truncated and the entries (without rows) from the per-column counts
inline void rank_audit_finish(RankReport& r, const RankAuditOpts& o) {
    r.total_entries = 0;
    r.entries.clear();
    for (size_t c = 0; c < r.chips.size(); c++) {
        RankChipStat& cs = r.chips[c];
        cs.loose_cols = cs.pinned_cols = cs.coupled_cols = 0;
        if (!cs.audited) continue;
        for (uint32_t k = 0; k < cs.width; k++) {
            if (cs.loose[k]) cs.loose_cols++; else cs.pinned_cols++;
            const uint64_t coupled = cs.loose[k] - cs.zeros[k];
            if (!coupled) continue;
            cs.coupled_cols++;
            r.total_entries++;
            if (r.entries.size() < o.max_entries) {
                RankEntry e;
                e.chip = (uint32_t)c; e.column = k; e.coupled = coupled;
                r.entries.push_back(std::move(e));
            }
        }
    }
    r.truncated = r.total_entries > r.entries.size();
}

// The contract on the host: a dual-number (value, derivative) evaluation of the chip's Program seeded at one (column, role), the interaction
// rows from the VirtualCol weights, RREF by row insertion; one thread.  per_row (optional) sees the reduced basis of every audited row, in
// (chip, row) order, right after the row's own analysis: the step audit (host/step_audit.hpp) takes its directions there.
using RankRowFn = std::function<void(size_t chip, uint64_t row, const RankBasis& basis)>;
inline RankReport rank_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                  const std::vector<ConstraintHostMatrix>& prep, const RankAuditOpts& opts_in, const RankRowFn& per_row = nullptr) {
    const RankAuditOpts o = rank_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("rank_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("rank_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    rank_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    RankReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<std::vector<RankListedRow>>> first(NC);
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        const vair::Program& p = air.program;
        const uint32_t K = p.num_asserts, W = air.width, PW = air.prep_width;
        const ConstraintHostMatrix& mm = main[c];
        const uint64_t n = mm.height;
        RankChipStat& cs = rep.chips[c];
        cs.width = W; cs.n_constraints = K; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = n;
        cs.audited = rank_audit_selected(o, c) ? 1u : 0u;
        cs.loose.assign(W, 0); cs.zeros.assign(W, 0);
        first[c].resize(W);
        if (!cs.audited || !W) continue;
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
        const std::vector<uint32_t> wr = ra_weight_rows(air);
        auto vcol = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* pr) {
            uint64_t acc = v.constant % vg::P;
            for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? pr : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
            return (uint32_t)acc;
        };
        std::vector<vg::Fp> jl((size_t)K * W ? (size_t)K * W : 1), jn(jl.size()), x(W);
        RankBasis B;
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t rp = (r + n - 1) & (n - 1);
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
            const uint32_t* crow = mm.data + r * W;
            const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
            for (size_t m = 0; m < air.interactions.size(); m++) {
                const uint32_t at = wr[2 + m], nf = wr[at];
                const bool live = vcol(air.interactions[m].count, crow, cprow) != 0;
                for (uint32_t j = 0; j < (live ? 1 + nf : 1u); j++) {
                    for (uint32_t k = 0; k < W; k++) x[k] = vg::Fp::raw(wr[at + 1 + (size_t)j * W + k]);
                    B.insert(x);
                }
            }
            const uint32_t nu = W - B.rho, z = B.zero_columns();
            cs.nullity += nu; cs.zero += z;
            if (nu > z) cs.coupled_rows++;
            cs.max_nullity = std::max(cs.max_nullity, nu);
            for (uint32_t col = 0; col < W; col++) {
                if (B.pinned(col)) continue;
                cs.loose[col]++;
                if (!B.nonzero[col]) { cs.zeros[col]++; continue; }
                if (first[c][col].size() < R) first[c][col].push_back(B.null_vector(col, (uint32_t)r));
            }
            if (per_row) per_row(c, r, B);
        }
    }
    rank_audit_finish(rep, o);
    for (auto& e : rep.entries) e.rows = std::move(first[e.chip][e.column]);
    return rep;
}

}  // namespace vhost
