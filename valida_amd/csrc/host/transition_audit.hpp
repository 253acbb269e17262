// Transition audit: the invariant audit (host/invariant_audit.hpp) over a two-row window and under a gate.  Which affine-linear relations between
// a row and its successor does the WITNESS keep, on every window or on the windows where a boolean column holds one value, and at which of those
// windows do the chip's constraints and records enforce each of them to first order.
//   windows     chip h, main matrix M (n x w, canonical): window r = 0 .. n - 2 (no wrap: the AIR's when_transition domain) is the row
//               a_r = (1, M[r][0..w), M[r + 1][0..w)) of AW = 2 w + 1 WINDOW COLUMNS: 0 the constant, 1 + c `local` c, 1 + w + c `next` c.
//               n = 1: no windows, the chip's block is zero but for its first six words.
//   gates       window column j >= 1 is BOOLEAN when its values over all windows lie in {0, 1} and both occur.  Gate 0: every window.  Then for
//               every boolean j ascending the gates (j = 1), (j = 0).  max_gates cuts this list (gate 0 included); n_bool and n_gates stay exact.
//               A gate of fewer than min_gate_windows windows is listed but not audited (a short program floods the report with accidental
//               relations otherwise); gate 0 is always audited.
//   space       R_g = the reduced row echelon form of the a_r of the windows where g holds, columns in that order: unique, so no grid, tree or
//               row order changes a word.  rho_g, d_g = AW - rho_g.  pivots(g) is a subset of pivots(0) (asserted).
//   entries     the canonical vector of a non-pivot column f: l_f = 1, l_p = -R_g[row of p][f] for the pivots p (all left of f), 0 elsewhere.
//               Gate 0 lists every non-pivot f of the `next` block whose vector has a non-zero `local` coefficient (kind 2); its other
//               non-pivots are only counted: local_only (the invariant audit's subject) and next_only (the same relations shifted).
//               Gate g >= 1 lists every f in pivots(0) \ pivots(g) but the gate's own column: what the gate adds.  kind 0: a constant (only l_0
//               and l_f), 1: one block, 2: both blocks.  Entries ascend by (chip, gate, f); max_entries cuts the list, and entries cut from it
//               are not judged.
//   verdict     per window r of the entry's gate, J the rank audit's Jacobian (host/rank_audit.hpp, the same matrix word for word): FREE at r
//               iff l's `local` part is outside the row space of J_r or its `next` part outside that of J_{r + 1} (a first-order-unnoticed move
//               of ONE of the two rows breaks the relation), otherwise HELD at r.  One-sided: free is a certificate; held is exact for a chip
//               none of whose constraints reads `next` (the joint Jacobian is block diagonal), otherwise "no one-row move breaks it".
// What it is not: affine-linear only; single gates (no conjunction of two); no joint 2 w-column Jacobian; THIS witness; per basis vector; first
// order, with the rank audit's caveats.  `check`'s exit status never depends on it.
// This header holds what the host and the device implementation share (options, the report and its word image, gates from the column flags,
// entries from the gates' bases) and the host implementation (plain C++, one thread, no limits).  The device pass is Prover::transition_audit
// (prover_audits.cpp, kernels/transition_audit.hip).
#pragma once
#include "rank_audit.hpp"

namespace vhost {

struct TransitionAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t chip_mask = 0;           // bit h: audit chip h; 0: all chips
    uint32_t max_terms = 8;           // (window column, coefficient) terms listed per entry
    uint32_t min_gate_windows = 64;   // a gate of fewer windows is not audited
    uint32_t max_gates = 256;         // gates listed per chip, gate 0 included
    uint32_t reserved[3] = {0, 0, 0};
};

struct TransitionChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t n_bool = 0, n_gates = 0, gates_listed = 0, gates_audited = 0;  // n_gates = 1 + 2 n_bool, exact whatever max_gates is
    uint32_t rank = 0, dim = 0;                                             // rho_0, d_0
    uint32_t local_only = 0, next_only = 0, transitions = 0, gated = 0;     // d_0 split three ways; entries of the gates >= 1
};
struct TransitionGate {
    uint32_t chip = 0, column = 0, value = 0, audited = 0;  // column 0: gate 0
    uint64_t windows = 0;
    uint32_t rank = 0, dim = 0, added = 0;  // added: the gate's entries, exact even when the list is cut
};
struct TransitionEntry {
    uint32_t chip = 0, gate_column = 0, gate_value = 0, column = 0, kind = 0;
    uint32_t l0 = 0, n_support = 0;  // canonical constant term; window columns >= 1 with a non-zero coefficient, f included
    std::vector<uint32_t> terms;     // the first max_terms (window column, coefficient), ascending
    uint64_t free_windows = 0, held_windows = 0;
    std::vector<uint32_t> rows;      // the first max_rows_per_entry free windows, ascending
    std::vector<vg::Fp> l;           // the whole vector, AW Montgomery words: not part of the word image
};
struct TransitionReport {
    bool truncated = false;
    uint32_t max_terms = 8, min_gate_windows = 64, max_gates = 256;
    uint64_t total_entries = 0;  // exact even when the list is cut
    std::vector<TransitionChipStat> chips;
    std::vector<TransitionGate> gates;      // ascending (chip, position in the chip's gate list)
    std::vector<TransitionEntry> entries;   // ascending (chip, gate, column)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31525456u;  // "VTR1"
    // Flat image (include/vgpu.h documents it next to vgpu_transition_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(max_terms); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        w.push_back((uint32_t)gates.size()); w.push_back(min_gate_windows); w.push_back(max_gates); w.push_back(0);
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height);
            w.push_back(c.n_bool); w.push_back(c.n_gates); w.push_back(c.gates_listed); w.push_back(c.gates_audited);
            w.push_back(c.rank); w.push_back(c.dim);
            w.push_back(c.local_only); w.push_back(c.next_only); w.push_back(c.transitions); w.push_back(c.gated);
        }
        for (auto& g : gates) {
            w.push_back(g.chip); w.push_back(g.column); w.push_back(g.value); w.push_back(g.audited);
            u64(g.windows);
            w.push_back(g.rank); w.push_back(g.dim); w.push_back(g.added); w.push_back(0);
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.gate_column); w.push_back(e.gate_value); w.push_back(e.column);
            w.push_back(e.kind); w.push_back(e.l0); w.push_back(e.n_support); w.push_back((uint32_t)(e.terms.size() / 2));
            w.push_back((uint32_t)e.rows.size()); w.push_back(0);
            u64(e.free_windows); u64(e.held_windows);
            w.insert(w.end(), e.terms.begin(), e.terms.end());
            w.insert(w.end(), e.rows.begin(), e.rows.end());
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string ta_renamed(const std::invalid_argument& e) {
    const std::string m = e.what(), from = "rank_audit: ";
    return m.compare(0, from.size(), from) == 0 ? "transition_audit: " + m.substr(from.size()) : m;
}

inline TransitionAuditOpts transition_audit_checked_opts(const TransitionAuditOpts& in, size_t n_chips) {
    if (in.reserved[0] != 0 || in.reserved[1] != 0 || in.reserved[2] != 0) throw std::invalid_argument("transition_audit: the reserved fields of the options must be zero");
    TransitionAuditOpts o = in;
    RankAuditOpts ro;
    ro.max_entries = in.max_entries; ro.max_rows_per_entry = in.max_rows_per_entry; ro.chip_mask = in.chip_mask;
    try {
        ro = rank_audit_checked_opts(ro, n_chips);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(ta_renamed(e));
    }
    o.max_entries = ro.max_entries; o.max_rows_per_entry = ro.max_rows_per_entry;
    if (o.max_terms == 0) o.max_terms = 8;
    if (o.max_terms > 4096) throw std::invalid_argument("transition_audit: max_terms is at most 4096");
    if (o.min_gate_windows == 0) o.min_gate_windows = 64;
    if (o.max_gates == 0) o.max_gates = 256;
    if (o.max_gates > 4096) throw std::invalid_argument("transition_audit: max_gates is at most 4096");
    return o;
}
inline bool transition_audit_selected(const TransitionAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void transition_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                  std::vector<int>& prep_slot) {
    try {
        rank_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(ta_renamed(e));
    }
}

// The static part of a chip's block
inline void transition_audit_chip_block(TransitionChipStat& cs, const AirDesc& air, uint64_t height, bool audited) {
    cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = height;
    cs.audited = audited ? 1u : 0u;
}
// does the chip have anything to audit
inline bool transition_audit_has_windows(const TransitionChipStat& cs) { return cs.audited && cs.width && cs.height >= 2; }

// Flags of a window column over all windows (both passes compute them)
constexpr uint32_t TA_OUTSIDE = 1, TA_ANY0 = 2, TA_ANY1 = 4;

// One chip's gate list from its window columns' flags [AW] (index 0 unused) and the windows on which each column is 1 [AW]: n_bool, n_gates,
// gates_listed, gates_audited of the chip's block and the listed gates (rank, dim, added are filled in later).
inline void transition_audit_gates(TransitionChipStat& cs, uint32_t chip, const std::vector<uint32_t>& flags, const std::vector<uint64_t>& ones, const TransitionAuditOpts& o,
                                   std::vector<TransitionGate>& out) {
    const uint32_t AW = 2 * cs.width + 1;
    const uint64_t NWIN = cs.height - 1;
    cs.n_bool = 0; cs.gates_listed = 0; cs.gates_audited = 0;
    auto push = [&](uint32_t j, uint32_t v, uint64_t windows) {
        if (cs.gates_listed >= o.max_gates) return;
        TransitionGate g;
        g.chip = chip; g.column = j; g.value = v; g.windows = windows;
        g.audited = (j == 0 || windows >= o.min_gate_windows) ? 1u : 0u;
        cs.gates_listed++; cs.gates_audited += g.audited;
        out.push_back(g);
    };
    push(0, 0, NWIN);
    for (uint32_t j = 1; j < AW; j++) {
        if (flags[j] != (TA_ANY0 | TA_ANY1)) continue;
        cs.n_bool++;
        push(j, 1, ones[j]);
        push(j, 0, NWIN - ones[j]);
    }
    cs.n_gates = 1 + 2 * cs.n_bool;
}

// The reduced basis of one gate as both passes hand it over: pivot [AW], and per non-pivot column ascending its canonical vector (AW Montgomery words)
struct TransitionBasis {
    std::vector<uint8_t> pivot;
    std::vector<vg::Fp> vec;
};

// The entries of one audited gate from its basis (b0: gate 0's basis of the chip): rank, dim, added of the gate and, for gate 0, the chip's split
// of d_0; all entries, the caller cuts the list.
inline void transition_audit_entries(TransitionChipStat& cs, TransitionGate& g, const TransitionBasis& b0, const TransitionBasis& b, uint32_t max_terms,
                                     std::vector<TransitionEntry>& out) {
    const uint32_t W = cs.width, AW = 2 * W + 1;
    g.rank = 0;
    for (uint32_t c = 0; c < AW; c++) {
        g.rank += b.pivot[c] ? 1u : 0u;
        if (b.pivot[c] && !b0.pivot[c]) throw std::logic_error("transition_audit: the pivots of a gate are not among the pivots of gate 0");
    }
    g.dim = AW - g.rank; g.added = 0;
    if (g.column == 0) { cs.rank = g.rank; cs.dim = g.dim; cs.local_only = cs.next_only = cs.transitions = 0; }
    uint32_t i = 0;
    for (uint32_t f = 0; f < AW; f++) {
        if (b.pivot[f]) continue;
        const vg::Fp* l = b.vec.data() + (size_t)i++ * AW;
        bool loc = false, nxt = false;
        for (uint32_t c = 1; c <= W; c++) loc |= !l[c].is_zero();
        for (uint32_t c = W + 1; c < AW; c++) nxt |= !l[c].is_zero();
        if (g.column == 0) {
            if (f <= W) { cs.local_only++; continue; }
            if (!loc) { cs.next_only++; continue; }
            cs.transitions++;
        } else {
            if (!b0.pivot[f] || f == g.column) continue;
            cs.gated++;
        }
        g.added++;
        TransitionEntry e;
        e.chip = g.chip; e.gate_column = g.column; e.gate_value = g.value; e.column = f; e.l0 = l[0].canonical();
        for (uint32_t c = 1; c < AW; c++) {
            if (l[c].is_zero()) continue;
            if (e.n_support < max_terms) { e.terms.push_back(c); e.terms.push_back(l[c].canonical()); }
            e.n_support++;
        }
        e.kind = e.n_support == 1 ? 0u : ((loc && nxt) ? 2u : 1u);
        e.l.assign(l, l + AW);
        out.push_back(std::move(e));
    }
}

// total_entries and the cut at max_entries: before the verdicts, entries cut from the list are not judged
inline void transition_audit_cut(TransitionReport& r, const TransitionAuditOpts& o) {
    r.max_terms = o.max_terms; r.min_gate_windows = o.min_gate_windows; r.max_gates = o.max_gates;
    r.total_entries = r.entries.size();
    if (r.entries.size() > o.max_entries) r.entries.resize((size_t)o.max_entries);
    r.truncated = r.total_entries > r.entries.size();
}

// The contract on the host: the flags by one pass over the columns, RREF of the gated windows by insertion (RankBasis of width 2 w + 1), then
// the rank audit's host Jacobian and RREF per row (rank_audit_host's per_row), each half of each listed vector reduced against it; one thread.
inline TransitionReport transition_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                              const std::vector<ConstraintHostMatrix>& prep, const TransitionAuditOpts& opts_in) {
    const TransitionAuditOpts o = transition_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("transition_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("transition_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    transition_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    TransitionReport rep;
    rep.chips.resize(NC);
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        TransitionChipStat& cs = rep.chips[c];
        transition_audit_chip_block(cs, air, main[c].height, transition_audit_selected(o, c));
        if (!transition_audit_has_windows(cs)) continue;
        const uint32_t W = air.width, AW = 2 * W + 1;
        const uint64_t n = main[c].height, NWIN = n - 1;
        const uint32_t* M = main[c].data;
        auto at = [&](uint64_t r, uint32_t j) { return j <= W ? M[r * W + (j - 1)] : M[(r + 1) * W + (j - 1 - W)]; };
        std::vector<uint32_t> flags(AW, 0);
        std::vector<uint64_t> ones(AW, 0);
        for (uint64_t r = 0; r < NWIN; r++)
            for (uint32_t j = 1; j < AW; j++) {
                const uint32_t v = at(r, j);
                flags[j] |= v == 0 ? TA_ANY0 : (v == 1 ? TA_ANY1 : TA_OUTSIDE);
                ones[j] += v == 1;
            }
        const size_t g0 = rep.gates.size();
        transition_audit_gates(cs, (uint32_t)c, flags, ones, o, rep.gates);
        TransitionBasis b0;
        std::vector<vg::Fp> x(AW);
        for (size_t gi = g0; gi < rep.gates.size(); gi++) {
            TransitionGate& g = rep.gates[gi];
            if (!g.audited) continue;
            RankBasis B;
            B.reset(AW);
            for (uint64_t r = 0; r < NWIN && B.rho < AW; r++) {
                if (g.column && at(r, g.column) != g.value) continue;
                x[0] = vg::Fp::one();
                for (uint32_t j = 1; j < AW; j++) x[j] = vg::Fp::from_canonical(at(r, j));
                B.insert(x);
            }
            TransitionBasis b;
            b.pivot.resize(AW);
            for (uint32_t f = 0; f < AW; f++) b.pivot[f] = B.row_of[f] >= 0;
            for (uint32_t f = 0; f < AW; f++) {
                if (b.pivot[f]) continue;
                for (uint32_t k = 0; k < AW; k++) b.vec.push_back(k == f ? vg::Fp::one() : (b.pivot[k] ? -B.rows[(size_t)B.row_of[k] * AW + f] : vg::Fp::zero()));
            }
            if (gi == g0) b0 = b;
            transition_audit_entries(cs, g, b0, b, o.max_terms, rep.entries);
        }
    }
    transition_audit_cut(rep, o);
    // the verdicts of the listed entries
    std::vector<size_t> e_at(NC + 1, rep.entries.size());
    uint32_t need_mask = 0;
    for (size_t e = rep.entries.size(); e-- > 0;) { e_at[rep.entries[e].chip] = e; if (rep.entries[e].chip < 32) need_mask |= 1u << rep.entries[e].chip; }
    for (size_t c = NC; c-- > 0;) if (e_at[c] > e_at[c + 1]) e_at[c] = e_at[c + 1];
    if (!rep.entries.empty()) {
        std::vector<uint8_t> prev_a(rep.entries.size(), 0);  // the `local` half of the entry was free at the row before
        std::vector<vg::Fp> x;
        auto outside = [&](const RankBasis& B, const vg::Fp* cv) {
            const uint32_t W = B.w;
            x.assign(cv, cv + W);
            // the basis is reduced: the coefficients can all be read before any update
            for (uint32_t p = 0; p < W; p++) {
                if (B.row_of[p] < 0 || cv[p].is_zero()) continue;
                const vg::Fp* b = &B.rows[(size_t)B.row_of[p] * W];
                for (uint32_t k = 0; k < W; k++) x[k] -= cv[p] * b[k];
            }
            for (uint32_t k = 0; k < W; k++) if (!x[k].is_zero()) return true;
            return false;
        };
        auto per_row = [&](size_t c, uint64_t r, const RankBasis& B) {
            const uint32_t W = B.w;
            const uint64_t n = main[c].height;
            const uint32_t* M = main[c].data;
            auto holds = [&](const TransitionEntry& e, uint64_t win) {
                const uint32_t j = e.gate_column;
                return !j || (j <= W ? M[win * W + (j - 1)] : M[(win + 1) * W + (j - 1 - W)]) == e.gate_value;
            };
            for (size_t ei = e_at[c]; ei < e_at[c + 1]; ei++) {
                TransitionEntry& e = rep.entries[ei];
                if (r >= 1 && holds(e, r - 1)) {
                    if (prev_a[ei] || outside(B, e.l.data() + 1 + W)) {
                        e.free_windows++;
                        if (e.rows.size() < R) e.rows.push_back((uint32_t)(r - 1));
                    } else {
                        e.held_windows++;
                    }
                }
                prev_a[ei] = (r + 1 < n && holds(e, r)) ? outside(B, e.l.data() + 1) : 0;
            }
        };
        RankAuditOpts ro;
        ro.max_entries = 1; ro.max_rows_per_entry = 1;
        ro.chip_mask = NC <= 32 ? need_mask : 0;  // chips without a listed entry have nothing to judge
        try {
            const RankReport rr = rank_audit_host(machine, main, prep_chips, prep, ro, per_row);
            rep.evaluations = rr.evaluations;
        } catch (const std::invalid_argument& e) {
            throw std::invalid_argument(ta_renamed(e));
        }
    }
    return rep;
}

}  // namespace vhost
