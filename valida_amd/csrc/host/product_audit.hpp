// Product audit: the invariant audit one degree up.  The invariant audit lists the affine-linear relations a chip's WITNESS keeps on every row; the
// constraints a chip consists of are mostly of degree two (b^2 = b, s t = 0, s t = s, s x = y, a b = c), and this audit lists those: the
// products of two columns that are an affine function of the row, and on how many rows the chip's own constraints and records enforce each.
//   space          chip h, main matrix M (n x w, canonical): a_r = (1, M[r][0], .., M[r][w - 1]); R = the reduced row echelon form of the a_r
//                  (the invariant audit's R, word for word), Pi its pivot columns (column 0 always), rho = |Pi|.  The q = rho - 1 pivot main
//                  columns are the INDEPENDENT columns; a non-pivot column is an affine function of earlier ones (the invariant audit reports
//                  that) and takes no part.
//   pairs          all (i, j), i <= j, both independent, in lexicographic order: m = q (q + 1) / 2.
//   relation       pair (i, j) is a relation iff some beta in F_p^(w + 1) supported on Pi has M[r][i] M[r][j] = beta . a_r on every row r.  The
//                  columns of Pi are linearly independent over the rows, so beta is unique: no grid, order or seed changes a word.
//   kinds          0 BOOLEAN: i = j and beta = e_i;  1 ZERO: beta = 0;  2 SELECT: i != j and beta = e_i or e_j (one column is 1 wherever the
//                  other is non-zero);  3 OTHER.
//   verdict        the gradient of x_i x_j - beta . (1, x) at row r: g_r[k] = [k = i] M[r][j] + [k = j] M[r][i] - beta_(k + 1) (i = j: 2 M[r][i]).
//                  ENFORCED at r iff g_r lies in the row space of the rank audit's Jacobian J_r (host/rank_audit.hpp, the same matrix word
//                  for word; n = 1 by its rule); FLAT iff g_r = 0 (counted among the enforced rows and on its own: first order says nothing
//                  there, as x y = 0 at x = y = 0); FREE otherwise: some first-order-unnoticed move of the row's cells breaks the relation.
// What it is not: single products only (s a - s b = 0 is found only when s a and s b are each affine); one row; THIS witness; first order, with
// the rank audit's caveats.  `check`'s exit status never depends on it.
// This header holds what the host and the device implementation share — options, the report and its word image, the entry of a pair from its
// beta — and the host implementation (plain C++, one thread, no limits).  The device pass is Prover::product_audit (prover_audits.cpp,
// kernels/product_audit.hip).
#pragma once
#include "invariant_audit.hpp"

namespace vhost {

struct ProductAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t chip_mask = 0;  // bit h: audit chip h; 0: all chips
    uint32_t max_terms = 8;  // (column, coefficient) terms listed per relation
    uint32_t reserved[3] = {0, 0, 0};
};

constexpr uint32_t PQ_BOOLEAN = 0, PQ_ZERO = 1, PQ_SELECT = 2, PQ_OTHER = 3;

struct ProductChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t rank = 0, pairs = 0;  // rho (q = rho - 1 independent columns), m = q (q + 1) / 2
    uint32_t relations = 0, boolean_ = 0, zero = 0, select = 0, other = 0;
    uint32_t every = 0, some = 0, never = 0;  // relations enforced on every row, on some rows, on no row
};
struct ProductEntry {
    uint32_t chip = 0, i = 0, j = 0, kind = 0;
    uint32_t b0 = 0, n_support = 0;  // canonical beta_0; main columns with a non-zero coefficient in beta (exact)
    std::vector<uint32_t> terms;     // the first max_terms (column, coefficient), ascending column
    uint64_t enforced = 0, free_rows = 0, flat_rows = 0;
    std::vector<uint32_t> rows;      // the first max_rows_per_entry free rows, ascending
};
// What the enforcement phase needs of an entry: -beta on the main columns, sparse, Montgomery
struct ProductVec {
    uint32_t i = 0, j = 0;
    std::vector<uint32_t> cols;
    std::vector<vg::Fp> neg;
};
struct ProductReport {
    bool truncated = false;
    uint32_t max_terms = 8;
    uint64_t total_entries = 0;  // the relations of the audited chips, exact even when the list is cut
    std::vector<ProductChipStat> chips;
    std::vector<ProductEntry> entries;  // ascending (chip, i, j)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31525156u;  // "VQR1"
    // Flat image (include/vgpu.h documents it next to vgpu_product_report_words)
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
            w.push_back(c.rank); w.push_back(c.pairs);
            w.push_back(c.relations); w.push_back(c.boolean_); w.push_back(c.zero); w.push_back(c.select); w.push_back(c.other);
            w.push_back(c.every); w.push_back(c.some); w.push_back(c.never);
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.i); w.push_back(e.j); w.push_back(e.kind);
            w.push_back(e.b0); w.push_back(e.n_support); w.push_back((uint32_t)(e.terms.size() / 2)); w.push_back((uint32_t)e.rows.size());
            u64(e.enforced); u64(e.free_rows); u64(e.flat_rows);
            w.push_back(0); w.push_back(0);
            w.insert(w.end(), e.terms.begin(), e.terms.end());
            w.insert(w.end(), e.rows.begin(), e.rows.end());
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string pq_renamed(const std::invalid_argument& e) {
    const std::string m = e.what(), from = "invariant_audit: ";
    return m.compare(0, from.size(), from) == 0 ? "product_audit: " + m.substr(from.size()) : m;
}

// the same defaults and refusals as the invariant audit's options
inline ProductAuditOpts product_audit_checked_opts(const ProductAuditOpts& in, size_t n_chips) {
    InvariantAuditOpts io;
    io.max_entries = in.max_entries; io.max_rows_per_entry = in.max_rows_per_entry; io.chip_mask = in.chip_mask; io.max_terms = in.max_terms;
    for (int k = 0; k < 3; k++) io.reserved[k] = in.reserved[k];
    try {
        io = invariant_audit_checked_opts(io, n_chips);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(pq_renamed(e));
    }
    ProductAuditOpts o = in;
    o.max_entries = io.max_entries; o.max_rows_per_entry = io.max_rows_per_entry; o.max_terms = io.max_terms;
    return o;
}
inline bool product_audit_selected(const ProductAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void product_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                               std::vector<int>& prep_slot) {
    try {
        invariant_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(pq_renamed(e));
    }
}

// The static part of a chip's block
inline void product_audit_chip_block(ProductChipStat& cs, const AirDesc& air, uint64_t height, bool audited) {
    cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = height;
    cs.audited = audited ? 1u : 0u;
}

// rho and m of a chip's block from its pivot columns (pcols: the augmented pivot columns ascending, pcols[0] = 0)
inline void product_audit_space(ProductChipStat& cs, const std::vector<uint32_t>& pcols) {
    const uint64_t q = pcols.size() - 1;
    cs.rank = (uint32_t)pcols.size();
    cs.pairs = (uint32_t)(q * (q + 1) / 2);
}

// Pair p (0 .. m - 1, lexicographic) of q independent columns as (ti, tj), 1 <= ti <= tj <= q: positions in pcols
inline void product_audit_pair(uint32_t q, uint32_t p, uint32_t& ti, uint32_t& tj) {
    uint32_t t = 1;
    while (p >= q - t + 1) { p -= q - t + 1; t++; }
    ti = t; tj = t + p;
}

// One relation from its beta over Pi (rho Montgomery words, beta[t] the coefficient of augmented column pcols[t]): the entry (counts and rows
// are filled in later), its enforcement vector, and the chip's counts by kind.
inline void product_audit_entry(ProductChipStat& cs, uint32_t chip, const std::vector<uint32_t>& pcols, uint32_t ti, uint32_t tj, const vg::Fp* beta, uint32_t max_terms,
                                std::vector<ProductEntry>& out, std::vector<ProductVec>& vecs) {
    ProductEntry e;
    ProductVec v;
    e.chip = chip; e.i = v.i = pcols[ti] - 1; e.j = v.j = pcols[tj] - 1; e.b0 = beta[0].canonical();
    bool unit_i = beta[0].is_zero(), unit_j = beta[0].is_zero();  // beta = e_i, beta = e_j
    for (uint32_t t = 1; t < pcols.size(); t++) {
        unit_i &= beta[t] == (t == ti ? vg::Fp::one() : vg::Fp::zero());
        unit_j &= beta[t] == (t == tj ? vg::Fp::one() : vg::Fp::zero());
        if (beta[t].is_zero()) continue;
        if (e.n_support < max_terms) { e.terms.push_back(pcols[t] - 1); e.terms.push_back(beta[t].canonical()); }
        e.n_support++;
        v.cols.push_back(pcols[t] - 1); v.neg.push_back(-beta[t]);
    }
    if (!e.n_support && !e.b0) e.kind = PQ_ZERO;
    else if (ti == tj && unit_i) e.kind = PQ_BOOLEAN;
    else if (ti != tj && (unit_i || unit_j)) e.kind = PQ_SELECT;
    else e.kind = PQ_OTHER;
    cs.relations++;
    (e.kind == PQ_BOOLEAN ? cs.boolean_ : e.kind == PQ_ZERO ? cs.zero : e.kind == PQ_SELECT ? cs.select : cs.other)++;
    out.push_back(std::move(e));
    vecs.push_back(std::move(v));
}

// One chip's entries from what the device pass found: rel (the pairs that are relations, ascending) and betas (per relation rho Montgomery words)
inline void product_audit_chip_entries(ProductChipStat& cs, uint32_t chip, const std::vector<uint32_t>& pcols, const std::vector<uint32_t>& rel, const std::vector<uint32_t>& betas,
                                       uint32_t max_terms, std::vector<ProductEntry>& out, std::vector<ProductVec>& vecs) {
    const uint32_t rho = (uint32_t)pcols.size();
    std::vector<vg::Fp> beta(rho);
    for (size_t k = 0; k < rel.size(); k++) {
        uint32_t ti, tj;
        product_audit_pair(rho - 1, rel[k], ti, tj);
        for (uint32_t t = 0; t < rho; t++) beta[t] = vg::Fp::raw(betas[k * rho + t]);
        product_audit_entry(cs, chip, pcols, ti, tj, beta.data(), max_terms, out, vecs);
    }
}

// The relations of one chip as the enforcement kernel takes them (kernels/launch.hpp, PqArgs): eoff [E + 1], ewords (i, j, then (column, -beta)
// per entry for beta's support and for i and j, each column once), and the groups staged in LDS at a time: consecutive entries, at most cap_entries of them and cap_words words (one entry always fits:
// 2 + 2 x 191 words).
struct ProductLists {
    std::vector<uint32_t> eoff, ewords, gstart;
    uint32_t GE = 0, GW = 0;  // the most entries and the most words of a group
};
inline ProductLists product_audit_lists(const ProductVec* v, size_t E, uint32_t cap_entries, uint32_t cap_words) {
    ProductLists l;
    l.eoff.push_back(0);
    for (size_t e = 0; e < E; e++) {
        l.ewords.push_back(v[e].i); l.ewords.push_back(v[e].j);
        bool has_i = false, has_j = false;
        for (size_t k = 0; k < v[e].cols.size(); k++) {
            l.ewords.push_back(v[e].cols[k]); l.ewords.push_back(v[e].neg[k].v);
            has_i |= v[e].cols[k] == v[e].i; has_j |= v[e].cols[k] == v[e].j;
        }
        // the kernel adds the row's cells where it scatters the list: i and j are always listed, each column once
        if (!has_i) { l.ewords.push_back(v[e].i); l.ewords.push_back(0); }
        if (!has_j && v[e].j != v[e].i) { l.ewords.push_back(v[e].j); l.ewords.push_back(0); }
        l.eoff.push_back((uint32_t)l.ewords.size());
    }
    l.gstart.push_back(0);
    size_t e0 = 0;
    for (size_t e = 0; e <= E; e++) {
        const bool full = e < E && (e - e0 == cap_entries || (e > e0 && l.eoff[e + 1] - l.eoff[e0] > cap_words));
        if (e == E || full) {
            if (e > e0) {
                l.gstart.push_back((uint32_t)e);
                l.GE = std::max<uint32_t>(l.GE, (uint32_t)(e - e0));
                l.GW = std::max<uint32_t>(l.GW, l.eoff[e] - l.eoff[e0]);
            }
            e0 = e;
        }
    }
    return l;
}

// every / some / never of the chips' blocks from the entries' counts (all entries of every audited chip), then the cut at max_entries
inline void product_audit_finish(ProductReport& r, const ProductAuditOpts& o) {
    r.max_terms = o.max_terms;
    for (auto& cs : r.chips) cs.every = cs.some = cs.never = 0;
    for (auto& e : r.entries) {
        ProductChipStat& cs = r.chips[e.chip];
        if (!e.free_rows) cs.every++; else if (!e.enforced) cs.never++; else cs.some++;
    }
    r.total_entries = r.entries.size();
    if (r.entries.size() > o.max_entries) r.entries.resize((size_t)o.max_entries);
    r.truncated = r.total_entries > r.entries.size();
}

// The inverse of the regular rho x rho matrix a (row-major), by Gauss-Jordan on (a | 1); false when a is singular
inline bool product_audit_invert(std::vector<vg::Fp>& a, uint32_t rho, std::vector<vg::Fp>& inv) {
    inv.assign((size_t)rho * rho, vg::Fp::zero());
    for (uint32_t k = 0; k < rho; k++) inv[(size_t)k * rho + k] = vg::Fp::one();
    for (uint32_t k = 0; k < rho; k++) {
        uint32_t p = k;
        while (p < rho && a[(size_t)p * rho + k].is_zero()) p++;
        if (p == rho) return false;
        if (p != k)
            for (uint32_t c = 0; c < rho; c++) { std::swap(a[(size_t)p * rho + c], a[(size_t)k * rho + c]); std::swap(inv[(size_t)p * rho + c], inv[(size_t)k * rho + c]); }
        const vg::Fp s = a[(size_t)k * rho + k].inv();
        for (uint32_t c = 0; c < rho; c++) { a[(size_t)k * rho + c] *= s; inv[(size_t)k * rho + c] *= s; }
        for (uint32_t r = 0; r < rho; r++) {
            const vg::Fp f = a[(size_t)r * rho + k];
            if (r == k || f.is_zero()) continue;
            for (uint32_t c = 0; c < rho; c++) { a[(size_t)r * rho + c] -= f * a[(size_t)k * rho + c]; inv[(size_t)r * rho + c] -= f * inv[(size_t)k * rho + c]; }
        }
    }
    return true;
}

// The contract on the host: the pivots by insertion (RankBasis of width w + 1, the invariant audit's), the rows that raised the rank, the
// inverse of their rho x rho matrix over Pi, per pair beta = inverse x products and a scan of every row; then the rank audit's host Jacobian and
// RREF per row (rank_audit_host's per_row), each g_r reduced against it; one thread.
inline ProductReport product_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                        const std::vector<ConstraintHostMatrix>& prep, const ProductAuditOpts& opts_in) {
    const ProductAuditOpts o = product_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("product_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("product_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    product_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t R = o.max_rows_per_entry;
    ProductReport rep;
    rep.chips.resize(NC);
    std::vector<size_t> e_at(NC + 1, 0);  // chip c's entries are [e_at[c], e_at[c + 1])
    std::vector<ProductVec> vecs;         // one per entry
    uint32_t need_mask = 0;
    bool need = false;
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        ProductChipStat& cs = rep.chips[c];
        product_audit_chip_block(cs, air, main[c].height, product_audit_selected(o, c));
        e_at[c] = rep.entries.size();
        if (!cs.audited || !air.width) continue;
        const uint32_t W = air.width, AW = W + 1;
        const uint64_t n = main[c].height;
        RankBasis B;
        B.reset(AW);
        std::vector<vg::Fp> x(AW);
        std::vector<uint64_t> brow;  // the rows that raised the rank
        for (uint64_t r = 0; r < n && B.rho < AW; r++) {
            x[0] = vg::Fp::one();
            for (uint32_t k = 0; k < W; k++) x[1 + k] = vg::Fp::from_canonical(main[c].data[r * W + k]);
            const uint32_t before = B.rho;
            B.insert(x);
            if (B.rho != before) brow.push_back(r);
        }
        std::vector<uint32_t> pcols;
        for (uint32_t f = 0; f < AW; f++) if (B.row_of[f] >= 0) pcols.push_back(f);
        product_audit_space(cs, pcols);
        const uint32_t rho = cs.rank, q = rho - 1;
        if (!q) continue;
        // the trace over Pi, Montgomery, row-major [n][rho]
        std::vector<vg::Fp> A((size_t)n * rho);
        for (uint64_t r = 0; r < n; r++) {
            A[r * rho] = vg::Fp::one();
            for (uint32_t t = 1; t < rho; t++) A[r * rho + t] = vg::Fp::from_canonical(main[c].data[r * W + pcols[t] - 1]);
        }
        std::vector<vg::Fp> G((size_t)rho * rho), inv;
        for (uint32_t k = 0; k < rho; k++) std::copy(A.begin() + brow[k] * rho, A.begin() + (brow[k] + 1) * rho, G.begin() + (size_t)k * rho);
        const std::vector<vg::Fp> G0 = G;
        if (!product_audit_invert(G, rho, inv)) throw std::logic_error("product_audit: the basis rows are not independent");
        std::vector<vg::Fp> y(rho), beta(rho);
        for (uint32_t ti = 1; ti <= q; ti++)
            for (uint32_t tj = ti; tj <= q; tj++) {
                for (uint32_t k = 0; k < rho; k++) y[k] = G0[(size_t)k * rho + ti] * G0[(size_t)k * rho + tj];
                for (uint32_t t = 0; t < rho; t++) {
                    vg::Fp s = vg::Fp::zero();
                    for (uint32_t k = 0; k < rho; k++) s += inv[(size_t)t * rho + k] * y[k];
                    beta[t] = s;
                }
                bool holds = true;
                for (uint64_t r = 0; r < n && holds; r++) {
                    const vg::Fp* a = &A[r * rho];
                    vg::Fp s = vg::Fp::zero();
                    for (uint32_t t = 0; t < rho; t++) s += beta[t] * a[t];
                    holds = s == a[ti] * a[tj];
                }
                if (holds) product_audit_entry(cs, (uint32_t)c, pcols, ti, tj, beta.data(), o.max_terms, rep.entries, vecs);
            }
        if (cs.relations) { need = true; if (c < 32) need_mask |= 1u << c; }
    }
    e_at[NC] = rep.entries.size();
    if (need) {
        std::vector<vg::Fp> g, x;
        auto per_row = [&](size_t c, uint64_t r, const RankBasis& B) {
            const uint32_t W = B.w;
            const uint32_t* row = main[c].data + r * W;
            for (size_t ei = e_at[c]; ei < e_at[c + 1]; ei++) {
                ProductEntry& e = rep.entries[ei];
                const ProductVec& v = vecs[ei];
                g.assign(W, vg::Fp::zero());
                for (size_t k = 0; k < v.cols.size(); k++) g[v.cols[k]] = v.neg[k];
                g[v.i] += vg::Fp::from_canonical(row[v.j]);
                g[v.j] += vg::Fp::from_canonical(row[v.i]);
                bool flat = true;
                for (uint32_t k = 0; k < W; k++) flat &= g[k].is_zero();
                if (flat) { e.flat_rows++; e.enforced++; continue; }
                x = g;
                // the basis is reduced: the coefficients can all be read before any update
                for (uint32_t p = 0; p < W; p++) {
                    if (B.row_of[p] < 0 || g[p].is_zero()) continue;
                    const vg::Fp* b = &B.rows[(size_t)B.row_of[p] * W];
                    for (uint32_t k = 0; k < W; k++) x[k] -= g[p] * b[k];
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
        ro.chip_mask = NC <= 32 ? need_mask : 0;  // chips without a relation have nothing to judge
        try {
            const RankReport rr = rank_audit_host(machine, main, prep_chips, prep, ro, per_row);
            rep.evaluations = rr.evaluations;
        } catch (const std::invalid_argument& e) {
            throw std::invalid_argument(pq_renamed(std::invalid_argument(ia_renamed(e))));
        }
    }
    product_audit_finish(rep, o);
    return rep;
}

}  // namespace vhost
