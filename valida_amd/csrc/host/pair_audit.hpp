// Pair audit: WHICH TWO cells of one row of a witness could be changed together without any AIR constraint or bus noticing although changing
// one of them alone is noticed — the next order of slack after the mutation audit (host/mutation_audit.hpp), whose rules it applies unchanged.
//   pair mutation  chip h with main matrix M (height n, width w), a row r, two main columns c1 < c2 and a delta pair q = i * D + j over the
//                  option's deltas: M'' = M except M''[r][c1] = M[r][c1] + d_i and M''[r][c2] = M[r][c2] + d_j mod p.  Both cells are on the
//                  same row; preprocessed columns are never mutated.
//   detected       the mutation audit's two rules on M'': AIR-detected when a constraint is non-zero at row r or (r - 1) mod n that was zero at
//                  that row on M (n = 1: one evaluation, both cells seen as local and as next); bus-detected when the record of some
//                  interaction of row r differs (count 0 is no record).
//   counts         per (chip, c1, c2, q), exact over all n rows: `free` = rows where the pair mutation is neither AIR- nor bus-detected;
//                  `compensated` = free rows where at least one of the single mutations (r, c1, d_i), (r, c2, d_j) IS detected by the mutation
//                  audit's rules.  Compensated rows are the finding; the other free rows are already in the mutation report.
//   coupled        a pair is coupled when some constraint of the chip's Program reads both columns (in any role: the registers' dependences
//                  are followed through the program), or some single interaction's virtual columns (count or fields) reference both, or n = 1.
//                  For an uncoupled pair no constraint and no record sees both changes, so the detectors of the pair mutation are the union of
//                  the singles' detectors: compensated = 0 and free = rows where both singles are free.  Uncoupled pairs are not evaluated.
// It covers same-row pairs only; cross-row pairs and triples are not looked for.  It is a statement about THIS witness, not a soundness proof.
// This header holds what the host and the device implementation share — options, coupling sets, bus masks, the report and its word image —
// and the host implementation (plain C++, one thread, no limits).  The device pass is Prover::pair_audit (prover_audits.cpp, kernels/pair_audit.hip).
#pragma once
#include "mutation_audit.hpp"

namespace vhost {

struct PairAuditOpts {
    uint64_t max_entries = 1024;
    uint32_t max_rows_per_entry = 4;
    uint32_t n_deltas = 0;  // 0: the default pair {1, p - 1}
    uint32_t deltas[MA_MAX_DELTAS] = {0, 0, 0, 0};
    uint32_t chip_mask = 0;  // bit h: audit chip h; 0: all chips
    uint32_t reserved = 0;
};

struct PairChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t coupled = 0, slack = 0;  // coupled pairs; pairs with compensated > 0 for some q
    uint64_t free_[MA_MAX_DELTAS * MA_MAX_DELTAS] = {}, compensated[MA_MAX_DELTAS * MA_MAX_DELTAS] = {};  // per q, sums over all the chip's pairs
};
struct PairEntry {
    uint32_t chip = 0, c1 = 0, c2 = 0, q = 0;
    uint64_t free_ = 0, compensated = 0;
    std::vector<uint32_t> rows;  // the first max_rows_per_entry compensated rows, ascending
};
struct PairReport {
    std::vector<uint32_t> deltas;  // canonical
    bool truncated = false;
    uint64_t total_entries = 0;  // (chip, c1, c2, q) with compensated > 0, exact even when the list is cut
    std::vector<PairChipStat> chips;
    std::vector<PairEntry> entries;  // ascending (chip, c1, c2, q)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31525056u;  // "VPR1"
    // Flat image (include/vgpu.h documents it next to vgpu_pair_report_words)
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
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height); w.push_back(c.coupled); w.push_back(c.slack);
            for (uint32_t q = 0; q < D * D; q++) { u64(c.free_[q]); u64(c.compensated[q]); }
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.c1); w.push_back(e.c2); w.push_back(e.q); w.push_back((uint32_t)e.rows.size()); w.push_back(0);
            u64(e.free_); u64(e.compensated);
            for (uint32_t r : e.rows) w.push_back(r);
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline PairAuditOpts pair_audit_checked_opts(const PairAuditOpts& in, size_t n_chips) {
    if (in.reserved != 0) throw std::invalid_argument("pair_audit: the reserved field of the options must be zero");
    MutationAuditOpts m;
    m.max_entries = in.max_entries; m.max_rows_per_entry = in.max_rows_per_entry; m.n_deltas = in.n_deltas;
    for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) m.deltas[i] = in.deltas[i];
    try {
        m = mutation_audit_checked_opts(m);  // the limits are the mutation audit's
    } catch (const std::invalid_argument& e) {
        const std::string s = e.what(), from = "mutation_audit: ";
        throw std::invalid_argument(s.compare(0, from.size(), from) == 0 ? "pair_audit: " + s.substr(from.size()) : s);
    }
    PairAuditOpts o = in;
    o.max_entries = m.max_entries; o.max_rows_per_entry = m.max_rows_per_entry; o.n_deltas = m.n_deltas;
    for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) o.deltas[i] = m.deltas[i];
    if (n_chips < 32 && (o.chip_mask >> n_chips) != 0) throw std::invalid_argument("pair_audit: chip_mask names a chip the machine does not have (" + std::to_string(n_chips) + " chips)");
    if (n_chips > 32 && o.chip_mask != 0) throw std::invalid_argument("pair_audit: chip_mask selects among at most 32 chips");
    return o;
}
inline bool pair_audit_selected(const PairAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

inline void pair_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                            std::vector<int>& prep_slot) {
    try {
        mutation_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what(), from = "mutation_audit: ";
        throw std::invalid_argument(m.compare(0, from.size(), from) == 0 ? "pair_audit: " + m.substr(from.size()) : m);
    }
}

// The coupling sets (beside ma_column_flags): byte [c1 * width + c2], c1 < c2, is 1 when the pair is coupled.  A register's dependence set is
// the union of the main columns loaded into what it was computed from; a constraint reads the set of its asserted register.
inline std::vector<uint8_t> pa_coupling(const AirDesc& a, uint64_t n) {
    const size_t w = a.width;
    std::vector<uint8_t> cp(w * w ? w * w : 1, 0);
    auto couple = [&](const std::vector<uint32_t>& cols) {
        for (size_t x = 0; x < cols.size(); x++)
            for (size_t y = x + 1; y < cols.size(); y++) cp[(size_t)cols[x] * w + cols[y]] = 1;
    };
    if (n == 1) {
        for (size_t x = 0; x < w; x++)
            for (size_t y = x + 1; y < w; y++) cp[x * w + y] = 1;
        return cp;
    }
    const size_t WW = (w + 63) / 64;
    std::vector<std::vector<uint64_t>> dep(a.program.num_regs ? a.program.num_regs : 1, std::vector<uint64_t>(WW ? WW : 1, 0));
    std::vector<uint64_t> tmp(WW ? WW : 1);
    std::vector<uint32_t> cols;
    for (const vair::Instr& in : a.program.instrs) {
        switch (in.op) {
            case vair::OP_LOAD_MAIN:
                std::fill(dep[in.dst].begin(), dep[in.dst].end(), 0);
                if (in.a < w) dep[in.dst][in.a >> 6] |= 1ull << (in.a & 63);
                break;
            case vair::OP_ADD: case vair::OP_SUB: case vair::OP_MUL:
                for (size_t k = 0; k < WW; k++) tmp[k] = dep[in.a][k] | dep[in.b][k];
                dep[in.dst] = tmp;
                break;
            case vair::OP_NEG: tmp = dep[in.a]; dep[in.dst] = tmp; break;
            case vair::OP_ASSERT:
                cols.clear();
                for (uint32_t c = 0; c < w; c++)
                    if ((dep[in.a][c >> 6] >> (c & 63)) & 1ull) cols.push_back(c);
                couple(cols);
                break;
            case vair::OP_CONST: case vair::OP_LOAD_PREP: case vair::OP_SEL_FIRST: case vair::OP_SEL_LAST: case vair::OP_SEL_TRANS:
                std::fill(dep[in.dst].begin(), dep[in.dst].end(), 0);
                break;
            default: break;
        }
    }
    for (auto& it : a.interactions) {
        std::vector<uint8_t> seen(w ? w : 1, 0);
        auto mark = [&](const vair::VirtualCol& v) {
            for (auto& t : v.terms)
                if (!t.preprocessed && t.col >= 0 && (size_t)t.col < w) seen[(size_t)t.col] = 1;
        };
        mark(it.count);
        for (auto& f : it.fields) mark(f);
        cols.clear();
        for (uint32_t c = 0; c < w; c++)
            if (seen[c]) cols.push_back(c);
        couple(cols);
    }
    return cp;
}
// The coupled pairs in ascending (c1, c2) order, packed c1 | c2 << 16 (both passes take chips of up to 65535 columns by this packing; the device pass stops at 4096, kernels/pair_audit.hip)
inline std::vector<uint32_t> pa_coupled_pairs(const AirDesc& a, uint64_t n) {
    const std::vector<uint8_t> cp = pa_coupling(a, n);
    std::vector<uint32_t> out;
    for (uint32_t x = 0; x < a.width; x++)
        for (uint32_t y = x + 1; y < a.width; y++)
            if (cp[(size_t)x * a.width + y]) out.push_back(x | (y << 16));
    return out;
}

// The bus rule of a pair mutation from the affine weights (extends ma_bus_masks): adding d_i to c1 and d_j to c2 changes a virtual column by
// w1 d_i + w2 d_j, with w1 / w2 the sums of the columns' weights in it — it changes iff that is non-zero mod p, on every row alike, and a sum
// that IS zero while w1 d_i or w2 d_j is not is exactly a compensation.  Per (pair, q) two masks over the interactions: [2 (p DD + q)] those
// whose COUNT changes, [.. + 1] those with a FIELD that changes.  Only for at most 32 interactions (`ok`).
inline std::vector<uint32_t> pa_bus_masks(const AirDesc& a, const std::vector<uint32_t>& pairs, const uint32_t* deltas, uint32_t D, bool& ok) {
    const uint32_t DD = D * D;
    std::vector<uint32_t> m(2 * pairs.size() * DD + 1, 0);
    ok = a.interactions.size() <= 32;
    if (!ok) return m;
    auto wsum = [&](const vair::VirtualCol& v, uint32_t c) {
        uint64_t s = 0;
        for (auto& t : v.terms)
            if (!t.preprocessed && t.col >= 0 && (uint32_t)t.col == c) s = (s + t.weight % vg::P) % vg::P;
        return s;
    };
    for (size_t p = 0; p < pairs.size(); p++) {
        const uint32_t c1 = pairs[p] & 0xffffu, c2 = pairs[p] >> 16;
        for (size_t k = 0; k < a.interactions.size(); k++) {
            auto changed = [&](const vair::VirtualCol& v, uint32_t which) {
                const uint64_t w1 = wsum(v, c1), w2 = wsum(v, c2);
                if (!w1 && !w2) return;
                for (uint32_t q = 0; q < DD; q++)
                    if ((w1 * deltas[q / D] % vg::P + w2 * deltas[q % D] % vg::P) % vg::P) m[2 * (p * DD + q) + which] |= 1u << k;
            };
            changed(a.interactions[k].count, 0);
            for (auto& f : a.interactions[k].fields) changed(f, 1);
        }
    }
    return m;
}

// Air::eval row evaluations of the device pass of one chip whose coupled pairs are cut into `slices` slices of `pps` pairs: per slice the
// baselines, the singles of the columns its pairs name (slice 0: of all columns) and its pairs, each at the rows the column flags leave.
inline double pa_device_evaluations(const AirDesc& a, uint64_t n, uint32_t D, const std::vector<uint32_t>& pairs, uint32_t pps, uint32_t slices) {
    if (!a.program.num_asserts) return 0;
    const std::vector<uint32_t> fl = ma_column_flags(a);
    auto evals = [&](uint32_t f) -> uint64_t { return n == 1 ? ((f & 3u) ? 1 : 0) : ((f & MA_COL_LOCAL) ? 1 : 0) + ((f & MA_COL_NEXT) ? 1 : 0); };
    uint64_t per_row = 0;
    std::vector<uint8_t> seen(a.width ? a.width : 1);
    for (uint32_t y = 0; y < slices; y++) {
        per_row += n == 1 ? 1 : 2;
        std::fill(seen.begin(), seen.end(), y == 0 ? 1 : 0);
        const size_t lo = std::min<size_t>((size_t)y * pps, pairs.size()), hi = std::min<size_t>(lo + pps, pairs.size());
        for (size_t p = lo; p < hi; p++) {
            seen[pairs[p] & 0xffffu] = seen[pairs[p] >> 16] = 1;
            per_row += evals(fl[pairs[p] & 0xffffu] | fl[pairs[p] >> 16]) * D * D;
        }
        for (uint32_t c = 0; c < a.width; c++)
            if (seen[c]) per_row += evals(fl[c]) * D;
    }
    return (double)n * (double)per_row;
}

// chips[].coupled / slack / sums, total_entries, truncated and the entries (without rows) from per-chip counts: pairs[c] the coupled pairs,
// counts[c][(p * DD + q) * 2 + {free, compensated}], uncoupled_free[c][q] the sum of `free` over the chip's uncoupled pairs.
inline void pair_audit_finish(PairReport& r, const std::vector<std::vector<uint32_t>>& pairs, const std::vector<std::vector<uint64_t>>& counts,
                              const std::vector<std::vector<uint64_t>>& uncoupled_free, const PairAuditOpts& o) {
    const uint32_t D = o.n_deltas, DD = D * D;
    r.deltas.assign(o.deltas, o.deltas + D);
    r.total_entries = 0;
    r.entries.clear();
    for (size_t c = 0; c < pairs.size(); c++) {
        PairChipStat& cs = r.chips[c];
        cs.coupled = cs.slack = 0;
        for (uint32_t q = 0; q < MA_MAX_DELTAS * MA_MAX_DELTAS; q++) cs.free_[q] = cs.compensated[q] = 0;
        if (!cs.audited) continue;
        cs.coupled = (uint32_t)pairs[c].size();
        for (uint32_t q = 0; q < DD; q++) cs.free_[q] = uncoupled_free[c][q];
        for (size_t p = 0; p < pairs[c].size(); p++) {
            bool slack = false;
            for (uint32_t q = 0; q < DD; q++) {
                const uint64_t* k = &counts[c][(p * DD + q) * 2];
                cs.free_[q] += k[0]; cs.compensated[q] += k[1];
                if (!k[1]) continue;
                slack = true;
                r.total_entries++;
                if (r.entries.size() < o.max_entries) {
                    PairEntry e;
                    e.chip = (uint32_t)c; e.c1 = pairs[c][p] & 0xffffu; e.c2 = pairs[c][p] >> 16; e.q = q; e.free_ = k[0]; e.compensated = k[1];
                    r.entries.push_back(std::move(e));
                }
            }
            if (slack) cs.slack++;
        }
    }
    r.truncated = r.total_entries > r.entries.size();
}

// The contract on the host: the chip's Program interpreted on the mutated rows, the interactions evaluated before and after; one thread.
inline PairReport pair_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                  const std::vector<ConstraintHostMatrix>& prep, const PairAuditOpts& opts_in) {
    const PairAuditOpts o = pair_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("pair_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("pair_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    pair_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t D = o.n_deltas, DD = D * D, R = o.max_rows_per_entry;
    PairReport rep;
    rep.chips.resize(NC);
    std::vector<std::vector<uint32_t>> pairs(NC);
    std::vector<std::vector<uint64_t>> counts(NC), ufree(NC);
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
        PairChipStat& cs = rep.chips[c];
        cs.width = W; cs.n_constraints = K; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = n;
        cs.audited = pair_audit_selected(o, c) ? 1u : 0u;
        ufree[c].assign(DD, 0);
        if (!cs.audited) continue;
        if (W > 65535) throw std::invalid_argument("pair_audit: chip " + air.name + " has more than 65535 columns");
        const std::vector<uint8_t> cp = pa_coupling(air, n);
        pairs[c] = pa_coupled_pairs(air, n);
        std::vector<uint32_t> pair_at((size_t)W * W ? (size_t)W * W : 1, 0);
        for (size_t k = 0; k < pairs[c].size(); k++) pair_at[(size_t)(pairs[c][k] & 0xffffu) * W + (pairs[c][k] >> 16)] = (uint32_t)k;
        counts[c].assign(pairs[c].size() * DD * 2, 0);
        first[c].resize(pairs[c].size() * DD);
        const ConstraintHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        const std::vector<uint32_t> flags = ma_column_flags(air);
        const size_t MW = (K + 63) / 64;
        std::vector<vg::Fp> regs(p.num_regs ? p.num_regs : 1);
        auto eval = [&](uint64_t q, const vg::Fp* ml, const vg::Fp* mn, const vg::Fp* pl, const vg::Fp* pn, const uint64_t* base, uint64_t* out) -> bool {
            uint32_t k = 0;
            rep.evaluations += 1;
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
        std::vector<uint8_t> det1((size_t)W * D ? (size_t)W * D : 1);
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t rp = (r + n - 1) & (n - 1), nx = (r + 1) & (n - 1);
            const uint32_t* crow = mm.data + r * W;
            const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
            for (uint32_t col = 0; col < W; col++) { cur[col] = mont[r * W + col]; mut[col] = crow[col]; }
            // detected(fl) of the row as `cur` (AIR) and `mut` (bus) hold it; fl = the union of the mutated columns' flags
            auto detected = [&](uint32_t fl) {
                bool det = false;
                if (K && (fl & (MA_COL_LOCAL | MA_COL_NEXT))) {
                    if (n == 1) det = eval(0, cur.data(), cur.data(), prow(0), prow(0), base.data(), nullptr);
                    else {
                        if (fl & MA_COL_LOCAL) det = eval(r, cur.data(), mont.data() + nx * W, prow(r), prow(nx), base.data() + r * MW, nullptr);
                        if (!det && (fl & MA_COL_NEXT)) det = eval(rp, mont.data() + rp * W, cur.data(), prow(rp), prow(r), base.data() + rp * MW, nullptr);
                    }
                }
                if (!det && (fl & MA_COL_BUS))
                    for (auto& it : air.interactions) {
                        const uint32_t c0 = vcol(it.count, crow, cprow), c1 = vcol(it.count, mut.data(), cprow);
                        if (c0 != c1) { det = true; break; }
                        if (!c0) continue;
                        for (auto& f : it.fields)
                            if (vcol(f, crow, cprow) != vcol(f, mut.data(), cprow)) { det = true; break; }
                        if (det) break;
                    }
                return det;
            };
            auto set = [&](uint32_t col, uint32_t i) { cur[col] = mont[r * W + col] + dm[i]; mut[col] = (uint32_t)(((uint64_t)crow[col] % vg::P + o.deltas[i]) % vg::P); };
            auto reset = [&](uint32_t col) { cur[col] = mont[r * W + col]; mut[col] = crow[col]; };
            for (uint32_t col = 0; col < W; col++)
                for (uint32_t i = 0; i < D; i++) { set(col, i); det1[(size_t)col * D + i] = detected(flags[col]) ? 1 : 0; reset(col); }
            for (uint32_t c1 = 0; c1 < W; c1++)
                for (uint32_t c2 = c1 + 1; c2 < W; c2++) {
                    if (!cp[(size_t)c1 * W + c2]) {
                        for (uint32_t q = 0; q < DD; q++)
                            if (!det1[(size_t)c1 * D + q / D] && !det1[(size_t)c2 * D + q % D]) ufree[c][q]++;
                        continue;
                    }
                    const size_t pi = pair_at[(size_t)c1 * W + c2];
                    for (uint32_t q = 0; q < DD; q++) {
                        set(c1, q / D); set(c2, q % D);
                        const bool det = detected(flags[c1] | flags[c2]);
                        reset(c1); reset(c2);
                        if (det) continue;
                        uint64_t* k = &counts[c][(pi * DD + q) * 2];
                        k[0]++;
                        if (det1[(size_t)c1 * D + q / D] || det1[(size_t)c2 * D + q % D])
                            if (k[1]++ < R) first[c][pi * DD + q].push_back((uint32_t)r);
                    }
                }
        }
    }
    pair_audit_finish(rep, pairs, counts, ufree, o);
    for (auto& e : rep.entries) {
        const auto& pl = pairs[e.chip];
        const size_t pi = (size_t)(std::lower_bound(pl.begin(), pl.end(), e.c1 | (e.c2 << 16), [](uint32_t a, uint32_t b) {
                                       return ((uint64_t)(a & 0xffffu) << 16 | (a >> 16)) < ((uint64_t)(b & 0xffffu) << 16 | (b >> 16)); }) - pl.begin());
        e.rows = std::move(first[e.chip][pi * o.n_deltas * o.n_deltas + e.q]);
    }
    return rep;
}

}  // namespace vhost
