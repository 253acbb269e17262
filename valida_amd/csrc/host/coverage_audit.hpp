// Coverage audit: WHICH constraint or bus interaction detects each mutation of the mutation audit (host/mutation_audit.hpp) — per detector, does
// this witness exercise it at all, and is it ever the only thing that catches a change.
//   mutations     exactly the mutation audit's: (chip, row r, main column c, delta index j), its trace domain, its 1 to 4 distinct deltas.
//   detectors     of a chip with K constraints and M interactions: 0 .. K - 1 the constraints in assert_zero call order (the constraint audit's
//                 numbering), K .. K + M - 1 the interactions in Chip::all_interactions order.
//   kills         constraint k kills (r, c, j) when on the mutated trace it is non-zero at row r or at row (r - 1) mod n and was zero at that
//                 same row on the unmutated trace (newly failing; for n = 1 one evaluation, the cell local and next).  Interaction m kills it
//                 when its record on row r differs before and after (count 0: no record, otherwise (count, fields), canonical).
//   counts        S(r, c, j) = the detectors that kill the mutation.  Per cell (chip, detector t, column c, delta j), exact over all n rows:
//                 kills = #{r : t in S}, sole = #{r : S = {t}}, first_row = min{r : t in S}, first_sole_row = min{r : S = {t}} or 0xFFFFFFFF.
//   classes       per detector over all columns and deltas: DEAD every kills is 0; SHADOWED some kills > 0 and every sole is 0; else essential.
//   per chip and delta   detected = #{(r, c) : S not empty}, free = n w - detected (the mutation audit's free).
// "Dead" speaks of THIS witness and single-cell mutations by these deltas: it measures what the test program reaches and is no fault of the
// witness or of the AIR.  "Shadowed" does not mean removable: a constraint that is never alone against one-cell changes may be the only guard
// against a two-cell change.
// This header holds what the host and the device implementation share — options, the report and its flat word image — and the host
// implementation (plain C++, one thread, no device, no limits).  The device pass is Prover::coverage_audit (prover_audits.cpp,
// kernels/coverage_audit.hip).
#pragma once
#include "mutation_audit.hpp"

namespace vhost {

constexpr uint32_t COV_NO_ROW = 0xFFFFFFFFu;

struct CoverageAuditOpts {
    uint64_t max_cells = 8192;
    uint32_t n_deltas = 0;  // 0: the default pair {1, p - 1}
    uint32_t deltas[MA_MAX_DELTAS] = {0, 0, 0, 0};
    uint32_t max_workgroups = 0;  // device: workgroups along a chip's rows (0: the default); the report never depends on it
    uint32_t reserved[2] = {0, 0};
};

struct CoverageChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0;
    uint64_t height = 0;
    uint32_t dead_constraints = 0, shadowed_constraints = 0, dead_interactions = 0, shadowed_interactions = 0;
    uint64_t detected[MA_MAX_DELTAS] = {0, 0, 0, 0}, free_[MA_MAX_DELTAS] = {0, 0, 0, 0};
    std::vector<uint64_t> kills, sole;  // [detector * D + delta], summed over the chip's columns
};
struct CoverageCell {
    uint32_t chip = 0, detector = 0, column = 0, delta = 0;
    uint64_t kills = 0, sole = 0;
    uint32_t first_row = COV_NO_ROW, first_sole_row = COV_NO_ROW;
};
struct CoverageReport {
    std::vector<uint32_t> deltas;  // canonical
    bool truncated = false;
    uint64_t total_cells = 0;               // (chip, detector, column, delta) with kills > 0, exact even when the list is cut
    std::vector<CoverageChipStat> chips;    // one per chip of the machine
    std::vector<CoverageCell> cells;        // ascending (chip, detector, column, delta index)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image
    static constexpr uint32_t MAGIC = 0x31524b56u;  // "VKR1"
    // Flat image (include/vgpu.h documents it next to vgpu_coverage_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        const uint32_t D = (uint32_t)deltas.size();
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(D); w.push_back(truncated ? 1u : 0u);
        u64(total_cells);
        w.push_back((uint32_t)cells.size()); w.push_back((uint32_t)chips.size());
        for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) w.push_back(i < D ? deltas[i] : 0u);
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(0); u64(c.height);
            w.push_back(c.dead_constraints); w.push_back(c.shadowed_constraints); w.push_back(c.dead_interactions); w.push_back(c.shadowed_interactions);
            for (uint32_t i = 0; i < D; i++) { u64(c.detected[i]); u64(c.free_[i]); }
            for (size_t k = 0; k < c.kills.size(); k++) { u64(c.kills[k]); u64(c.sole[k]); }
        }
        for (auto& e : cells) {
            w.push_back(e.chip); w.push_back(e.detector); w.push_back(e.column); w.push_back(e.delta);
            u64(e.kills); u64(e.sole);
            w.push_back(e.first_row); w.push_back(e.first_sole_row);
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline CoverageAuditOpts coverage_audit_checked_opts(const CoverageAuditOpts& in) {
    CoverageAuditOpts o = in;
    if (o.reserved[0] != 0 || o.reserved[1] != 0) throw std::invalid_argument("coverage_audit: the reserved fields of the options must be zero");
    if (o.max_cells == 0) o.max_cells = 8192;
    if (o.max_cells > (1ull << 24)) throw std::invalid_argument("coverage_audit: max_cells is at most 2^24");
    if (o.n_deltas == 0) { o.n_deltas = 2; o.deltas[0] = 1; o.deltas[1] = vg::P - 1; o.deltas[2] = o.deltas[3] = 0; }
    if (o.n_deltas > MA_MAX_DELTAS) throw std::invalid_argument("coverage_audit: at most " + std::to_string(MA_MAX_DELTAS) + " deltas (got " + std::to_string(o.n_deltas) + ")");
    for (uint32_t i = 0; i < o.n_deltas; i++) {
        if (o.deltas[i] == 0 || o.deltas[i] >= vg::P) throw std::invalid_argument("coverage_audit: a delta must be a canonical value in 1..p-1 (delta " + std::to_string(i) + ": " + std::to_string(o.deltas[i]) + ")");
        for (uint32_t j = 0; j < i; j++)
            if (o.deltas[j] == o.deltas[i]) throw std::invalid_argument("coverage_audit: the deltas must be distinct (" + std::to_string(o.deltas[i]) + " is repeated)");
    }
    return o;
}

// The mutation audit's shape checks under this audit's name
inline void coverage_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                std::vector<int>& prep_slot) {
    try {
        mutation_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what(), from = "mutation_audit: ";
        throw std::invalid_argument(m.compare(0, from.size(), from) == 0 ? "coverage_audit: " + m.substr(from.size()) : m);
    }
}

// The classes of a chip's detectors and its free cells from its sums (kills, sole, detected filled in)
inline void coverage_classify(CoverageChipStat& cs, uint32_t D) {
    cs.dead_constraints = cs.shadowed_constraints = cs.dead_interactions = cs.shadowed_interactions = 0;
    for (uint32_t t = 0; t < cs.n_constraints + cs.n_interactions; t++) {
        uint64_t k = 0, s = 0;
        for (uint32_t i = 0; i < D; i++) { k += cs.kills[(size_t)t * D + i]; s += cs.sole[(size_t)t * D + i]; }  // sums of counts of rows: no overflow below 2^64
        const bool constraint = t < cs.n_constraints;
        if (!k) (constraint ? cs.dead_constraints : cs.dead_interactions)++;
        else if (!s) (constraint ? cs.shadowed_constraints : cs.shadowed_interactions)++;
    }
    for (uint32_t i = 0; i < MA_MAX_DELTAS; i++) cs.free_[i] = i < D ? cs.height * cs.width - cs.detected[i] : 0;
}

// The contract on the host: the chip's Program interpreted on the mutated rows, the interactions evaluated before and after; one thread.
inline CoverageReport coverage_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                          const std::vector<ConstraintHostMatrix>& prep, const CoverageAuditOpts& opts_in) {
    const CoverageAuditOpts o = coverage_audit_checked_opts(opts_in);
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("coverage_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("coverage_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    coverage_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NC = machine.airs.size();
    const uint32_t D = o.n_deltas;
    CoverageReport rep;
    rep.deltas.assign(o.deltas, o.deltas + D);
    rep.chips.resize(NC);
    const vg::Fp one = vg::Fp::one(), zero = vg::Fp::zero();
    vg::Fp dm[MA_MAX_DELTAS];
    for (uint32_t i = 0; i < D; i++) dm[i] = vg::Fp::from_canonical(o.deltas[i]);
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        const vair::Program& p = air.program;
        const uint32_t K = p.num_asserts, W = air.width, PW = air.prep_width, M = (uint32_t)air.interactions.size(), TD = K + M;
        const ConstraintHostMatrix& mm = main[c];
        const uint64_t n = mm.height;
        CoverageChipStat& cs = rep.chips[c];
        cs.width = W; cs.n_constraints = K; cs.n_interactions = M; cs.height = n;
        cs.kills.assign((size_t)TD * D, 0); cs.sole.assign((size_t)TD * D, 0);
        rep.evaluations += ma_evaluations(air, n, D);
        // the chip's cells [(t * W + column) * D + delta]
        std::vector<uint64_t> kills((size_t)TD * W * D, 0), sole((size_t)TD * W * D, 0);
        std::vector<uint32_t> first((size_t)TD * W * D, COV_NO_ROW), first_sole((size_t)TD * W * D, COV_NO_ROW);
        const ConstraintHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        const std::vector<uint32_t> flags = ma_column_flags(air);
        std::vector<vg::Fp> regs(p.num_regs ? p.num_regs : 1);
        // Air::eval at row q with the given local / next rows (Montgomery): fail[k] = constraint k is non-zero
        auto eval = [&](uint64_t q, const vg::Fp* ml, const vg::Fp* mn, const vg::Fp* pl, const vg::Fp* pn, uint8_t* fail) {
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
                    case vair::OP_ASSERT: fail[k++] = regs[in.a].is_zero() ? 0 : 1; break;
                    default: break;
                }
            }
        };
        std::vector<vg::Fp> mont((size_t)n * W), pmont(pm ? (size_t)n * PW : 0);
        for (size_t i = 0; i < mont.size(); i++) mont[i] = vg::Fp::from_canonical(mm.data[i]);
        for (size_t i = 0; i < pmont.size(); i++) pmont[i] = vg::Fp::from_canonical(pm->data[i]);
        auto prow = [&](uint64_t q) -> const vg::Fp* { return pm ? pmont.data() + q * PW : nullptr; };
        std::vector<uint8_t> base((size_t)n * K, 0), fail(K ? K : 1);
        for (uint64_t q = 0; K && q < n; q++) { const uint64_t nx = (q + 1) & (n - 1); eval(q, mont.data() + q * W, mont.data() + nx * W, prow(q), prow(nx), base.data() + q * K); }
        auto vcol = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* pr) {
            uint64_t acc = v.constant % vg::P;
            for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? pr : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
            return (uint32_t)acc;
        };
        std::vector<vg::Fp> cur(W ? W : 1);
        std::vector<uint32_t> mut(W ? W : 1);
        std::vector<uint8_t> S(TD ? TD : 1);
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t rp = (r + n - 1) & (n - 1), nx = (r + 1) & (n - 1);
            const uint32_t* crow = mm.data + r * W;
            const uint32_t* cprow = pm ? pm->data + r * PW : nullptr;
            for (uint32_t col = 0; col < W; col++) cur[col] = mont[r * W + col];
            for (uint32_t col = 0; col < W; col++) {
                const uint32_t fl = flags[col];
                for (uint32_t i = 0; i < D; i++) {
                    std::fill(S.begin(), S.end(), 0);
                    if (K && (fl & (MA_COL_LOCAL | MA_COL_NEXT))) {
                        cur[col] = mont[r * W + col] + dm[i];
                        auto newly = [&](uint64_t q) { for (uint32_t k = 0; k < K; k++) if (fail[k] && !base[q * K + k]) S[k] = 1; };
                        if (n == 1) { eval(0, cur.data(), cur.data(), prow(0), prow(0), fail.data()); newly(0); }
                        else {
                            if (fl & MA_COL_LOCAL) { eval(r, cur.data(), mont.data() + nx * W, prow(r), prow(nx), fail.data()); newly(r); }
                            if (fl & MA_COL_NEXT) { eval(rp, mont.data() + rp * W, cur.data(), prow(rp), prow(r), fail.data()); newly(rp); }
                        }
                        cur[col] = mont[r * W + col];
                    }
                    if (fl & MA_COL_BUS) {
                        for (uint32_t k = 0; k < W; k++) mut[k] = crow[k];
                        mut[col] = (uint32_t)(((uint64_t)crow[col] % vg::P + o.deltas[i]) % vg::P);
                        for (uint32_t m = 0; m < M; m++) {
                            const vair::Interaction& it = air.interactions[m];
                            const uint32_t c0 = vcol(it.count, crow, cprow), c1 = vcol(it.count, mut.data(), cprow);
                            bool differs = c0 != c1;
                            if (!differs && c0)
                                for (auto& f : it.fields)
                                    if (vcol(f, crow, cprow) != vcol(f, mut.data(), cprow)) { differs = true; break; }
                            if (differs) S[K + m] = 1;
                        }
                    }
                    uint32_t size = 0;
                    for (uint32_t t = 0; t < TD; t++) size += S[t];
                    if (!size) continue;
                    cs.detected[i]++;
                    for (uint32_t t = 0; t < TD; t++) {
                        if (!S[t]) continue;
                        const size_t at = ((size_t)t * W + col) * D + i;
                        if (!kills[at]++) first[at] = (uint32_t)r;
                        if (size == 1 && !sole[at]++) first_sole[at] = (uint32_t)r;
                    }
                }
            }
        }
        for (uint32_t t = 0; t < TD; t++)
            for (uint32_t col = 0; col < W; col++)
                for (uint32_t i = 0; i < D; i++) {
                    const size_t at = ((size_t)t * W + col) * D + i;
                    if (!kills[at]) continue;
                    cs.kills[(size_t)t * D + i] += kills[at]; cs.sole[(size_t)t * D + i] += sole[at];
                    rep.total_cells++;
                    if (rep.cells.size() < o.max_cells) {
                        CoverageCell e;
                        e.chip = (uint32_t)c; e.detector = t; e.column = col; e.delta = i; e.kills = kills[at]; e.sole = sole[at]; e.first_row = first[at]; e.first_sole_row = first_sole[at];
                        rep.cells.push_back(e);
                    }
                }
        coverage_classify(cs, D);
    }
    rep.truncated = rep.total_cells > rep.cells.size();
    return rep;
}

}  // namespace vhost
