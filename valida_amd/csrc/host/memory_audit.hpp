// Memory audit: is the memory table of a witness a memory?  The reference's memory AIR is commented out (memory/src/stark.rs:22-78) and so
// are compute_address_diffs and insert_dummy_reads (memory/src/lib.rs:160-184): nothing in the proof system requires a read to return the last
// value written to its address, and a wrong value planted consistently on both sides of the memory bus passes every other audit.  This audit
// replays the receives of one bus as a memory and names the records that break it.
//
// Contract (include/vgpu.h, "Memory audit", states it for the C ABI):
//   inputs    what vgpu_prove and the audits take.  The audited bus is global bus 2 by default (bus_is_global, bus_index name another).  Every
//             RECEIVE on it is read through its vcols and must have exactly 8 fields (is_read, clk, addr, is_static_initial, v0, v1, v2, v3),
//             the shape of memory/src/lib.rs:216-233.
//   records   a SLOT is (chip, receive, row), LIVE iff its count != 0 there; values canonical.  READ iff is_read == 1, otherwise a WRITE; STATIC
//             iff is_static_initial == 1.
//   order     live records by key = addr << 32 | clk << 1 | !static, ties in seq order = lexicographic (chip, row, interaction): a stable sort
//             of the slots enumerated in seq order.  Inside one (addr, clk) the trace's own order decides (same_cycle_pairs counts the
//             verdicts that rest on it).
//   state     per address the last WRITE before a record in that order, or none; an address nobody has written reads as 0 (read_or_init,
//             memory/src/lib.rs:107-120).
//   findings  at most one kind per live record, the lowest applicable: 1 MALFORMED (reason bit 0 count != 1, bit 1 is_read not 0 / 1, bit 2
//             is_static not 0 / 1, bit 3 static with is_read == 1 or clk != 0, bit 4 a value field >= 256; the record still takes its place and
//             acts by the rule above), 2 DUPLICATE_STATIC (a static record whose predecessor is a static record of the same address), 3
//             STALE_READ (a read whose four value fields differ from the last write's, as field elements), 4 UNINIT_READ (a read with no
//             write before it and a non-zero value).
//   counters  exact: live, reads, writes, statics, addresses, min / max addr, max clk, uninit_zero_reads, same_cycle_pairs (a position whose
//             predecessor has the same (addr, clk), both non-static, one of them a write), max_clk_gap (successive records of one address),
//             dummy_reads_clk (sum of gap / L over same-address successors with gap > L), dummy_reads_addr (the same over successive
//             different addresses), L = live records; layout_descents (rows r with rows r, r + 1 of one chip and receive both live and
//             key(r) > key(r + 1)) and the first such (chip, row); one count per kind.
//   list      the first max_findings findings in ascending order position (default 64, at most 2^20, 0 lists nothing).
// This header holds the plan, the report with its image "VMM1" and the host twin (plain C++, one thread, std::stable_sort, no limits).  The
// device pass is Prover::memory_audit (prover_audits.cpp, kernels/memory_audit.hip).
#pragma once
#include "bus_audit.hpp"

namespace vhost {

struct MemoryAuditOpts {
    uint32_t max_findings = 64;
    uint32_t bus_is_global = 1, bus_index = 2;
    uint32_t reserved = 0;
};

enum : uint32_t { MM_MALFORMED = 1, MM_DUPLICATE_STATIC = 2, MM_STALE_READ = 3, MM_UNINIT_READ = 4 };
constexpr uint32_t MM_FIELDS = 8, MM_NONE = 0xffffffffu;

struct MemoryFinding {
    uint32_t kind = 0, reason = 0, chip = 0, interaction = 0, row = 0, addr = 0, clk = 0;
    uint32_t value[4] = {0, 0, 0, 0}, expected[4] = {0, 0, 0, 0};
    uint32_t w_chip = MM_NONE, w_interaction = MM_NONE, w_row = MM_NONE;  // the last write, all ones when there is none
    uint32_t position = 0;                                                // in the order
};

struct MemoryReport {
    uint32_t is_global = 1, bus_index = 2, max_findings = 64;
    std::vector<std::pair<uint32_t, uint32_t>> receives;  // (chip, interaction), seq order
    uint64_t slots = 0, live = 0, reads = 0, writes = 0, statics = 0, addresses = 0;
    uint32_t min_addr = 0, max_addr = 0, max_clk = 0, max_clk_gap = 0;
    uint64_t uninit_zero_reads = 0, same_cycle_pairs = 0, dummy_reads_clk = 0, dummy_reads_addr = 0, layout_descents = 0;
    uint32_t descent_chip = MM_NONE, descent_row = MM_NONE;
    uint64_t total_findings = 0, kinds[4] = {0, 0, 0, 0};
    std::vector<MemoryFinding> findings;
    double device_ms = 0, host_ms = 0, evaluations = 0;  // evaluations: slots evaluated
    static constexpr uint32_t MAGIC = 0x314d4d56u;        // "VMM1"
    static constexpr uint32_t HEADER = 48, FINDING_WORDS = 20;
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0); w.push_back(is_global); w.push_back(bus_index);
        w.push_back((uint32_t)receives.size()); w.push_back(total_findings > findings.size() ? 1u : 0u); w.push_back((uint32_t)findings.size()); w.push_back(max_findings);
        u64(slots); u64(live); u64(reads); u64(writes); u64(statics); u64(addresses);
        w.push_back(min_addr); w.push_back(max_addr); w.push_back(max_clk); w.push_back(max_clk_gap);
        u64(uninit_zero_reads); u64(same_cycle_pairs); u64(dummy_reads_clk); u64(dummy_reads_addr);
        u64(layout_descents); w.push_back(descent_chip); w.push_back(descent_row);
        u64(total_findings);
        for (int k = 0; k < 4; k++) u64(kinds[k]);
        u64(0);
        for (auto& r : receives) { w.push_back(r.first); w.push_back(r.second); }
        for (auto& f : findings) {
            w.push_back(f.kind); w.push_back(f.reason); w.push_back(f.chip); w.push_back(f.interaction); w.push_back(f.row); w.push_back(f.addr); w.push_back(f.clk);
            for (int k = 0; k < 4; k++) w.push_back(f.value[k]);
            for (int k = 0; k < 4; k++) w.push_back(f.expected[k]);
            w.push_back(f.w_chip); w.push_back(f.w_interaction); w.push_back(f.w_row); w.push_back(f.position); w.push_back(0);
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline MemoryAuditOpts memory_audit_checked_opts(const MemoryAuditOpts& o) {
    if (o.max_findings > (1u << 20)) throw std::invalid_argument("memory_audit: max_findings is at most 2^20");
    if (o.bus_is_global > 1) throw std::invalid_argument("memory_audit: bus_is_global is 0 or 1");
    if (o.reserved) throw std::invalid_argument("memory_audit: reserved must be zero");
    return o;
}

// The slots: per chip its receives on the audited bus (ascending interaction); slot = first_slot(chip) + row * R(chip) + k: integer order is
// seq order.
struct MemoryPlan {
    struct Chip { uint64_t first_slot = 0, height = 0; std::vector<uint32_t> receives; };
    std::vector<Chip> chips;
    uint64_t n_slots = 0;
    void decode(uint64_t slot, uint32_t& chip, uint32_t& interaction, uint32_t& row) const {
        size_t c = 0;
        for (size_t i = 0; i < chips.size(); i++)
            if (!chips[i].receives.empty() && chips[i].first_slot <= slot) c = i;
        const uint64_t off = slot - chips[c].first_slot, R = chips[c].receives.size();
        chip = (uint32_t)c; row = (uint32_t)(off / R); interaction = chips[c].receives[(size_t)(off % R)];
    }
};

// Validates the shapes as the bus audit does (its messages, under this audit's name) and lays out the slots
inline MemoryPlan memory_audit_plan(const MachineDesc& machine, const std::vector<BusShape>& main, const std::vector<int>& prep_chips, const std::vector<BusShape>& prep,
                                    std::vector<int>& prep_slot, const MemoryAuditOpts& o, BusPlan* bus_plan = nullptr) {
    BusPlan bp;
    try {
        bp = bus_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what();
        throw std::invalid_argument("memory_audit" + (m.rfind("bus_audit", 0) == 0 ? m.substr(9) : ": " + m));
    }
    const std::string bus = std::string(o.bus_is_global ? "global" : "local") + " bus " + std::to_string(o.bus_index);
    MemoryPlan p;
    p.chips.resize(machine.airs.size());
    size_t n_recv = 0;
    for (size_t i = 0; i < machine.airs.size(); i++) {
        const AirDesc& a = machine.airs[i];
        MemoryPlan::Chip& c = p.chips[i];
        c.height = main[i].height;
        for (size_t m = 0; m < a.interactions.size(); m++) {
            const vair::Interaction& it = a.interactions[m];
            if (it.is_send() || (it.is_local() ? 0u : 1u) != o.bus_is_global || (uint32_t)it.bus_index != o.bus_index) continue;
            if (it.fields.size() != MM_FIELDS)
                throw std::invalid_argument("memory_audit: interaction " + std::to_string(m) + " of chip " + a.name + " receives " + std::to_string(it.fields.size()) + " fields on " + bus +
                                            "; a memory record has exactly 8 (is_read, clk, addr, is_static_initial, v0, v1, v2, v3)");
            c.receives.push_back((uint32_t)m);
        }
        c.first_slot = p.n_slots;
        p.n_slots += c.height * c.receives.size();
        n_recv += c.receives.size();
    }
    if (!n_recv) throw std::invalid_argument("memory_audit: no chip receives on " + bus + ": there is no memory table to audit");
    if (p.n_slots >= 0xffffffffull) throw std::invalid_argument("memory_audit: more than 2^32 - 2 record slots (" + std::to_string(p.n_slots) + "); slot ids are 32-bit");
    if (bus_plan) *bus_plan = std::move(bp);
    return p;
}

inline void memory_audit_header(MemoryReport& rep, const MemoryPlan& plan, const MemoryAuditOpts& o) {
    rep.is_global = o.bus_is_global; rep.bus_index = o.bus_index; rep.max_findings = o.max_findings;
    rep.slots = plan.n_slots; rep.evaluations = (double)plan.n_slots;
    for (size_t i = 0; i < plan.chips.size(); i++)
        for (uint32_t m : plan.chips[i].receives) rep.receives.push_back({(uint32_t)i, m});
}

inline unsigned long long memory_audit_key(uint32_t addr, uint32_t clk, uint32_t is_static) {
    return ((unsigned long long)addr << 32) | ((unsigned long long)clk << 1) | (is_static == 1 ? 0ull : 1ull);
}
inline uint32_t memory_audit_reason(uint32_t count, uint32_t is_read, uint32_t clk, uint32_t is_static, const uint32_t* v) {
    uint32_t r = 0;
    if (count != 1) r |= 1u;
    if (is_read > 1) r |= 2u;
    if (is_static > 1) r |= 4u;
    if (is_static == 1 && (is_read == 1 || clk != 0)) r |= 8u;
    if (v[0] >= 256 || v[1] >= 256 || v[2] >= 256 || v[3] >= 256) r |= 16u;
    return r;
}

// ---- what the device pass and its emulation share (the layouts are stated in kernels/launch.hpp, memory_audit.hip) ----
// the slot table `mt`; entries: the chip of each entry
inline std::vector<uint32_t> memory_audit_mt(const MemoryPlan& plan, std::vector<uint32_t>& entries) {
    entries.clear();
    for (size_t i = 0; i < plan.chips.size(); i++) if (!plan.chips[i].receives.empty()) entries.push_back((uint32_t)i);
    std::vector<uint32_t> w(1 + 4 * entries.size(), 0);
    w[0] = (uint32_t)entries.size();
    for (size_t e = 0; e < entries.size(); e++) {
        const MemoryPlan::Chip& c = plan.chips[entries[e]];
        w[1 + 4 * e] = entries[e]; w[1 + 4 * e + 1] = (uint32_t)c.first_slot; w[1 + 4 * e + 2] = (uint32_t)c.receives.size(); w[1 + 4 * e + 3] = (uint32_t)w.size();
        w.insert(w.end(), c.receives.begin(), c.receives.end());
    }
    return w;
}
// the radix passes: the key bytes in which some live key differs (key_or / key_or_not: the OR of the live keys and of their complements), least
// significant first; with a dead slot (key ~0; a live key's bit 63 is 0) the top byte last, which sinks them behind the live ones
inline int memory_audit_shifts(unsigned long long key_or, unsigned long long key_or_not, bool any_dead, int shifts[8]) {
    const unsigned long long varies = key_or & key_or_not;
    int n = 0;
    for (int b = 0; b < 8; b++)
        if (((varies >> (8 * b)) & 0xffull) || (b == 7 && any_dead)) shifts[n++] = 8 * b;
    return n;
}
// tot: the keys pass's totals; cnt: the judge's; out: the listed findings (MM_OUT = 16 words each)
inline void memory_audit_from_device(MemoryReport& rep, const MemoryPlan& plan, const unsigned long long* tot, const unsigned long long* cnt, const uint32_t* out, size_t listed) {
    rep.live = tot[0]; rep.layout_descents = tot[3];
    if (tot[4]) { rep.descent_chip = (uint32_t)(~tot[4] >> 32); rep.descent_row = (uint32_t)~tot[4]; }
    if (!cnt) return;
    rep.reads = cnt[0]; rep.writes = cnt[1]; rep.statics = cnt[2]; rep.addresses = cnt[3]; rep.uninit_zero_reads = cnt[4]; rep.same_cycle_pairs = cnt[5];
    for (int k = 0; k < 4; k++) { rep.kinds[k] = cnt[6 + k]; rep.total_findings += cnt[6 + k]; }
    rep.dummy_reads_clk = cnt[10]; rep.dummy_reads_addr = cnt[11]; rep.max_clk = (uint32_t)cnt[12]; rep.max_clk_gap = (uint32_t)cnt[13];
    rep.min_addr = (uint32_t)cnt[14]; rep.max_addr = (uint32_t)cnt[15];
    for (size_t t = 0; t < listed; t++) {
        const uint32_t* o = out + 16 * t;
        MemoryFinding f;
        f.kind = o[0]; f.reason = o[1]; f.addr = o[3]; f.clk = o[4]; f.position = o[14];
        plan.decode(o[2], f.chip, f.interaction, f.row);
        for (int j = 0; j < 4; j++) { f.value[j] = o[5 + j]; f.expected[j] = o[9 + j]; }
        if (o[13] != MM_NONE) plan.decode(o[13], f.w_chip, f.w_interaction, f.w_row);
        rep.findings.push_back(f);
    }
}

// The contract on the host: evaluate, stable sort, one walk.
inline MemoryReport memory_audit_host(const MachineDesc& machine, const std::vector<BusHostMatrix>& main, const std::vector<int>& prep_chips, const std::vector<BusHostMatrix>& prep,
                                      const MemoryAuditOpts& opts_in) {
    const MemoryAuditOpts o = memory_audit_checked_opts(opts_in);
    std::vector<BusShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("memory_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("memory_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    const MemoryPlan plan = memory_audit_plan(machine, ms, prep_chips, ps, prep_slot, o);
    MemoryReport rep;
    memory_audit_header(rep, plan, o);
    auto eval = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* prow) {
        uint64_t acc = v.constant % vg::P;
        for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? prow : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
        return (uint32_t)acc;
    };
    struct Rec { unsigned long long key; uint32_t slot, count, is_read, clk, addr, is_static, v[4]; };
    std::vector<Rec> recs;
    for (size_t c = 0; c < machine.airs.size(); c++) {
        const MemoryPlan::Chip& pc = plan.chips[c];
        const size_t R = pc.receives.size();
        if (!R) continue;
        const BusHostMatrix& mm = main[c];
        const BusHostMatrix* pm = prep_slot[c] >= 0 ? &prep[(size_t)prep_slot[c]] : nullptr;
        std::vector<unsigned long long> prev_key(R, 0);
        std::vector<char> prev_live(R, 0);
        for (uint64_t r = 0; r < mm.height; r++) {
            const uint32_t* mrow = mm.data + r * mm.width;
            const uint32_t* prow = pm ? pm->data + r * pm->width : nullptr;
            for (size_t k = 0; k < R; k++) {
                const vair::Interaction& it = machine.airs[c].interactions[pc.receives[k]];
                Rec x;
                x.count = eval(it.count, mrow, prow);
                if (!x.count) { prev_live[k] = 0; continue; }
                x.is_read = eval(it.fields[0], mrow, prow); x.clk = eval(it.fields[1], mrow, prow); x.addr = eval(it.fields[2], mrow, prow); x.is_static = eval(it.fields[3], mrow, prow);
                for (int j = 0; j < 4; j++) x.v[j] = eval(it.fields[4 + j], mrow, prow);
                x.key = memory_audit_key(x.addr, x.clk, x.is_static);
                x.slot = (uint32_t)(pc.first_slot + r * R + k);
                if (prev_live[k] && prev_key[k] > x.key && !rep.layout_descents++) { rep.descent_chip = (uint32_t)c; rep.descent_row = (uint32_t)(r - 1); }  // chips and rows ascend
                prev_live[k] = 1; prev_key[k] = x.key;
                recs.push_back(x);
            }
        }
    }
    std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.key < b.key; });
    const uint64_t L = recs.size();
    rep.live = L;
    if (L) { rep.min_addr = recs.front().addr; rep.max_addr = recs.back().addr; }
    const Rec* last_write = nullptr;
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec& x = recs[i];
        const Rec* pv = i ? &recs[i - 1] : nullptr;
        const bool first = !pv || pv->addr != x.addr, read = x.is_read == 1, is_static = x.is_static == 1;
        if (first) { last_write = nullptr; rep.addresses++; }
        (read ? rep.reads : rep.writes)++;
        if (is_static) rep.statics++;
        rep.max_clk = std::max(rep.max_clk, x.clk);
        if (!first) {
            const uint32_t gap = x.clk - pv->clk;
            rep.max_clk_gap = std::max(rep.max_clk_gap, gap);
            if (gap > L) rep.dummy_reads_clk += gap / L;
            if (pv->clk == x.clk && !is_static && pv->is_static != 1 && (!read || pv->is_read != 1)) rep.same_cycle_pairs++;
        } else if (pv) {
            const uint32_t diff = x.addr - pv->addr;
            if (diff > L) rep.dummy_reads_addr += diff / L;
        }
        const bool differs = last_write && (x.v[0] != last_write->v[0] || x.v[1] != last_write->v[1] || x.v[2] != last_write->v[2] || x.v[3] != last_write->v[3]);
        const bool nonzero = (x.v[0] | x.v[1] | x.v[2] | x.v[3]) != 0;
        if (read && !last_write && !nonzero) rep.uninit_zero_reads++;
        const uint32_t reason = memory_audit_reason(x.count, x.is_read, x.clk, x.is_static, x.v);
        uint32_t kind = 0;
        if (reason) kind = MM_MALFORMED;
        else if (is_static && !first && pv->is_static == 1) kind = MM_DUPLICATE_STATIC;
        else if (read && differs) kind = MM_STALE_READ;
        else if (read && !last_write && nonzero) kind = MM_UNINIT_READ;
        if (kind) {
            rep.total_findings++;
            rep.kinds[kind - 1]++;
            if (rep.findings.size() < o.max_findings) {
                MemoryFinding f;
                f.kind = kind; f.reason = reason; f.addr = x.addr; f.clk = x.clk; f.position = (uint32_t)i;
                plan.decode(x.slot, f.chip, f.interaction, f.row);
                for (int j = 0; j < 4; j++) { f.value[j] = x.v[j]; f.expected[j] = last_write ? last_write->v[j] : 0u; }
                if (last_write) plan.decode(last_write->slot, f.w_chip, f.w_interaction, f.w_row);
                rep.findings.push_back(f);
            }
        }
        if (!read) last_write = &x;
    }
    return rep;
}

}  // namespace vhost
