// Domain audit: the other audits judge a witness by local algebra; a LOOKUP MEMBERSHIP ties a cell to a set ("this cell is a byte because it is
// sent to the range bus"), and none of them sees a missing one.  This audit reports, per chip and main column, the set of values the witness puts
// there and the rows on which a narrow column is not a field of a live send to a lookup table.
//   vcol           constant + sum weight * cell (mod p) at row r over main / preprocessed cells of row r (vair::VirtualCol).  A field or count is
//                  BARE(c) iff it has one term, main, column c, weight 1, constant 0.  A record (chip, interaction, row) is LIVE iff its count
//                  vcol != 0 at that row.
//   column domain  per main column of every audited chip, over all n rows, canonical values: min, max, nonzero_rows, wide_rows (value >= 2^16),
//                  distinct_narrow (distinct values < 2^16, exact), dense (wide_rows = 0 and distinct_narrow = max - min + 1), bits (bit length of
//                  max), class 0 CONSTANT (min = max), 1 BOOLEAN (max <= 1), 2 BYTE (max < 2^8), 3 HALF (max < 2^16), 4 WIDE.  NARROW iff the
//                  class is BYTE or HALF and max < 2^max_bits (max_bits <= 16).
//   lookup buses   a TABLE CHIP has no constraint, no send and at least one receive.  Bus (is_global, bus_index) is a LOOKUP BUS iff it has a
//                  receive and every receive on it, machine-wide, belongs to a table chip: a rule of the machine's structure alone
//                  (lookup_auto = 1).  lookup_auto = 0: bit bus_index of lookup_global_mask / lookup_local_mask decides (bus indices >= 64 are
//                  refused then).  Buses ascend by (is_global, bus_index).
//   appearances    (interaction, field position) at which column c is bare; per appearance live_rows.  Per column: guarded_rows (rows with a
//                  live bare SEND on a lookup bus), sent_rows (a live bare send on any other bus), received_rows (a live bare receive),
//                  unguarded_rows = n - guarded_rows, unguarded_nonzero_rows (unguarded and the cell != 0), mixed_rows (rows with a live send one
//                  of whose fields reads c but is not bare(c): 256 a + b guards neither a nor b).
//   entries        the narrow columns with unguarded_nonzero_rows > 0, ascending (chip, column), each with its appearances and its first
//                  max_rows_per_entry unguarded non-zero rows (row, value) ascending; total_entries stays exact when the list is cut.
//   bus positions  per bus, field position and direction, over the live records of the WHOLE machine (chip_mask does not narrow them): min,
//                  max, distinct_narrow, wide_records, records, and the bus's lookup flag: what a table actually offers.
// What it is not: THIS witness only (a short program leaves columns accidentally narrow); only bare fields guard; values near p (small
// negatives) are WIDE; a guard says the cell is looked up, not that the table is sound.  `check`'s exit status never depends on it.
// This header holds what the host and the device implementation share — options, the plan (lookup buses, appearances, the virtual-column table),
// the report and its word image, the entries from the columns' numbers — and the host implementation (plain C++, one thread, no limits).  The
// device pass is Prover::domain_audit (prover_audits.cpp, kernels/domain_audit.hip).
#pragma once
#include <map>
#include "rank_audit.hpp"

namespace vhost {

struct DomainAuditOpts {
    uint64_t max_entries = 1024;      // taken as given: 0 lists no entry (the counts stay exact)
    uint32_t max_rows_per_entry = 4;  // taken as given: 0 lists no row
    uint32_t chip_mask = 0;           // bit h: audit chip h; 0: all chips
    uint32_t max_bits = 16;           // 0: 16
    uint32_t lookup_auto = 1;         // taken as given
    uint64_t lookup_global_mask = 0, lookup_local_mask = 0;
    uint32_t reserved[2] = {0, 0};
};

constexpr uint32_t DM_CONSTANT = 0, DM_BOOLEAN = 1, DM_BYTE = 2, DM_HALF = 3, DM_WIDE = 4;
constexpr uint32_t DM_BITMAP_WORDS = 2048;                                      // one bit per value < 2^16
constexpr uint32_t DM_GUARDED = 0, DM_SENT = 1, DM_RECEIVED = 2, DM_MIXED = 3;  // what a live item says about its column's row
constexpr uint32_t DM_COLUMN_WORDS = 24, DM_POSITION_WORDS = 12, DM_CHIP_WORDS = 10, DM_APPEARANCE_WORDS = 8;

inline std::string dm_renamed(const std::invalid_argument& e, const char* from_name) {
    const std::string m = e.what(), from = std::string(from_name) + ": ";
    return m.compare(0, from.size(), from) == 0 ? "domain_audit: " + m.substr(from.size()) : m;
}

inline DomainAuditOpts domain_audit_checked_opts(const DomainAuditOpts& in, size_t n_chips) {
    if (in.reserved[0] != 0 || in.reserved[1] != 0) throw std::invalid_argument("domain_audit: the reserved fields of the options must be zero");
    DomainAuditOpts o = in;
    if (o.max_entries > (1ull << 24)) throw std::invalid_argument("domain_audit: max_entries is at most 2^24");
    if (o.max_rows_per_entry > 4096) throw std::invalid_argument("domain_audit: max_rows_per_entry is at most 4096");
    if (n_chips < 32 && (o.chip_mask >> n_chips) != 0) throw std::invalid_argument("domain_audit: chip_mask names a chip the machine does not have (" + std::to_string(n_chips) + " chips)");
    if (n_chips > 32 && o.chip_mask != 0) throw std::invalid_argument("domain_audit: chip_mask selects among at most 32 chips");
    if (o.max_bits == 0) o.max_bits = 16;
    if (o.max_bits > 16) throw std::invalid_argument("domain_audit: max_bits is at most 16 (" + std::to_string(o.max_bits) + " given): distinct values are counted below 2^16");
    if (o.lookup_auto > 1) throw std::invalid_argument("domain_audit: lookup_auto is 0 or 1");
    return o;
}
inline bool domain_audit_selected(const DomainAuditOpts& o, size_t chip) { return o.chip_mask == 0 || ((o.chip_mask >> chip) & 1u); }

// ---- the plan: what the machine's structure alone decides ----------------------------------------------------------------------------------
struct DomainBus {
    uint32_t is_global = 0, bus_index = 0, lookup = 0, width = 0;  // width: the most fields of an interaction on it
    uint32_t pos_at = 0;                                           // its first position record: position j, direction d (0 send, 1 receive) is pos_at + 2 j + d
};
struct DomainAppearance { uint32_t column, interaction, position, is_send, bus, lookup; };  // bus: index into DomainPlan::buses
struct DomainItem { uint32_t column, interaction, kind, appearance; };                      // kind: DM_*; appearance: index or ~0 (mixed)
struct DomainChipPlan {
    uint32_t is_table = 0;
    std::vector<DomainAppearance> apps;  // ascending (column, interaction, position)
    std::vector<DomainItem> items;       // ascending column: the appearances, then the column's mixed sends (each interaction once)
    std::vector<uint32_t> item_at;       // [w + 1]: column c's items are [item_at[c], item_at[c + 1])
    std::vector<uint32_t> field_at;      // [M + 1]: interaction m's fields are the field vcols field_at[m] ..
    std::vector<uint32_t> field_pos;     // per field vcol its position record
};
struct DomainPlan {
    std::vector<DomainBus> buses;
    uint32_t n_positions = 0;
    std::vector<DomainChipPlan> chips;
    std::vector<int> prep_slot;
};

inline bool dm_bare(const vair::VirtualCol& v, uint32_t& c) {
    if (v.terms.size() != 1 || v.constant != 0 || v.terms[0].preprocessed || v.terms[0].weight != 1 || v.terms[0].col < 0) return false;
    c = (uint32_t)v.terms[0].col;
    return true;
}

inline DomainPlan domain_audit_plan(const MachineDesc& machine, const std::vector<ConstraintShape>& main, const std::vector<int>& prep_chips, const std::vector<ConstraintShape>& prep,
                                    const DomainAuditOpts& o) {
    DomainPlan plan;
    try {
        mutation_audit_plan(machine, main, prep_chips, prep, plan.prep_slot);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(dm_renamed(e, "mutation_audit"));
    }
    const size_t NC = machine.airs.size();
    plan.chips.resize(NC);
    // table chips, then the buses in ascending (is_global, bus_index)
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& a = machine.airs[c];
        bool sends = false, receives = false;
        for (auto& it : a.interactions) (it.is_send() ? sends : receives) = true;
        plan.chips[c].is_table = (!a.program.num_asserts && !sends && receives) ? 1u : 0u;
    }
    struct Seen { uint32_t width = 0; bool receive = false, all_table = true; };
    std::map<std::pair<uint32_t, uint32_t>, Seen> seen;
    for (size_t c = 0; c < NC; c++)
        for (auto& it : machine.airs[c].interactions) {
            if (it.bus_index < 0) throw std::invalid_argument("domain_audit: a negative bus index (chip " + machine.airs[c].name + ")");
            if (!o.lookup_auto && it.bus_index >= 64)
                throw std::invalid_argument("domain_audit: bus index " + std::to_string(it.bus_index) + " of chip " + machine.airs[c].name +
                                            " does not fit the 64-bit lookup masks (lookup_auto = 1 takes any index)");
            Seen& s = seen[{it.is_local() ? 0u : 1u, (uint32_t)it.bus_index}];
            s.width = std::max<uint32_t>(s.width, (uint32_t)it.fields.size());
            if (!it.is_send()) { s.receive = true; s.all_table &= plan.chips[c].is_table != 0; }
        }
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> slot;
    for (auto& kv : seen) {
        DomainBus b;
        b.is_global = kv.first.first; b.bus_index = kv.first.second; b.width = kv.second.width;
        if (o.lookup_auto) b.lookup = (kv.second.receive && kv.second.all_table) ? 1u : 0u;
        else b.lookup = (uint32_t)(((b.is_global ? o.lookup_global_mask : o.lookup_local_mask) >> b.bus_index) & 1u);
        b.pos_at = plan.n_positions;
        plan.n_positions += 2 * b.width;
        slot[kv.first] = (uint32_t)plan.buses.size();
        plan.buses.push_back(b);
    }
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& a = machine.airs[c];
        DomainChipPlan& cp = plan.chips[c];
        const uint32_t W = a.width, M = (uint32_t)a.interactions.size();
        std::vector<std::vector<DomainItem>> per(W);
        cp.field_at.assign(M + 1, 0);
        for (uint32_t m = 0; m < M; m++) {
            const vair::Interaction& it = a.interactions[m];
            const uint32_t bs = slot[{it.is_local() ? 0u : 1u, (uint32_t)it.bus_index}];
            const DomainBus& b = plan.buses[bs];
            cp.field_at[m + 1] = cp.field_at[m] + (uint32_t)it.fields.size();
            std::vector<char> mixed(W, 0);
            for (uint32_t j = 0; j < it.fields.size(); j++) {
                cp.field_pos.push_back(b.pos_at + 2 * j + (it.is_send() ? 0u : 1u));
                uint32_t col = 0;
                if (dm_bare(it.fields[j], col)) {
                    const uint32_t lookup = (it.is_send() && b.lookup) ? 1u : 0u;
                    per[col].push_back({col, m, it.is_send() ? (lookup ? DM_GUARDED : DM_SENT) : DM_RECEIVED, j});  // appearance: the position for now
                } else if (it.is_send()) {
                    for (auto& t : it.fields[j].terms) if (!t.preprocessed) mixed[(size_t)t.col] = 1;
                }
            }
            for (uint32_t col = 0; col < W; col++) if (mixed[col]) per[col].push_back({col, m, DM_MIXED, 0xffffffffu});
        }
        cp.item_at.assign(W + 1, 0);
        for (uint32_t col = 0; col < W; col++) {
            // the appearances ascend by (interaction, position) as pushed; the mixed sends go behind them
            std::stable_sort(per[col].begin(), per[col].end(), [](const DomainItem& x, const DomainItem& y) { return (x.kind == DM_MIXED) < (y.kind == DM_MIXED); });
            for (DomainItem it : per[col]) {
                if (it.kind != DM_MIXED) {
                    const vair::Interaction& in = a.interactions[it.interaction];
                    const uint32_t bs = slot[{in.is_local() ? 0u : 1u, (uint32_t)in.bus_index}];
                    cp.apps.push_back({col, it.interaction, it.appearance, in.is_send() ? 1u : 0u, bs, it.kind == DM_GUARDED ? 1u : 0u});
                    it.appearance = (uint32_t)cp.apps.size() - 1;
                }
                cp.items.push_back(it);
            }
            cp.item_at[col + 1] = (uint32_t)cp.items.size();
        }
    }
    return plan;
}

// ---- the report -----------------------------------------------------------------------------------------------------------------------------
struct DomainColumn {
    uint32_t min = 0, max = 0, distinct = 0, cls = 0, dense = 0, bits = 0, narrow = 0, n_appearances = 0;
    uint64_t nonzero = 0, wide = 0, guarded = 0, sent = 0, received = 0, unguarded = 0, unguarded_nonzero = 0, mixed = 0;
};
struct DomainPosition {
    uint32_t bus = 0, position = 0, is_send = 0, lookup = 0, min = 0, max = 0, distinct = 0;
    uint64_t wide = 0, records = 0;
};
struct DomainChipStat {
    uint32_t width = 0, n_constraints = 0, n_interactions = 0, audited = 0;
    uint64_t height = 0;
    uint32_t is_table = 0, narrow = 0, entries = 0, n_appearances = 0;
    std::vector<DomainColumn> cols;   // [width]; zero records for a chip that is not audited
    std::vector<uint64_t> app_live;   // per appearance of the chip's plan its live rows
};
struct DomainEntry {
    uint32_t chip = 0, column = 0, cls = 0, max = 0;
    uint64_t unguarded_nonzero = 0;
    std::vector<uint32_t> apps;  // DM_APPEARANCE_WORDS per appearance: interaction, position, is_send, is_global, bus_index, lookup, live_rows lo, hi
    std::vector<uint32_t> rows;  // (row, value) pairs, ascending row
};
struct DomainReport {
    bool truncated = false;
    uint32_t max_bits = 16, lookup_auto = 1;
    uint64_t total_entries = 0;
    std::vector<DomainChipStat> chips;
    std::vector<DomainBus> buses;
    std::vector<DomainPosition> positions;
    std::vector<DomainEntry> entries;  // ascending (chip, column)
    double device_ms = 0, host_ms = 0, evaluations = 0;  // not part of the word image; evaluations: cells scanned
    static constexpr uint32_t MAGIC = 0x314d4456u;  // "VDM1"
    // Flat image (include/vgpu.h documents it next to vgpu_domain_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(max_bits); w.push_back(truncated ? 1u : 0u);
        u64(total_entries);
        w.push_back((uint32_t)entries.size()); w.push_back((uint32_t)chips.size());
        w.push_back(lookup_auto); w.push_back((uint32_t)buses.size()); w.push_back((uint32_t)positions.size()); w.push_back(0);
        for (auto& c : chips) {
            w.push_back(c.width); w.push_back(c.n_constraints); w.push_back(c.n_interactions); w.push_back(c.audited);
            u64(c.height);
            w.push_back(c.is_table); w.push_back(c.narrow); w.push_back(c.entries); w.push_back(c.n_appearances);
            for (auto& k : c.cols) {
                w.push_back(k.min); w.push_back(k.max); w.push_back(k.distinct); w.push_back(k.cls);
                w.push_back(k.dense); w.push_back(k.bits); w.push_back(k.narrow); w.push_back(k.n_appearances);
                u64(k.nonzero); u64(k.wide); u64(k.guarded); u64(k.sent); u64(k.received); u64(k.unguarded); u64(k.unguarded_nonzero); u64(k.mixed);
            }
        }
        for (auto& b : buses) { w.push_back(b.is_global); w.push_back(b.bus_index); w.push_back(b.lookup); w.push_back(b.width); }
        for (auto& p : positions) {
            w.push_back(p.bus); w.push_back(p.position); w.push_back(p.is_send); w.push_back(p.lookup);
            w.push_back(p.min); w.push_back(p.max); w.push_back(p.distinct); w.push_back(0);
            u64(p.wide); u64(p.records);
        }
        for (auto& e : entries) {
            w.push_back(e.chip); w.push_back(e.column); w.push_back(e.cls); w.push_back(e.max);
            w.push_back((uint32_t)(e.apps.size() / DM_APPEARANCE_WORDS)); w.push_back((uint32_t)(e.rows.size() / 2));
            u64(e.unguarded_nonzero);
            w.insert(w.end(), e.apps.begin(), e.apps.end());
            w.insert(w.end(), e.rows.begin(), e.rows.end());
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

// What a scan of one virtual column leaves: the device pass keeps the same five numbers and the same bitmap per slot
struct DomainScan {
    uint32_t min = 0xffffffffu, max = 0;
    uint64_t nonzero = 0, wide = 0, live = 0;
    std::vector<uint32_t> bitmap = std::vector<uint32_t>(DM_BITMAP_WORDS, 0);
    void add(uint32_t v) {
        min = std::min(min, v); max = std::max(max, v);
        live++; nonzero += v != 0;
        if (v >> 16) wide++; else bitmap[v >> 5] |= 1u << (v & 31u);
    }
    uint32_t distinct() const { uint32_t s = 0; for (uint32_t x : bitmap) s += (uint32_t)__builtin_popcount(x); return s; }
};

// class, dense, bits and the narrow flag of a column from its numbers
inline void domain_audit_classify(DomainColumn& k, uint32_t max_bits) {
    k.cls = k.min == k.max ? DM_CONSTANT : k.max <= 1 ? DM_BOOLEAN : k.max < 256 ? DM_BYTE : k.max < 65536 ? DM_HALF : DM_WIDE;
    k.dense = (!k.wide && k.distinct == k.max - k.min + 1) ? 1u : 0u;
    k.bits = k.max ? 32u - (uint32_t)__builtin_clz(k.max) : 0u;
    k.narrow = ((k.cls == DM_BYTE || k.cls == DM_HALF) && k.max < (1u << max_bits)) ? 1u : 0u;
}

// The static part of the report: chip blocks, buses and position records (their numbers are filled in later)
inline void domain_audit_blocks(DomainReport& rep, const MachineDesc& machine, const DomainPlan& plan, const std::vector<ConstraintShape>& main, const DomainAuditOpts& o) {
    const size_t NC = machine.airs.size();
    rep.max_bits = o.max_bits; rep.lookup_auto = o.lookup_auto;
    rep.chips.assign(NC, DomainChipStat{});
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        DomainChipStat& cs = rep.chips[c];
        cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = main[c].height;
        cs.audited = domain_audit_selected(o, c) ? 1u : 0u;
        cs.is_table = plan.chips[c].is_table;
        cs.cols.assign(air.width, DomainColumn{});
        if (!cs.audited) continue;
        cs.n_appearances = (uint32_t)plan.chips[c].apps.size();
        cs.app_live.assign(plan.chips[c].apps.size(), 0);
        for (auto& a : plan.chips[c].apps) cs.cols[a.column].n_appearances++;
    }
    rep.buses = plan.buses;
    rep.positions.assign(plan.n_positions, DomainPosition{});
    for (size_t b = 0; b < plan.buses.size(); b++)
        for (uint32_t j = 0; j < plan.buses[b].width; j++)
            for (uint32_t d = 0; d < 2; d++) {
                DomainPosition& p = rep.positions[plan.buses[b].pos_at + 2 * j + d];
                p.bus = (uint32_t)b; p.position = j; p.is_send = d == 0 ? 1u : 0u; p.lookup = plan.buses[b].lookup;
            }
}

// The entries (without rows) from the columns' numbers, the chips' counts, and the cut at max_entries
inline void domain_audit_entries(DomainReport& rep, const DomainPlan& plan, const DomainAuditOpts& o) {
    rep.entries.clear();
    rep.total_entries = 0;
    for (size_t c = 0; c < rep.chips.size(); c++) {
        DomainChipStat& cs = rep.chips[c];
        cs.narrow = cs.entries = 0;
        if (!cs.audited) continue;
        const DomainChipPlan& cp = plan.chips[c];
        for (uint32_t col = 0; col < cs.width; col++) {
            const DomainColumn& k = cs.cols[col];
            if (!k.narrow) continue;
            cs.narrow++;
            if (!k.unguarded_nonzero) continue;
            cs.entries++;
            rep.total_entries++;
            if (rep.entries.size() >= o.max_entries) continue;
            DomainEntry e;
            e.chip = (uint32_t)c; e.column = col; e.cls = k.cls; e.max = k.max; e.unguarded_nonzero = k.unguarded_nonzero;
            for (size_t i = 0; i < cp.apps.size(); i++) {
                const DomainAppearance& a = cp.apps[i];
                if (a.column != col) continue;
                const DomainBus& b = plan.buses[a.bus];
                const uint32_t aw[DM_APPEARANCE_WORDS] = {a.interaction, a.position, a.is_send, b.is_global, b.bus_index, a.lookup, (uint32_t)cs.app_live[i], (uint32_t)(cs.app_live[i] >> 32)};
                e.apps.insert(e.apps.end(), aw, aw + DM_APPEARANCE_WORDS);
            }
            rep.entries.push_back(std::move(e));
        }
    }
    rep.truncated = rep.total_entries > rep.entries.size();
}

// a position record's numbers from its scan (no live record: all zero)
inline void domain_audit_position(DomainPosition& p, const DomainScan& s) {
    if (!s.live) return;
    p.min = s.min; p.max = s.max; p.distinct = s.distinct(); p.wide = s.wide; p.records = s.live;
}

// ---- what the device pass takes (kernels/launch.hpp: DaArgs) ---------------------------------------------------------------------------------
// Where the count vcol and the field vcols of each interaction start in the chip's encoded interactions (kernels/interactions.hpp)
struct DomainOffsets { std::vector<uint32_t> count_at; std::vector<std::vector<uint32_t>> field_at; };
inline DomainOffsets domain_audit_offsets(const std::vector<uint32_t>& iw) {
    DomainOffsets o;
    const uint32_t M = iw.empty() ? 0u : iw[0];
    for (uint32_t m = 0; m < M; m++) {
        uint32_t pos = iw[2 + m];
        const uint32_t nf = iw[pos + 1];
        pos += 2;
        o.count_at.push_back(pos);
        pos += 2 + 2 * iw[pos];
        o.field_at.emplace_back();
        for (uint32_t j = 0; j < nf; j++) { o.field_at.back().push_back(pos); pos += 2 + 2 * iw[pos]; }
    }
    return o;
}
// Slots: the position records first, then the main columns of the audited chips in machine order (slot0[c]: chip c's column 0)
inline uint32_t domain_audit_slots(const MachineDesc& machine, const DomainPlan& plan, const DomainAuditOpts& o, std::vector<uint32_t>& slot0) {
    uint32_t n = plan.n_positions;
    slot0.assign(machine.airs.size(), 0);
    for (size_t c = 0; c < machine.airs.size(); c++) {
        slot0[c] = n;
        if (domain_audit_selected(o, c)) n += machine.airs[c].width;
    }
    return n;
}
// The virtual columns a chip's scan walks: [NV][4] kind, column / field offset, count offset, slot
inline std::vector<uint32_t> domain_audit_vt(const AirDesc& air, const DomainChipPlan& cp, bool audited, uint32_t slot0) {
    std::vector<uint32_t> vt;
    if (audited)
        for (uint32_t col = 0; col < air.width; col++) { vt.push_back(0); vt.push_back(col); vt.push_back(0); vt.push_back(slot0 + col); }
    const DomainOffsets off = domain_audit_offsets(air.interaction_words);
    for (size_t m = 0; m < off.count_at.size(); m++)
        for (size_t j = 0; j < off.field_at[m].size(); j++) { vt.push_back(1); vt.push_back(off.field_at[m][j]); vt.push_back(off.count_at[m]); vt.push_back(cp.field_pos[cp.field_at[m] + j]); }
    return vt;
}
// The guard table of a chip: [0] items, [1] width, item_at [w + 1], then per item count offset, kind, appearance
inline std::vector<uint32_t> domain_audit_gt(const AirDesc& air, const DomainChipPlan& cp) {
    const DomainOffsets off = domain_audit_offsets(air.interaction_words);
    std::vector<uint32_t> gt{(uint32_t)cp.items.size(), air.width};
    gt.insert(gt.end(), cp.item_at.begin(), cp.item_at.end());
    for (auto& it : cp.items) { gt.push_back(off.count_at[it.interaction]); gt.push_back(it.kind); gt.push_back(it.appearance); }
    return gt;
}

// The contract on the host; one thread.
inline DomainReport domain_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                      const std::vector<ConstraintHostMatrix>& prep, const DomainAuditOpts& opts_in) {
    const DomainAuditOpts o = domain_audit_checked_opts(opts_in, machine.airs.size());
    std::vector<ConstraintShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("domain_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("domain_audit: null trace"); ps.push_back({m.height, m.width}); }
    const DomainPlan plan = domain_audit_plan(machine, ms, prep_chips, ps, o);
    const size_t NC = machine.airs.size();
    DomainReport rep;
    domain_audit_blocks(rep, machine, plan, ms, o);
    std::vector<DomainScan> pscan(plan.n_positions);
    auto vcol = [&](size_t c, const vair::VirtualCol& v, uint64_t r) {
        uint64_t acc = v.constant % vg::P;
        for (auto& t : v.terms) {
            const ConstraintHostMatrix& m = t.preprocessed ? prep[(size_t)plan.prep_slot[c]] : main[c];
            acc = (acc + (uint64_t)(t.weight % vg::P) * (m.data[r * m.width + (uint64_t)t.col] % vg::P)) % vg::P;
        }
        return (uint32_t)acc;
    };
    for (size_t c = 0; c < NC; c++) {
        const AirDesc& air = machine.airs[c];
        DomainChipStat& cs = rep.chips[c];
        const DomainChipPlan& cp = plan.chips[c];
        const uint64_t n = main[c].height;
        const uint32_t W = air.width, M = (uint32_t)air.interactions.size();
        // the field vcols gated by live, of every chip
        std::vector<uint8_t> live((size_t)n * (M ? M : 1), 0);
        for (uint32_t m = 0; m < M; m++) {
            const vair::Interaction& it = air.interactions[m];
            for (uint64_t r = 0; r < n; r++) {
                if (!vcol(c, it.count, r)) continue;
                live[r * M + m] = 1;
                for (uint32_t j = 0; j < it.fields.size(); j++) pscan[cp.field_pos[cp.field_at[m] + j]].add(vcol(c, it.fields[j], r));
            }
            rep.evaluations += (double)n * (1.0 + it.fields.size());
        }
        if (!cs.audited || !W) continue;
        rep.evaluations += (double)n * W;
        for (uint32_t col = 0; col < W; col++) {
            DomainColumn& k = cs.cols[col];
            DomainScan s;
            for (uint64_t r = 0; r < n; r++) s.add(main[c].data[r * W + col] % vg::P);
            k.min = s.min; k.max = s.max; k.distinct = s.distinct(); k.nonzero = s.nonzero; k.wide = s.wide;
            domain_audit_classify(k, o.max_bits);
            for (uint64_t r = 0; r < n; r++) {
                bool f[4] = {false, false, false, false};
                for (uint32_t i = cp.item_at[col]; i < cp.item_at[col + 1]; i++) {
                    const DomainItem& it = cp.items[i];
                    if (!live[r * M + it.interaction]) continue;
                    f[it.kind] = true;
                    if (it.kind != DM_MIXED) cs.app_live[it.appearance]++;
                }
                k.guarded += f[DM_GUARDED]; k.sent += f[DM_SENT]; k.received += f[DM_RECEIVED]; k.mixed += f[DM_MIXED];
                k.unguarded_nonzero += !f[DM_GUARDED] && main[c].data[r * W + col] % vg::P != 0;
            }
            k.unguarded = n - k.guarded;
        }
    }
    for (uint32_t p = 0; p < plan.n_positions; p++) domain_audit_position(rep.positions[p], pscan[p]);
    domain_audit_entries(rep, plan, o);
    for (DomainEntry& e : rep.entries) {
        const size_t c = e.chip;
        const DomainChipPlan& cp = plan.chips[c];
        const uint32_t W = machine.airs[c].width;
        for (uint64_t r = 0; r < main[c].height && e.rows.size() < 2ull * o.max_rows_per_entry; r++) {
            const uint32_t v = main[c].data[r * W + e.column] % vg::P;
            if (!v) continue;
            bool guarded = false;
            for (uint32_t i = cp.item_at[e.column]; i < cp.item_at[e.column + 1] && !guarded; i++)
                guarded = cp.items[i].kind == DM_GUARDED && vcol(c, machine.airs[c].interactions[cp.items[i].interaction].count, r) != 0;
            if (!guarded) { e.rows.push_back((uint32_t)r); e.rows.push_back(v); }
        }
    }
    return rep;
}

}  // namespace vhost
