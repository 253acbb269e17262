// Link audit: the join the field audit leaves to the reader.  A floating field on a send usually means that the chip delegates; the finding
// is a field that floats at EVERY record carrying the tuple, on the sending and on the receiving side.
//   records, buses, "same tuple" (after zero-padding to the bus's widest interaction) and record order are the bus audit's (host/bus_audit.hpp),
//   float masks are the field audit's (host/field_audit.hpp: the same Jacobian rows, the same n = 1 rule, the same constant rule); all chips
//   are audited: a join needs every end.
//   record mask  of a live record of interaction m with nf fields on a bus of width W <= 32: bit j < nf is set iff field j floats at that row;
//                bits nf .. W - 1 are clear (a padded position is the constant 0: pinned), constant and determined fields are clear.
//   tuple mask   the AND of the record masks of all the tuple's records, sends and receives alike.  Position j is OPEN in the tuple iff its
//                bit is set, otherwise ANCHORED; a tuple with a non-zero mask is an open tuple.  `net` is ignored: balanced and unbalanced
//                witnesses are audited alike.
//   per record   a field that floats at a record is OPEN there when its position is open in the record's tuple, otherwise ANSWERED: it
//                floats locally and another record of the tuple pins it.
// It is first order, on this witness.  Each record is judged alone (the field audit does not hold sister records of the same row fixed), so
// "open" means that no single record's own chip pins the position: a joint move may still be blocked by a sister record.  "Anchored" is per
// tuple as it stands: a lookup bus whose receiver can move multiplicities between tuples is not modelled.
// This header holds what host and device share — the options, the report and its word image, the finishing step — and the host
// implementation (plain C++, one thread, no limit beyond the 32-field bus).  The device pass is Prover::link_audit (prover_audits.cpp,
// kernels/link_audit.hip).
#pragma once
#include "bus_audit.hpp"
#include "field_audit.hpp"

namespace vhost {

struct LinkAuditOpts {
    uint64_t max_tuples = 64;
    uint32_t max_records_per_tuple = 4;
    uint32_t hash_bits = 64;  // the bus audit's test hook: the device's grouping key is cut to this many bits (the report must not change)
    uint32_t reserved = 0;
};
constexpr uint32_t LA_MAX_WIDTH = 32;  // fields of a bus: the tuple mask is one word

struct LinkBusStat {
    uint32_t is_global = 0, bus_index = 0, width = 0;
    uint64_t live = 0, tuples = 0, open_tuples = 0;
    std::vector<uint64_t> open_in, open_records;  // per position: tuples in which it is open, and the records of those tuples
};
struct LinkInteractionStat {
    uint32_t is_send = 0, is_global = 0, bus_index = 0, n_fields = 0;
    uint64_t live_rows = 0;
    std::vector<uint32_t> constant;        // per field: 1 when it has no main-column weight
    std::vector<uint64_t> floating, open;  // per field: rows where it floats; of those, rows where its position is open in the tuple
};
struct LinkRecord { uint32_t chip = 0, row = 0, interaction = 0, is_send = 0, mask = 0; };
struct LinkTuple {
    uint32_t is_global = 0, bus_index = 0, mask = 0;
    uint64_t n_send = 0, n_recv = 0;
    std::vector<uint32_t> fields;     // padded to the bus's width
    std::vector<LinkRecord> records;  // the first max_records_per_tuple in record order
};
struct LinkReport {
    bool truncated = false;
    uint64_t total_open = 0;  // open tuples, exact even when the list is cut
    std::vector<LinkBusStat> buses;                       // ascending (is_global, bus_index)
    std::vector<std::vector<LinkInteractionStat>> chips;  // machine order
    std::vector<LinkTuple> tuples;                        // the open tuples, ascending by first record
    double device_ms = 0, host_ms = 0, evaluations = 0;   // not part of the word image
    static constexpr uint32_t MAGIC = 0x31414C56u;  // "VLA1"
    // Flat image (include/vgpu.h documents it next to vgpu_link_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(truncated ? 1u : 0u);
        u64(total_open);
        w.push_back((uint32_t)tuples.size()); w.push_back((uint32_t)buses.size()); w.push_back((uint32_t)chips.size());
        for (auto& b : buses) {
            w.push_back(b.is_global); w.push_back(b.bus_index); w.push_back(b.width);
            u64(b.live); u64(b.tuples); u64(b.open_tuples);
            for (uint32_t j = 0; j < b.width; j++) { u64(b.open_in[j]); u64(b.open_records[j]); }
        }
        for (auto& c : chips) {
            w.push_back((uint32_t)c.size());
            for (auto& it : c) {
                w.push_back(it.is_send); w.push_back(it.is_global); w.push_back(it.bus_index); w.push_back(it.n_fields);
                u64(it.live_rows);
                for (uint32_t j = 0; j < it.n_fields; j++) { w.push_back(it.constant[j]); u64(it.floating[j]); u64(it.open[j]); }
            }
        }
        for (auto& t : tuples) {
            w.push_back(t.is_global); w.push_back(t.bus_index); w.push_back((uint32_t)t.fields.size()); w.push_back(t.mask);
            u64(t.n_send); u64(t.n_recv);
            w.push_back((uint32_t)t.records.size());
            for (uint32_t f : t.fields) w.push_back(f);
            for (auto& r : t.records) { w.push_back(r.chip); w.push_back(r.row); w.push_back(r.interaction); w.push_back(r.is_send); w.push_back(r.mask); }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline std::string link_audit_renamed(const std::string& m) {
    for (const char* from : {"bus_audit: ", "field_audit: ", "rank_audit: "}) {
        const std::string f = from;
        if (m.compare(0, f.size(), f) == 0) return "link_audit: " + m.substr(f.size());
    }
    return m;
}
inline LinkAuditOpts link_audit_checked_opts(const LinkAuditOpts& in) {
    if (in.reserved) throw std::invalid_argument("link_audit: the reserved option word must be zero");
    BusAuditOpts b;
    b.max_tuples = in.max_tuples; b.max_records_per_tuple = in.max_records_per_tuple; b.hash_bits = in.hash_bits;
    try {
        b = bus_audit_checked_opts(b);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(link_audit_renamed(e.what()));
    }
    LinkAuditOpts o;
    o.max_tuples = b.max_tuples; o.max_records_per_tuple = b.max_records_per_tuple; o.hash_bits = b.hash_bits;
    return o;
}
// The bus audit's plan under this audit's name, and the one refusal of its own: a bus wider than the tuple mask
inline BusPlan link_audit_plan(const MachineDesc& machine, const std::vector<BusShape>& main, const std::vector<int>& prep_chips, const std::vector<BusShape>& prep,
                               std::vector<int>& prep_slot) {
    try {
        BusPlan p = bus_audit_plan(machine, main, prep_chips, prep, prep_slot);
        for (auto& b : p.buses)
            if (b.width > LA_MAX_WIDTH)
                throw std::invalid_argument("link_audit: bus (" + std::to_string(b.is_global) + ", " + std::to_string(b.bus_index) + ") is " + std::to_string(b.width) +
                                            " fields wide; a tuple's mask is one 32-bit word, one bit per position: at most " + std::to_string(LA_MAX_WIDTH) + " fields (" +
                                            std::to_string(b.width) + " - " + std::to_string(LA_MAX_WIDTH) + " = " + std::to_string(b.width - LA_MAX_WIDTH) + " too many)");
        return p;
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(link_audit_renamed(e.what()));
    }
}

// The report before any row is looked at: buses, interactions and the constant flags (the field audit's: from the weight rows)
inline void link_audit_blocks(LinkReport& rep, const MachineDesc& machine, const BusPlan& plan) {
    rep.buses.clear();
    for (auto& b : plan.buses) {
        LinkBusStat s;
        s.is_global = b.is_global; s.bus_index = b.bus_index; s.width = b.width;
        s.open_in.assign(b.width, 0); s.open_records.assign(b.width, 0);
        rep.buses.push_back(std::move(s));
    }
    rep.chips.assign(machine.airs.size(), {});
    for (size_t c = 0; c < machine.airs.size(); c++) {
        FieldChipStat cs;
        field_audit_chip_block(cs, machine.airs[c], plan.chips[c].height, true, ra_weight_rows(machine.airs[c]));
        for (auto& f : cs.interactions) {
            LinkInteractionStat s;
            s.is_send = f.is_send; s.is_global = f.is_global; s.bus_index = f.bus_index; s.n_fields = f.n_fields;
            s.constant = f.constant; s.floating.assign(f.n_fields, 0); s.open.assign(f.n_fields, 0);
            rep.chips[c].push_back(std::move(s));
        }
    }
}

inline void link_audit_finish(LinkReport& r, const LinkAuditOpts& o) {
    (void)o;
    r.truncated = r.total_open > r.tuples.size();
}

// The contract on the host, literally: the field audit's masks per record, the bus audit's records sorted by full padded tuple, AND per tuple.
inline LinkReport link_audit_host(const MachineDesc& machine, const std::vector<ConstraintHostMatrix>& main, const std::vector<int>& prep_chips,
                                  const std::vector<ConstraintHostMatrix>& prep, const LinkAuditOpts& opts_in) {
    const LinkAuditOpts o = link_audit_checked_opts(opts_in);
    std::vector<BusShape> ms, ps;
    std::vector<BusHostMatrix> bm, bp;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("link_audit: null trace"); ms.push_back({m.height, m.width}); bm.push_back({m.data, m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("link_audit: null trace"); ps.push_back({m.height, m.width}); bp.push_back({m.data, m.height, m.width}); }
    std::vector<int> prep_slot;
    const BusPlan plan = link_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    LinkReport rep;
    link_audit_blocks(rep, machine, plan);

    // the masks: slot = record id (a chip the field audit skips — no column — has only constant fields: mask 0)
    std::vector<uint32_t> mask((size_t)plan.n_slots, 0);
    const FieldRecordFn on_record = [&](uint32_t chip, uint64_t row, uint32_t m, uint32_t fm) {
        mask[(size_t)(plan.chips[chip].first_id + row * plan.chips[chip].M + m)] = fm;
    };
    try {
        RankAuditOpts fo;
        fo.max_entries = 1; fo.max_rows_per_entry = 1;
        const FieldReport fr = field_audit_host(machine, main, prep_chips, prep, fo, &on_record);
        rep.evaluations = fr.evaluations;
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(link_audit_renamed(e.what()));
    }

    std::vector<BusStat> stats = plan.buses;
    const BusHostRecords recs = bus_audit_host_records(machine, plan, bm, bp, prep_slot, stats);
    struct Open { uint64_t first_id; uint32_t bus; size_t lo, hi; uint32_t mask; uint64_t ns, nr; };
    std::vector<Open> open;
    for (size_t b = 0; b < plan.buses.size(); b++) {
        const BusHostRecords::PerBus& pb = recs.per[b];
        const std::vector<uint32_t>& idx = recs.order[b];
        const uint32_t W = plan.buses[b].width;
        const uint32_t* f = pb.fields.data();
        LinkBusStat& bs = rep.buses[b];
        bs.live = stats[b].live;
        for (size_t lo = 0; lo < idx.size();) {
            size_t hi = lo + 1;
            while (hi < idx.size() && (W == 0 || memcmp(f + (size_t)idx[lo] * W, f + (size_t)idx[hi] * W, (size_t)W * 4) == 0)) hi++;
            uint32_t tm = 0xffffffffu;
            uint64_t ns = 0, nr = 0;
            for (size_t k = lo; k < hi; k++) { tm &= mask[(size_t)pb.id[idx[k]]]; (pb.send[idx[k]] ? ns : nr)++; }
            bs.tuples++;
            if (tm) {
                bs.open_tuples++;
                for (uint32_t j = 0; j < W; j++)
                    if ((tm >> j) & 1u) { bs.open_in[j]++; bs.open_records[j] += hi - lo; }
                open.push_back({pb.id[idx[lo]], (uint32_t)b, lo, hi, tm, ns, nr});
            }
            for (size_t k = lo; k < hi; k++) {
                const BusRecord r = plan.decode(pb.id[idx[k]]);
                LinkInteractionStat& s = rep.chips[r.chip][r.interaction];
                const uint32_t fm = mask[(size_t)pb.id[idx[k]]];
                s.live_rows++;
                for (uint32_t j = 0; j < s.n_fields && j < LA_MAX_WIDTH; j++) {
                    if ((fm >> j) & 1u) s.floating[j]++;
                    if ((fm & tm) >> j & 1u) s.open[j]++;
                }
            }
            lo = hi;
        }
    }
    std::sort(open.begin(), open.end(), [](const Open& x, const Open& y) { return x.first_id < y.first_id; });
    rep.total_open = open.size();
    for (size_t t = 0; t < open.size() && t < o.max_tuples; t++) {
        const Open& u = open[t];
        const BusHostRecords::PerBus& pb = recs.per[u.bus];
        const std::vector<uint32_t>& idx = recs.order[u.bus];
        const uint32_t W = plan.buses[u.bus].width;
        LinkTuple lt;
        lt.is_global = plan.buses[u.bus].is_global; lt.bus_index = plan.buses[u.bus].bus_index; lt.mask = u.mask;
        lt.fields.assign(pb.fields.begin() + (size_t)idx[u.lo] * W, pb.fields.begin() + (size_t)idx[u.lo] * W + W);
        lt.n_send = u.ns; lt.n_recv = u.nr;
        for (size_t k = u.lo; k < u.hi && k - u.lo < o.max_records_per_tuple; k++) {
            const BusRecord r = plan.decode(pb.id[idx[k]]);
            lt.records.push_back(LinkRecord{r.chip, r.row, r.interaction, (uint32_t)pb.send[idx[k]], mask[(size_t)pb.id[idx[k]]]});
        }
        rep.tuples.push_back(std::move(lt));
    }
    link_audit_finish(rep, o);
    return rep;
}

}  // namespace vhost
