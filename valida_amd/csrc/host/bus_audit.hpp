// Bus audit: the exact, challenge-free form of check_cumulative_sums (basic/src/lib.rs:373-375) over a full witness.
// Every (chip, row, interaction) of Chip::all_interactions order (machine/src/chip.rs:40-63) whose count is non-zero is a RECORD; records
// of one bus carry the same TUPLE when their fields agree after zero-padding to the widest interaction of that bus (the permutation
// argument reduces a tuple as sum_j f_j beta^j, machine/src/chip.rs:121-208, so a trailing zero field is invisible to it); a tuple is
// unbalanced when its sends minus its receives are non-zero in F_p.  This header holds what the host and the device implementation
// share — the plan (record ids, bus table, the device descriptor), the report and its flat word image — and the host implementation of
// the contract over host matrices (plain C++, no device).  The device pass is Prover::bus_audit (prover_audits.cpp, kernels/bus_audit.hip).
#pragma once
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "machine.hpp"

namespace vhost {

struct BusAuditOpts {
    uint64_t max_tuples = 64;
    uint32_t max_records_per_tuple = 4;
    uint32_t hash_bits = 64;  // test hook: the device's grouping key is cut to this many bits (the report must not change)
};

struct BusRecord { uint32_t chip, row, interaction, is_send, count; };
struct BusTuple {
    uint32_t is_global = 0, bus_index = 0;
    std::vector<uint32_t> fields;  // padded to the bus's width
    uint32_t net = 0, send_sum = 0, recv_sum = 0;  // canonical
    uint64_t n_send = 0, n_recv = 0;
    std::vector<BusRecord> records;  // the first max_records_per_tuple in record order
};
struct BusStat { uint32_t is_global = 0, bus_index = 0, width = 0; uint64_t live = 0, sends = 0, receives = 0, unbalanced = 0; };
struct BusReport {
    bool balanced = true, truncated = false;
    uint64_t total_unbalanced = 0;
    std::vector<BusStat> buses;    // ascending (is_global, bus_index)
    std::vector<BusTuple> tuples;  // ascending by first record
    double device_ms = 0;          // the device pass (0 for the host implementation); not part of the word image
    double host_ms = 0;            // wall time of the whole call
    static constexpr uint32_t MAGIC = 0x31524256u;  // "VBR1"
    // Flat image (include/vgpu.h documents it next to vgpu_bus_report_words)
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0);
        w.push_back(balanced ? 1u : 0u); w.push_back(truncated ? 1u : 0u);
        u64(total_unbalanced);
        w.push_back((uint32_t)tuples.size()); w.push_back((uint32_t)buses.size());
        for (auto& b : buses) {
            w.push_back(b.is_global); w.push_back(b.bus_index); w.push_back(b.width); w.push_back(0);
            u64(b.live); u64(b.sends); u64(b.receives); u64(b.unbalanced);
        }
        for (auto& t : tuples) {
            w.push_back(t.is_global); w.push_back(t.bus_index); w.push_back((uint32_t)t.fields.size()); w.push_back(t.net);
            w.push_back(t.send_sum); w.push_back(t.recv_sum);
            u64(t.n_send); u64(t.n_recv);
            w.push_back((uint32_t)t.records.size());
            for (uint32_t f : t.fields) w.push_back(f);
            for (auto& r : t.records) { w.push_back(r.chip); w.push_back(r.row); w.push_back(r.interaction); w.push_back(r.is_send); w.push_back(r.count); }
        }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

// Layout of the device descriptor (u32 words; constants and weights in Montgomery form, vk::encode_vcol):
//   [0] n_chips [1] n_buses [2] widest bus [3] offset of the bus table
//   chip c at BA_HDR + c * BA_CHIP_WORDS: [0] first record id [1] height [2] M [3] offset of its interaction table
//                                         [4,5] main column 0 (device pointer) [6] main stride [7,8] preprocessed column 0 [9] its stride
//   interaction m of a chip at its table + 4 m: [0] offset of its vcols (count, then the fields) [1] is_send [2] bus slot [3] n_fields
//   bus slot b at the bus table + 2 b: [0] width [1] is_global << 31 | bus_index
// A record id is first_id(chip) + row * M(chip) + interaction: integer order is record order.
constexpr uint32_t BA_HDR = 4, BA_CHIP_WORDS = 12;

struct BusPlan {
    struct Chip { uint64_t first_id = 0, height = 0; uint32_t M = 0; std::vector<uint32_t> bus_slot; };
    std::vector<Chip> chips;
    std::vector<BusStat> buses;  // slot order = ascending (is_global, bus_index)
    uint64_t n_slots = 0;
    uint32_t wmax = 0;

    int slot_of(uint32_t is_global, uint32_t bus_index) const {
        for (size_t b = 0; b < buses.size(); b++) if (buses[b].is_global == is_global && buses[b].bus_index == bus_index) return (int)b;
        return -1;
    }
    // (chip, row, interaction) of a record id
    BusRecord decode(uint64_t id) const {
        size_t c = 0;
        while (c + 1 < chips.size() && chips[c + 1].first_id <= id) c++;
        const uint64_t off = id - chips[c].first_id;
        return BusRecord{(uint32_t)c, (uint32_t)(off / chips[c].M), (uint32_t)(off % chips[c].M), 0, 0};
    }
};

struct BusShape { uint64_t height, width; };

inline BusAuditOpts bus_audit_checked_opts(const BusAuditOpts& in) {
    BusAuditOpts o = in;
    if (o.max_tuples == 0) o.max_tuples = 64;
    if (o.max_records_per_tuple == 0) o.max_records_per_tuple = 4;
    if (o.hash_bits == 0) o.hash_bits = 64;
    if (o.hash_bits > 64) throw std::invalid_argument("bus_audit: hash_bits must be 1..64 (0 selects the default, 64)");
    if (o.max_tuples > (1ull << 24) || o.max_records_per_tuple > 4096) throw std::invalid_argument("bus_audit: max_tuples is at most 2^24 and max_records_per_tuple at most 4096");
    return o;
}

// Validates the shapes exactly as prove does (one main trace per chip, widths, power-of-two heights, preprocessed traces for exactly the
// chips that have preprocessed columns) and lays out record ids and buses.  prep_slot[chip] = index into the preprocessed list or -1.
inline BusPlan bus_audit_plan(const MachineDesc& machine, const std::vector<BusShape>& main, const std::vector<int>& prep_chips, const std::vector<BusShape>& prep,
                              std::vector<int>& prep_slot) {
    const size_t NC = machine.airs.size();
    if (main.size() != NC) throw std::invalid_argument("bus_audit: need one main trace per chip (" + std::to_string(NC) + "), got " + std::to_string(main.size()));
    prep_slot.assign(NC, -1);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& a = machine.airs[i];
        if (main[i].width != a.width) throw std::invalid_argument("bus_audit: trace width mismatch for chip " + a.name + " (" + std::to_string(main[i].width) + ", expected " + std::to_string(a.width) + ")");
        const uint64_t h = main[i].height;
        if (h == 0 || (h & (h - 1)) || h > (1ull << 27)) throw std::invalid_argument("bus_audit: trace heights must be powers of two up to 2^27 (chip " + a.name + ": " + std::to_string(h) + ")");
    }
    for (size_t k = 0; k < prep_chips.size(); k++) {
        const int chip = prep_chips[k];
        if (chip < 0 || (size_t)chip >= NC || prep_slot[chip] >= 0) throw std::invalid_argument("bus_audit: bad or repeated preprocessed chip index");
        if (machine.airs[chip].prep_width == 0) throw std::invalid_argument("bus_audit: chip " + machine.airs[chip].name + " has no preprocessed columns");
        if (prep[k].width != machine.airs[chip].prep_width || prep[k].height != main[chip].height) throw std::invalid_argument("bus_audit: preprocessed trace shape mismatch for chip " + machine.airs[chip].name);
        prep_slot[chip] = (int)k;
    }
    BusPlan p;
    std::vector<std::pair<uint32_t, uint32_t>> keys;
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& a = machine.airs[i];
        if (a.prep_width && prep_slot[i] < 0) throw std::invalid_argument("bus_audit: chip " + a.name + " needs its preprocessed trace");
        for (auto& it : a.interactions) {
            auto check = [&](const vair::VirtualCol& v) {
                for (auto& t : v.terms)
                    if (t.col < 0 || (uint32_t)t.col >= (t.preprocessed ? a.prep_width : a.width)) throw std::invalid_argument("bus_audit: an interaction of chip " + a.name + " reads a column outside its trace");
            };
            check(it.count);
            for (auto& f : it.fields) check(f);
            keys.emplace_back(it.is_local() ? 0u : 1u, (uint32_t)it.bus_index);
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (auto& k : keys) { BusStat b; b.is_global = k.first; b.bus_index = k.second; p.buses.push_back(b); }
    p.chips.resize(NC);
    for (size_t i = 0; i < NC; i++) {
        const AirDesc& a = machine.airs[i];
        BusPlan::Chip& c = p.chips[i];
        c.first_id = p.n_slots; c.height = main[i].height; c.M = (uint32_t)a.interactions.size();
        for (auto& it : a.interactions) {
            const int b = p.slot_of(it.is_local() ? 0u : 1u, (uint32_t)it.bus_index);
            c.bus_slot.push_back((uint32_t)b);
            p.buses[b].width = std::max<uint32_t>(p.buses[b].width, (uint32_t)it.fields.size());
        }
        p.n_slots += c.height * c.M;
    }
    for (auto& b : p.buses) p.wmax = std::max(p.wmax, b.width);
    return p;
}

// The descriptor of the layout above; main_ptr / prep_ptr: device column-major views per chip (prep may be null)
inline std::vector<uint32_t> bus_audit_descriptor(const MachineDesc& machine, const BusPlan& p, const std::vector<const uint32_t*>& main_ptr, const std::vector<uint64_t>& main_stride,
                                                  const std::vector<const uint32_t*>& prep_ptr, const std::vector<uint64_t>& prep_stride) {
    const uint32_t NC = (uint32_t)machine.airs.size();
    std::vector<uint32_t> w(BA_HDR + (size_t)NC * BA_CHIP_WORDS, 0);
    w[0] = NC; w[1] = (uint32_t)p.buses.size(); w[2] = p.wmax;
    for (uint32_t c = 0; c < NC; c++) {
        const size_t tab = w.size();
        const uint32_t M = p.chips[c].M;
        w.resize(tab + 4 * (size_t)M);
        for (uint32_t m = 0; m < M; m++) {
            const vair::Interaction& it = machine.airs[c].interactions[m];
            w[tab + 4 * m] = (uint32_t)w.size();
            w[tab + 4 * m + 1] = it.is_send() ? 1u : 0u;
            w[tab + 4 * m + 2] = p.chips[c].bus_slot[m];
            w[tab + 4 * m + 3] = (uint32_t)it.fields.size();
            vk::encode_vcol(w, it.count);
            for (auto& f : it.fields) vk::encode_vcol(w, f);
        }
        uint32_t* e = w.data() + BA_HDR + (size_t)c * BA_CHIP_WORDS;
        e[0] = (uint32_t)p.chips[c].first_id; e[1] = (uint32_t)p.chips[c].height; e[2] = M; e[3] = (uint32_t)tab;
        const uint64_t mp = (uint64_t)main_ptr[c], pp = (uint64_t)prep_ptr[c];
        e[4] = (uint32_t)mp; e[5] = (uint32_t)(mp >> 32); e[6] = (uint32_t)main_stride[c];
        e[7] = (uint32_t)pp; e[8] = (uint32_t)(pp >> 32); e[9] = (uint32_t)prep_stride[c];
    }
    w[3] = (uint32_t)w.size();
    for (auto& b : p.buses) { w.push_back(b.width); w.push_back((b.is_global << 31) | b.bus_index); }
    return w;
}

inline void bus_audit_finish(BusReport& r, const BusAuditOpts& o) {
    r.balanced = r.total_unbalanced == 0;
    r.truncated = r.total_unbalanced > r.tuples.size();
    (void)o;
}

struct BusHostMatrix { const uint32_t* data; uint64_t height, width; };  // canonical row-major (the reference's RowMajorMatrix<Val>)

// Every live record of the witness per bus slot, in record order, with its tuple padded to the bus's width, and per bus the order that makes
// equal tuples adjacent (ties in record order): what bus_audit_host reduces and the link audit joins (host/link_audit.hpp).  Adds the records to
// live / sends / receives of `stats` (one entry per bus slot).
struct BusHostRecords {
    struct PerBus { std::vector<uint32_t> fields; std::vector<uint64_t> id; std::vector<uint32_t> cnt; std::vector<uint8_t> send; };
    std::vector<PerBus> per;
    std::vector<std::vector<uint32_t>> order;
};
inline BusHostRecords bus_audit_host_records(const MachineDesc& machine, const BusPlan& plan, const std::vector<BusHostMatrix>& main, const std::vector<BusHostMatrix>& prep,
                                             const std::vector<int>& prep_slot, std::vector<BusStat>& stats) {
    const size_t NB = plan.buses.size();
    using PerBus = BusHostRecords::PerBus;
    BusHostRecords out;
    out.per.resize(NB);
    out.order.resize(NB);
    std::vector<PerBus>& per = out.per;
    auto eval = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* prow) {
        uint64_t acc = v.constant % vg::P;
        for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? prow : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
        return (uint32_t)acc;
    };
    for (size_t c = 0; c < machine.airs.size(); c++) {
        const AirDesc& a = machine.airs[c];
        const uint32_t M = plan.chips[c].M;
        if (!M) continue;
        const BusHostMatrix& mm = main[c];
        const BusHostMatrix* pm = prep_slot[c] >= 0 ? &prep[prep_slot[c]] : nullptr;
        for (uint64_t r = 0; r < mm.height; r++) {
            const uint32_t* mrow = mm.data + r * mm.width;
            const uint32_t* prow = pm ? pm->data + r * pm->width : nullptr;
            for (uint32_t m = 0; m < M; m++) {
                const vair::Interaction& it = a.interactions[m];
                const uint32_t cnt = eval(it.count, mrow, prow);
                if (!cnt) continue;
                const uint32_t b = plan.chips[c].bus_slot[m];
                PerBus& pb = per[b];
                const uint32_t W = plan.buses[b].width;
                const size_t at = pb.fields.size();
                pb.fields.resize(at + W, 0);
                for (size_t j = 0; j < it.fields.size(); j++) pb.fields[at + j] = eval(it.fields[j], mrow, prow);
                pb.id.push_back(plan.chips[c].first_id + r * M + m);
                pb.cnt.push_back(cnt);
                pb.send.push_back(it.is_send() ? 1 : 0);
                stats[b].live++;
                (it.is_send() ? stats[b].sends : stats[b].receives)++;
            }
        }
    }
    std::vector<std::vector<uint32_t>>& order = out.order;
    for (size_t b = 0; b < NB; b++) {
        PerBus& pb = per[b];
        const uint32_t W = plan.buses[b].width;
        std::vector<uint32_t>& idx = order[b];
        idx.resize(pb.id.size());
        for (size_t i = 0; i < idx.size(); i++) idx[i] = (uint32_t)i;
        const uint32_t* f = pb.fields.data();
        // records were appended in record order, so the index breaks ties in record order
        std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
            const int c = W ? memcmp(f + (size_t)x * W, f + (size_t)y * W, (size_t)W * 4) : 0;  // any total order on tuples groups them
            return c != 0 ? c < 0 : x < y;
        });
    }
    return out;
}

// The contract on the host: evaluate, sort, reduce.  One thread; exact by construction (records are grouped by their full tuples).
inline BusReport bus_audit_host(const MachineDesc& machine, const std::vector<BusHostMatrix>& main, const std::vector<int>& prep_chips,
                                const std::vector<BusHostMatrix>& prep, const BusAuditOpts& opts_in) {
    const BusAuditOpts o = bus_audit_checked_opts(opts_in);
    std::vector<BusShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("bus_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("bus_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    const BusPlan plan = bus_audit_plan(machine, ms, prep_chips, ps, prep_slot);
    const size_t NB = plan.buses.size();
    BusReport rep;
    rep.buses = plan.buses;
    const BusHostRecords recs = bus_audit_host_records(machine, plan, main, prep, prep_slot, rep.buses);
    using PerBus = BusHostRecords::PerBus;
    const std::vector<PerBus>& per = recs.per;
    const std::vector<std::vector<uint32_t>>& order = recs.order;
    struct Unb { uint64_t first_id; uint32_t bus; size_t lo, hi; uint32_t send, recv; uint64_t ns, nr; };
    std::vector<Unb> unb;
    for (size_t b = 0; b < NB; b++) {
        const PerBus& pb = per[b];
        const std::vector<uint32_t>& idx = order[b];
        const uint32_t W = plan.buses[b].width;
        const uint32_t* f = pb.fields.data();
        for (size_t lo = 0; lo < idx.size();) {
            size_t hi = lo + 1;
            while (hi < idx.size() && (W == 0 || memcmp(f + (size_t)idx[lo] * W, f + (size_t)idx[hi] * W, (size_t)W * 4) == 0)) hi++;
            uint64_t s = 0, r = 0, ns = 0, nr = 0;
            for (size_t k = lo; k < hi; k++) { if (pb.send[idx[k]]) { s += pb.cnt[idx[k]]; ns++; } else { r += pb.cnt[idx[k]]; nr++; } }
            const uint32_t sm = (uint32_t)(s % vg::P), rm = (uint32_t)(r % vg::P);
            if (sm != rm) { unb.push_back({pb.id[idx[lo]], (uint32_t)b, lo, hi, sm, rm, ns, nr}); rep.buses[b].unbalanced++; }
            lo = hi;
        }
    }
    std::sort(unb.begin(), unb.end(), [](const Unb& x, const Unb& y) { return x.first_id < y.first_id; });
    rep.total_unbalanced = unb.size();
    for (size_t t = 0; t < unb.size() && t < o.max_tuples; t++) {
        const Unb& u = unb[t];
        const PerBus& pb = per[u.bus];
        const uint32_t W = plan.buses[u.bus].width;
        BusTuple bt;
        bt.is_global = plan.buses[u.bus].is_global; bt.bus_index = plan.buses[u.bus].bus_index;
        bt.fields.assign(pb.fields.begin() + (size_t)order[u.bus][u.lo] * W, pb.fields.begin() + (size_t)order[u.bus][u.lo] * W + W);
        bt.send_sum = u.send; bt.recv_sum = u.recv; bt.net = (u.send + vg::P - u.recv) % vg::P;
        bt.n_send = u.ns; bt.n_recv = u.nr;
        for (size_t k = u.lo; k < u.hi && k - u.lo < o.max_records_per_tuple; k++) {
            const uint32_t i = order[u.bus][k];
            BusRecord r = plan.decode(pb.id[i]);
            r.is_send = pb.send[i]; r.count = pb.cnt[i];
            bt.records.push_back(r);
        }
        rep.tuples.push_back(std::move(bt));
    }
    bus_audit_finish(rep, o);
    return rep;
}

}  // namespace vhost
