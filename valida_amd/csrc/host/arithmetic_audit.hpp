// Arithmetic audit: do the ALU records of a witness compute their opcode?  `div`'s eval is a TODO in the reference (chips/basic_machine.hpp
// restates it that way) and the field audit reports all 13 fields of its receive as floating; `shift` delegates to `mul` and `div` on the
// general bus with a power of two as operand; `lt`, `com`, `mul` and `bitwise` are only as tight as their transcribed constraints.  So a
// quotient, or any other ALU result, planted consistently in the ALU chip's row, the cpu's write channel and the memory table passes every other
// audit.  This audit replays the general bus as arithmetic: for each live record (opcode, x, y, z) it recomputes z from x and y in 32-bit integer
// arithmetic and names the records where the stored result differs.
//
// Contract (include/vgpu.h, "Arithmetic audit", states it for the C ABI):
//   inputs    what vgpu_prove and the audits take.  The audited bus is global bus 0 by default (bus_is_global, bus_index name another); sides
//             selects records: bit 0 the receives, bit 1 the sends (default 1).
//   entries   an ENTRY is a (chip, interaction) on that bus and a selected side, in ascending (chip, interaction) order, read through its vcols.
//             Fields 0..12 are opcode, x[0..3], y[0..3], z[0..3], bytes most significant first; fields beyond 12 (a clk) are ignored.
//   records   a SLOT is (entry, row), LIVE iff its count != 0 there (any multiplicity); values canonical.  A live record is JUDGED iff its opcode
//             is in 100..118 (index = opcode - 100), otherwise OTHER: counted, never judged.
//   expected  ADD, SUB, MUL the low word; MULHU and MULHS the UNSIGNED high word of the 64-bit product (the reference zero-extends); DIV the
//             unsigned quotient; SDIV the signed quotient truncated toward zero; SHL, SHR shift by y; SRA shifts by y and replicates the sign;
//             AND, OR, XOR; LT, LTE unsigned, SLT, SLE signed, NE, EQ: a boolean result is the word (0, 0, 0, r).
//   findings  per judged record at most one kind, the first that applies: 1 MALFORMED (some field among 1..12 is >= 256; mask bit j - 1 for
//             field j), 2 UNDEFINED (reason 1: DIV or SDIV with y = 0; 2: SDIV of 0x80000000 by 0xFFFFFFFF; 3: SHL, SHR or SRA with y >= 32:
//             the VM refuses these), none if z is the expected word, 4 SHIFT_QUOTIENT (SDIV, y = 2^k, z = sra(x, k)), 5 ARITHMETIC_SHR (SHR,
//             z = sra(x, y)), 3 WRONG_RESULT otherwise; mask of kinds 3, 4, 5: the differing bytes of z, bit j for z[j].  1, 2, 3 are HARD, 4 and
//             5 SOFT: counted and listed apart, never a fault.
//   counters  exact: slots, live, judged, other, one count per opcode, per kind and per UNDEFINED reason, mulhs_sign_matters (the well-formed
//             MULHS records whose signed high word differs from the unsigned one: counted, never a finding), per entry live and hard.
//   lists     the first max_findings hard findings and the first max_findings soft findings, each in slot order (entry-major, rows ascending);
//             default 64, at most 2^20, 0 lists nothing while every count stays exact.
// What it is not: it judges each record alone and this witness only; whether senders and receivers agree is the bus audit's question; it does
// not read the chips' auxiliary columns and says nothing about the cpu's flags, pc or fp.
// This header holds the options check, the plan, the report with its image "VAR1" and the host twin (plain C++, one thread).  The rule for one
// record is kernels/arithmetic_rule.hpp, shared with the device pass, Prover::arithmetic_audit (prover_audits.cpp, kernels/arithmetic_audit.hip).
#pragma once
#include "bus_audit.hpp"
#include "../kernels/arithmetic_rule.hpp"

namespace vhost {

struct ArithmeticAuditOpts {
    uint32_t max_findings = 64;
    uint32_t bus_is_global = 1, bus_index = 0;
    uint32_t sides = 1;
    uint32_t reserved = 0;
};

constexpr uint32_t AR_FIELDS = 13;

struct ArithmeticFinding {
    uint32_t kind = 0, mask = 0, chip = 0, interaction = 0, row = 0, opcode = 0;
    uint32_t f[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // x[0..3], y[0..3], z[0..3]
    uint32_t expected = 0, count = 0, is_send = 0;
};

struct ArithmeticEntry {
    uint32_t chip = 0, interaction = 0, is_send = 0, n_fields = 0;
    uint64_t live = 0, hard = 0;
};

struct ArithmeticReport {
    uint32_t is_global = 1, bus_index = 0, sides = 1, max_findings = 64;
    std::vector<ArithmeticEntry> entries;
    uint64_t slots = 0, live = 0, judged = 0, other = 0, kinds[5] = {0, 0, 0, 0, 0}, mulhs_sign_matters = 0, reasons[3] = {0, 0, 0};
    uint64_t opcodes[vk::AR_OPCODES] = {};
    std::vector<ArithmeticFinding> hard_list, soft_list;
    double device_ms = 0, host_ms = 0, evaluations = 0;  // evaluations: the live records
    static constexpr uint32_t MAGIC = 0x31524156u;        // "VAR1"
    static constexpr uint32_t HEADER = 80, ENTRY_WORDS = 8, FINDING_WORDS = 24;
    uint64_t hard() const { return kinds[0] + kinds[1] + kinds[2]; }
    uint64_t soft() const { return kinds[3] + kinds[4]; }
    std::vector<uint32_t> words() const {
        std::vector<uint32_t> w;
        auto u64 = [&](uint64_t v) { w.push_back((uint32_t)v); w.push_back((uint32_t)(v >> 32)); };
        w.push_back(MAGIC); w.push_back(0); w.push_back(is_global); w.push_back(bus_index); w.push_back(sides);
        w.push_back((hard() > hard_list.size() ? 1u : 0u) | (soft() > soft_list.size() ? 2u : 0u));
        w.push_back((uint32_t)hard_list.size()); w.push_back((uint32_t)soft_list.size()); w.push_back(max_findings); w.push_back((uint32_t)entries.size());
        u64(slots); u64(live); u64(judged); u64(other);
        u64(hard()); u64(kinds[0]); u64(kinds[1]); u64(kinds[2]); u64(soft()); u64(kinds[3]); u64(kinds[4]);
        u64(mulhs_sign_matters);
        for (int k = 0; k < 3; k++) u64(reasons[k]);
        for (uint32_t k = 0; k < vk::AR_OPCODES; k++) u64(opcodes[k]);
        u64(0);
        for (auto& e : entries) { w.push_back(e.chip); w.push_back(e.interaction); w.push_back(e.is_send); w.push_back(e.n_fields); u64(e.live); u64(e.hard); }
        for (const auto* list : {&hard_list, &soft_list})
            for (auto& f : *list) {
                w.push_back(f.kind); w.push_back(f.mask); w.push_back(f.chip); w.push_back(f.interaction); w.push_back(f.row); w.push_back(f.opcode);
                for (int k = 0; k < 12; k++) w.push_back(f.f[k]);
                w.push_back(f.expected); w.push_back(f.count); w.push_back(f.is_send);
                for (int k = 0; k < 3; k++) w.push_back(0);
            }
        w[1] = (uint32_t)w.size();
        return w;
    }
};

inline ArithmeticAuditOpts arithmetic_audit_checked_opts(const ArithmeticAuditOpts& o) {
    if (o.max_findings > (1u << 20)) throw std::invalid_argument("arithmetic_audit: max_findings is at most 2^20");
    if (o.bus_is_global > 1) throw std::invalid_argument("arithmetic_audit: bus_is_global is 0 or 1");
    if (o.sides < 1 || o.sides > 3) throw std::invalid_argument("arithmetic_audit: sides is 1 (receives), 2 (sends) or 3 (both), got " + std::to_string(o.sides));
    if (o.reserved) throw std::invalid_argument("arithmetic_audit: reserved must be zero");
    return o;
}

// The entries in ascending (chip, interaction) order; slot = first_slot(entry) + row: integer order is entry-major with rows ascending.
struct ArithmeticPlan {
    struct Entry { uint32_t chip = 0, interaction = 0, is_send = 0, n_fields = 0; uint64_t first_slot = 0, height = 0; };
    std::vector<Entry> entries;
    uint64_t n_slots = 0;
};

// Validates the shapes as the bus audit does (its messages, under this audit's name) and lays out the slots
inline ArithmeticPlan arithmetic_audit_plan(const MachineDesc& machine, const std::vector<BusShape>& main, const std::vector<int>& prep_chips, const std::vector<BusShape>& prep,
                                            std::vector<int>& prep_slot, const ArithmeticAuditOpts& o, BusPlan* bus_plan = nullptr) {
    BusPlan bp;
    try {
        bp = bus_audit_plan(machine, main, prep_chips, prep, prep_slot);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what();
        throw std::invalid_argument("arithmetic_audit" + (m.rfind("bus_audit", 0) == 0 ? m.substr(9) : ": " + m));
    }
    const std::string bus = std::string(o.bus_is_global ? "global" : "local") + " bus " + std::to_string(o.bus_index);
    ArithmeticPlan p;
    for (size_t i = 0; i < machine.airs.size(); i++) {
        const AirDesc& a = machine.airs[i];
        for (size_t m = 0; m < a.interactions.size(); m++) {
            const vair::Interaction& it = a.interactions[m];
            if ((it.is_local() ? 0u : 1u) != o.bus_is_global || (uint32_t)it.bus_index != o.bus_index || !(o.sides & (it.is_send() ? 2u : 1u))) continue;
            if (it.fields.size() < AR_FIELDS)
                throw std::invalid_argument("arithmetic_audit: interaction " + std::to_string(m) + " of chip " + a.name + " has " + std::to_string(it.fields.size()) + " fields on " + bus +
                                            "; an ALU record has at least 13 (opcode, x[0..3], y[0..3], z[0..3])");
            ArithmeticPlan::Entry e;
            e.chip = (uint32_t)i; e.interaction = (uint32_t)m; e.is_send = it.is_send() ? 1u : 0u; e.n_fields = (uint32_t)it.fields.size();
            e.first_slot = p.n_slots; e.height = main[i].height;
            p.n_slots += e.height;
            p.entries.push_back(e);
        }
    }
    if (p.entries.empty())
        throw std::invalid_argument("arithmetic_audit: no chip " + std::string(o.sides == 1 ? "receives" : o.sides == 2 ? "sends" : "sends or receives") + " on " + bus +
                                    ": there is no ALU record to audit");
    if (p.n_slots >= 0xffffffffull) throw std::invalid_argument("arithmetic_audit: more than 2^32 - 2 record slots (" + std::to_string(p.n_slots) + "); slot ids are 32-bit");
    if (bus_plan) *bus_plan = std::move(bp);
    return p;
}

inline void arithmetic_audit_header(ArithmeticReport& rep, const ArithmeticPlan& plan, const ArithmeticAuditOpts& o) {
    rep.is_global = o.bus_is_global; rep.bus_index = o.bus_index; rep.sides = o.sides; rep.max_findings = o.max_findings;
    rep.slots = plan.n_slots;
    for (auto& e : plan.entries) {
        ArithmeticEntry r;
        r.chip = e.chip; r.interaction = e.interaction; r.is_send = e.is_send; r.n_fields = e.n_fields;
        rep.entries.push_back(r);
    }
}

// One verdict into the counters of the report and of its entry
inline void arithmetic_audit_count(ArithmeticReport& rep, ArithmeticEntry& en, uint32_t word) {
    if (!(word & vk::AR_LIVE)) return;
    rep.live++; en.live++;
    if (!(word & vk::AR_JUDGED)) { rep.other++; return; }
    rep.judged++;
    rep.opcodes[vk::ar_index(word)]++;
    if (word & vk::AR_SIGN_MATTERS) rep.mulhs_sign_matters++;
    const uint32_t kind = vk::ar_kind(word);
    if (!kind) return;
    rep.kinds[kind - 1]++;
    if (kind == vk::AR_UNDEFINED) rep.reasons[vk::ar_mask(word) - 1]++;
    if (vk::ar_is_hard(word)) en.hard++;
}

// ---- what the device pass and its emulation share (the layouts are stated in kernels/launch.hpp, arithmetic_audit.hip) ----
// tot: per entry AR_TOT u64 totals; out: the listed records in the image's own layout (24 words each: the hard ones, then the soft ones)
inline void arithmetic_audit_from_device(ArithmeticReport& rep, const unsigned long long* tot, uint32_t tot_stride, const uint32_t* out, size_t listed_hard, size_t listed_soft) {
    for (size_t e = 0; e < rep.entries.size(); e++) {
        const unsigned long long* t = tot + e * tot_stride;
        rep.live += t[0]; rep.judged += t[1]; rep.other += t[2];
        for (int k = 0; k < 5; k++) rep.kinds[k] += t[3 + k];
        rep.mulhs_sign_matters += t[8];
        for (int k = 0; k < 3; k++) rep.reasons[k] += t[9 + k];
        for (uint32_t k = 0; k < vk::AR_OPCODES; k++) rep.opcodes[k] += t[12 + k];
        rep.entries[e].live = t[0]; rep.entries[e].hard = t[3] + t[4] + t[5];
    }
    for (size_t t = 0; t < listed_hard + listed_soft; t++) {
        const uint32_t* o = out + ArithmeticReport::FINDING_WORDS * t;
        ArithmeticFinding f;
        f.kind = o[0]; f.mask = o[1]; f.chip = o[2]; f.interaction = o[3]; f.row = o[4]; f.opcode = o[5];
        for (int k = 0; k < 12; k++) f.f[k] = o[6 + k];
        f.expected = o[18]; f.count = o[19]; f.is_send = o[20];
        (t < listed_hard ? rep.hard_list : rep.soft_list).push_back(f);
    }
    rep.evaluations = (double)rep.live;
}

// The contract on the host: one walk over the slots.
inline ArithmeticReport arithmetic_audit_host(const MachineDesc& machine, const std::vector<BusHostMatrix>& main, const std::vector<int>& prep_chips, const std::vector<BusHostMatrix>& prep,
                                              const ArithmeticAuditOpts& opts_in) {
    const ArithmeticAuditOpts o = arithmetic_audit_checked_opts(opts_in);
    std::vector<BusShape> ms, ps;
    for (auto& m : main) { if (!m.data) throw std::invalid_argument("arithmetic_audit: null trace"); ms.push_back({m.height, m.width}); }
    for (auto& m : prep) { if (!m.data) throw std::invalid_argument("arithmetic_audit: null trace"); ps.push_back({m.height, m.width}); }
    std::vector<int> prep_slot;
    const ArithmeticPlan plan = arithmetic_audit_plan(machine, ms, prep_chips, ps, prep_slot, o);
    ArithmeticReport rep;
    arithmetic_audit_header(rep, plan, o);
    auto eval = [](const vair::VirtualCol& v, const uint32_t* mrow, const uint32_t* prow) {
        uint64_t acc = v.constant % vg::P;
        for (auto& t : v.terms) acc = (acc + (uint64_t)((t.preprocessed ? prow : mrow)[t.col] % vg::P) * (t.weight % vg::P)) % vg::P;
        return (uint32_t)acc;
    };
    for (size_t e = 0; e < plan.entries.size(); e++) {
        const ArithmeticPlan::Entry& pe = plan.entries[e];
        const vair::Interaction& it = machine.airs[pe.chip].interactions[pe.interaction];
        const BusHostMatrix& mm = main[pe.chip];
        const BusHostMatrix* pm = prep_slot[pe.chip] >= 0 ? &prep[(size_t)prep_slot[pe.chip]] : nullptr;
        for (uint64_t r = 0; r < mm.height; r++) {
            const uint32_t* mrow = mm.data + r * mm.width;
            const uint32_t* prow = pm ? pm->data + r * pm->width : nullptr;
            const uint32_t count = eval(it.count, mrow, prow);
            if (!count) continue;
            ArithmeticFinding f;
            f.opcode = eval(it.fields[0], mrow, prow);
            for (int j = 0; j < 12; j++) f.f[j] = eval(it.fields[1 + j], mrow, prow);
            const uint32_t word = vk::ar_judge(count, f.opcode, f.f, &f.expected);
            arithmetic_audit_count(rep, rep.entries[e], word);
            if (!vk::ar_kind(word)) continue;
            std::vector<ArithmeticFinding>& list = vk::ar_is_hard(word) ? rep.hard_list : rep.soft_list;
            if (list.size() >= o.max_findings) continue;
            f.kind = vk::ar_kind(word); f.mask = vk::ar_mask(word); f.chip = pe.chip; f.interaction = pe.interaction; f.row = (uint32_t)r; f.count = count; f.is_send = pe.is_send;
            if (f.kind <= vk::AR_UNDEFINED) f.expected = 0;
            list.push_back(f);
        }
    }
    rep.evaluations = (double)rep.live;
    return rep;
}

}  // namespace vhost
