// The domain-audit kernels of valida_amd/csrc/kernels/domain_audit.hip — the very source, with the rank audit's scan kernel — compiled for the
// HOST under tools/hipemu and run on host traces: the scan of every virtual column (slices of 256-row tiles merging through the bitmaps and the
// totals as they do in device memory), the classification, the guard pass, the scan over workgroups and the listing pass, driven as
// Prover::domain_audit drives them and assembled by the same host code into the report's word image (tests/test_domain_audit_cpu.py compares it
// with the host audit).  A workgroup has its 256 threads and four waves here; the wave primitives get emulation forms: a ballot and a shuffle go
// through the wave's LDS words between __syncthreads() (every call site is workgroup-uniform).  machine = 0: the BasicMachine; 1: the needle
// machine of tests/domain_audit_cases.py (bus: its bus index); 2: its edge machine.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
#define VGPU_DA_WAVE_PRIMS 1
namespace vk {
uint32_t ra_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
uint32_t da_lds[40 * 1024];
inline unsigned long long ra_ballot(bool pred, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) { slot[0] = 0; slot[1] = 0; }
    __syncthreads();
    if (pred) slot[lane >> 5] |= 1u << (lane & 31u);
    __syncthreads();
    const unsigned long long r = (unsigned long long)slot[0] | ((unsigned long long)slot[1] << 32);
    __syncthreads();
    return r;
}
inline void ra_wave_sync() { __syncthreads(); }
inline unsigned long long da_ballot(bool pred, uint32_t* slot) { return ra_ballot(pred, slot); }
inline uint32_t da_shfl(uint32_t v, uint32_t src, uint32_t* slot) {
    slot[2 + (threadIdx.x & 63u)] = v;
    __syncthreads();
    const uint32_t r = slot[2 + src];
    __syncthreads();
    return r;
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/rank_audit.hip"
#include "../../valida_amd/csrc/kernels/domain_audit.hip"
#include "../../valida_amd/csrc/host/domain_audit.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using namespace vhost;

namespace {
std::vector<uint32_t> working(const uint32_t* m, uint64_t h, uint64_t w) {  // column-major Montgomery: the prover's working layout
    std::vector<uint32_t> c(h * w);
    for (uint64_t r = 0; r < h; r++)
        for (uint64_t k = 0; k < w; k++) c[k * h + r] = vg::Fp::from_canonical(m[r * w + k]).v;
    return c;
}

AirDesc captured(const char* name, int width, std::vector<vair::Interaction> its) {
    vair::Dag d;
    d.width = width; d.prep_width = 0;
    return MachineDesc::make_air_from_dag(name, d, std::move(its));
}
vair::Interaction interaction(bool send, int bus, std::vector<vair::VirtualCol> fields, vair::VirtualCol count) {
    vair::Interaction it;
    it.fields = std::move(fields); it.count = std::move(count); it.bus_kind = vair::BusKind::Global; it.bus_index = bus;
    it.type = send ? vair::InteractionType::GlobalSend : vair::InteractionType::GlobalReceive;
    return it;
}
MachineDesc machine_of(uint32_t kind, uint32_t bus) {
    using V = vair::VirtualCol;
    if (kind == 0) return MachineDesc::basic();
    MachineDesc m;
    if (kind == 1) {
        m.airs.push_back(captured("user", 3, {interaction(true, (int)bus, {V::single_main(0)}, V::single_main(1))}));
        m.airs.push_back(captured("table", 2, {interaction(false, (int)bus, {V::single_main(0)}, V::single_main(1))}));
    } else {
        m.airs.push_back(captured("edge", 3, {interaction(true, 0, {V::single_main(0), V::new_main({{0, 2}, {2, 1}}, 7)}, V::single_main(1))}));
    }
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces); max_slices: the most slices of a virtual column's scan (the device
// pass uses 2048).  out: the report's word image.  Returns the words written, or -1.
int64_t emu_domain_audit(uint32_t machine_kind, uint32_t bus, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                         const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t max_slices, uint32_t max_entries, uint32_t R, uint32_t chip_mask,
                         uint32_t max_bits, uint32_t* out, uint64_t cap) {
    try {
        MachineDesc machine = machine_of(machine_kind, bus);
        for (AirDesc& a : machine.airs)
            if (a.interaction_words.empty()) a.interaction_words = vk::encode_interactions(a.interactions);
        DomainAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask; o.max_bits = max_bits;
        o = domain_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        const DomainPlan plan = domain_audit_plan(machine, ms, chips, ps, o);
        const size_t NC = machine.airs.size();
        DomainReport rep;
        domain_audit_blocks(rep, machine, plan, ms, o);
        std::vector<uint32_t> slot0;
        const uint32_t n_slots = domain_audit_slots(machine, plan, o, slot0);
        std::vector<vk::DaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), vt(NC), gt(NC), table(NC), prefix(NC);
        std::vector<std::vector<unsigned long long>> gtot(NC);
        std::vector<unsigned long long> tot((size_t)n_slots * vk::DA_TOT + 1, 0);
        std::vector<uint32_t> bitmaps((size_t)n_slots * vk::DA_BITMAP_WORDS + 1, 0), cls((size_t)n_slots * vk::DA_CLS + 1, 0xdeadbeefu);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::DaArgs& a = args[i];
            a = vk::DaArgs{};
            a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            vk::da_shape(a, max_slices);
            const bool audited = rep.chips[i].audited && air.width;
            vt[i] = domain_audit_vt(air, plan.chips[i], audited, slot0[i]);
            a.NV = (uint32_t)(vt[i].size() / 4);
            a.vt = vt[i].data();
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i];
            if (plan.prep_slot[i] >= 0) { const int k = plan.prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols[i].data(); a.pstride = ph[k]; }
            a.iw = air.interaction_words.data();
            if (!audited) { a.width = 0; continue; }
            gt[i] = domain_audit_gt(air, plan.chips[i]);
            a.gt = gt[i].data(); a.GW = (uint32_t)gt[i].size(); a.A = (uint32_t)plan.chips[i].apps.size(); a.slot0 = slot0[i];
            gtot[i].assign(5 * (size_t)air.width + a.A, 0);
            table[i].assign((size_t)air.width * a.NB, 0);
            prefix[i].assign((size_t)air.width * a.NB, 0xdeadbeefu);
        }
        for (size_t i = 0; i < NC; i++)
            if (args[i].NV) vk::launch_da_scan(nullptr, args[i], tot.data(), bitmaps.data());
        vk::launch_da_classify(nullptr, tot.data(), bitmaps.data(), cls.data(), n_slots, o.max_bits);
        for (size_t i = 0; i < NC; i++)
            if (args[i].width) vk::launch_da_guard(nullptr, args[i], vk::MA_COUNT, cls.data(), gtot[i].data(), table[i].data(), nullptr, 0, 0, nullptr);
        for (uint32_t p = 0; p < plan.n_positions; p++) {
            if (!tot[(size_t)p * vk::DA_TOT + 4]) continue;
            const uint32_t* k = cls.data() + (size_t)p * vk::DA_CLS;
            DomainPosition& dp = rep.positions[p];
            dp.min = k[5]; dp.max = k[6]; dp.distinct = k[0]; dp.wide = tot[(size_t)p * vk::DA_TOT + 3]; dp.records = tot[(size_t)p * vk::DA_TOT + 4];
        }
        for (size_t i = 0; i < NC; i++) {
            if (!args[i].width) continue;
            DomainChipStat& cs = rep.chips[i];
            const uint32_t W = args[i].width;
            for (uint32_t col = 0; col < W; col++) {
                const uint32_t s = slot0[i] + col;
                const uint32_t* k = cls.data() + (size_t)s * vk::DA_CLS;
                DomainColumn& dc = cs.cols[col];
                dc.distinct = k[0]; dc.cls = k[1]; dc.dense = k[2]; dc.bits = k[3]; dc.narrow = k[4]; dc.min = k[5]; dc.max = k[6];
                dc.nonzero = tot[(size_t)s * vk::DA_TOT + 2]; dc.wide = tot[(size_t)s * vk::DA_TOT + 3];
                dc.guarded = gtot[i][5 * (size_t)col]; dc.sent = gtot[i][5 * (size_t)col + 1]; dc.received = gtot[i][5 * (size_t)col + 2]; dc.mixed = gtot[i][5 * (size_t)col + 3];
                dc.unguarded = args[i].n - dc.guarded;
                const bool walked = dc.narrow || plan.chips[i].item_at[col] != plan.chips[i].item_at[col + 1];
                dc.unguarded_nonzero = walked ? gtot[i][5 * (size_t)col + 4] : dc.nonzero;
            }
            for (uint32_t k = 0; k < args[i].A; k++) cs.app_live[k] = gtot[i][5 * (size_t)W + k];
        }
        domain_audit_entries(rep, plan, o);
        for (size_t e0 = 0; R && e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            const vk::DaArgs& a = args[chip];
            const uint32_t c_cut = rep.entries[e1 - 1].column + 1;
            std::vector<uint32_t> rows((size_t)c_cut * R * 2, 0xdeadbeefu);
            vk::launch_ra_scan(nullptr, vk::da_scan_args(a), table[chip].data(), prefix[chip].data(), c_cut);
            vk::launch_da_guard(nullptr, a, vk::MA_LIST, cls.data(), nullptr, table[chip].data(), prefix[chip].data(), c_cut, R, rows.data());
            for (size_t e = e0; e < e1; e++) {
                DomainEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.unguarded_nonzero, R);
                en.rows.assign(rows.begin() + (size_t)en.column * R * 2, rows.begin() + (size_t)en.column * R * 2 + (size_t)listed * 2);
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        std::copy(w.begin(), w.end(), out);
        return (int64_t)w.size();
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_domain_audit: %s\n", e.what());
        return -1;
    }
}
}
