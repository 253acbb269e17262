// The arithmetic-audit kernels of valida_amd/csrc/kernels/arithmetic_audit.hip — the very source, with the memory audit's one-workgroup scan
// they launch — compiled for the HOST under tools/hipemu and run on host traces, driven as Prover::arithmetic_audit drives them and assembled by
// the same host code into the report's word image (tests/test_arithmetic_audit_cpu.py compares it with the host audit): the judge's descriptor
// walk, verdict words, ballots and LDS counters, the two workgroup tables across entries, their scans and the listing pass.  A workgroup has its
// 256 threads and four waves here; the wave primitives get emulation forms: a ballot goes through the wave's LDS words between __syncthreads()
// (every call site is workgroup-uniform).  machine = 0: the BasicMachine; 1: the `alu` machine of tests/arithmetic_audit_cases.py; 2: its
// `alu_pair` variant (a receiving and a sending chip).  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#define HIPEMU_STATIC_SHARED 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_AR_WAVE_PRIMS 1
#define VGPU_MM_WAVE_PRIMS 1
#include <cstdint>
namespace vk {
inline unsigned long long ar_ballot(bool pred, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) { slot[0] = 0; slot[1] = 0; }
    __syncthreads();
    if (pred) slot[lane >> 5] |= 1u << (lane & 31u);
    __syncthreads();
    const unsigned long long r = (unsigned long long)slot[0] | ((unsigned long long)slot[1] << 32);
    __syncthreads();
    return r;
}
inline unsigned long long mm_ballot(bool pred, uint32_t* slot) { return ar_ballot(pred, slot); }
inline uint32_t mm_shfl_up(uint32_t v, uint32_t delta, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    slot[2 + lane] = v;
    __syncthreads();
    const uint32_t r = lane >= delta ? slot[2 + lane - delta] : v;
    __syncthreads();
    return r;
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/arithmetic_audit.hip"
#include "../../valida_amd/csrc/kernels/memory_audit.hip"
#include "../../valida_amd/csrc/host/arithmetic_audit.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using namespace vhost;
static_assert(sizeof(ArithmeticAuditOpts) == 20, "the options cross as the C struct");

namespace {
std::vector<uint32_t> working(const uint32_t* m, uint64_t h, uint64_t w) {  // column-major Montgomery: the prover's working layout
    std::vector<uint32_t> c(h * w);
    for (uint64_t r = 0; r < h; r++)
        for (uint64_t k = 0; k < w; k++) c[k * h + r] = vg::Fp::from_canonical(m[r * w + k]).v;
    return c;
}
AirDesc alu_chip(const char* name, bool send) {
    using V = vair::VirtualCol;
    vair::Interaction it;
    for (int k = 0; k < 13; k++) it.fields.push_back(V::single_main(k));
    it.count = V::single_main(13);
    it.bus_kind = vair::BusKind::Global; it.bus_index = 0; it.type = send ? vair::InteractionType::GlobalSend : vair::InteractionType::GlobalReceive;
    vair::Dag d;
    d.width = 14; d.prep_width = 0;
    return MachineDesc::make_air_from_dag(name, d, {it});
}
MachineDesc machine_of(uint32_t kind) {
    if (kind == 0) return MachineDesc::basic();
    MachineDesc m;
    m.airs.push_back(alu_chip("alu", false));
    if (kind == 2) m.airs.push_back(alu_chip("tx", true));
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces).  out: the report's word image.  Returns the words written, or -1.
int64_t emu_arithmetic_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                             const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, const ArithmeticAuditOpts* opts, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = machine_of(machine_kind);
        const ArithmeticAuditOpts o = arithmetic_audit_checked_opts(*opts);
        std::vector<BusShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        BusPlan bus_plan;
        const ArithmeticPlan plan = arithmetic_audit_plan(machine, ms, chips, ps, prep_slot, o, &bus_plan);
        const size_t NC = machine.airs.size(), NE = plan.entries.size();
        std::vector<std::vector<uint32_t>> cols;
        cols.reserve(2 * NC);
        std::vector<const uint32_t*> mp(NC, nullptr), pp(NC, nullptr);
        std::vector<uint64_t> mst(NC, 0), pst(NC, 0);
        for (size_t i = 0; i < NC; i++) { cols.push_back(working(main[i], heights[i], widths[i])); mp[i] = cols.back().data(); mst[i] = heights[i]; }
        for (size_t i = 0; i < NC; i++)
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; cols.push_back(working(prep[k], ph[k], pw[k])); pp[i] = cols.back().data(); pst[i] = ph[k]; }
        const std::vector<uint32_t> desc = bus_audit_descriptor(machine, bus_plan, mp, mst, pp, pst);
        ArithmeticReport rep;
        arithmetic_audit_header(rep, plan, o);
        const uint64_t n = plan.n_slots;
        std::vector<uint32_t> block_base(NE, 0);
        uint64_t nb = 0;
        for (size_t e = 0; e < NE; e++) { block_base[e] = (uint32_t)nb; nb += (plan.entries[e].height + 255) / 256; }
        std::vector<unsigned long long> tot((size_t)vk::AR_TOT * NE, 0);
        std::vector<uint32_t> verdict(n + 1, 0xdeadbeefu), tabs(2 * nb + 1, 0xdeadbeefu);
        uint32_t* hard_tab = tabs.data();
        uint32_t* soft_tab = tabs.data() + nb;
        for (size_t e = 0; e < NE; e++) {
            const ArithmeticPlan::Entry& pe = plan.entries[e];
            vk::launch_ar_judge(nullptr, desc.data(), pe.chip, pe.interaction, pe.height, (uint32_t)pe.first_slot, block_base[e], verdict.data(), tot.data() + e * vk::AR_TOT, hard_tab,
                                soft_tab);
        }
        if (verdict[n] != 0xdeadbeefu || tabs[2 * nb] != 0xdeadbeefu) throw std::runtime_error("the judge wrote past its verdicts or tables");
        for (uint64_t k = 0; k < n; k++)
            if (verdict[k] == 0xdeadbeefu) throw std::runtime_error("the judge left slot " + std::to_string(k) + " without a verdict");
        for (uint64_t k = 0; k < 2 * nb; k++)
            if (tabs[k] == 0xdeadbeefu) throw std::runtime_error("the judge left a table entry unwritten");
        uint64_t n_hard = 0, n_soft = 0;
        for (size_t e = 0; e < NE; e++) { const unsigned long long* t = tot.data() + e * vk::AR_TOT; n_hard += t[3] + t[4] + t[5]; n_soft += t[6] + t[7]; }
        const size_t listed_hard = (size_t)std::min<uint64_t>(n_hard, o.max_findings), listed_soft = (size_t)std::min<uint64_t>(n_soft, o.max_findings);
        const size_t n_out = (listed_hard + listed_soft) * vk::AR_OUT;
        std::vector<uint32_t> ow(n_out + 1, 0xdeadbeefu);
        if (n_out) {
            vk::launch_ar_scan(nullptr, hard_tab, soft_tab, nb);
            for (size_t e = 0; e < NE; e++) {
                const ArithmeticPlan::Entry& pe = plan.entries[e];
                const unsigned long long* t = tot.data() + e * vk::AR_TOT;
                if (!(t[3] + t[4] + t[5] + t[6] + t[7])) continue;
                vk::launch_ar_list(nullptr, desc.data(), pe.chip, pe.interaction, pe.is_send, pe.height, (uint32_t)pe.first_slot, block_base[e], verdict.data(), hard_tab, soft_tab,
                                   (uint32_t)listed_hard, (uint32_t)listed_soft, ow.data(), ow.data() + listed_hard * vk::AR_OUT);
            }
            for (size_t k = 0; k < n_out; k++)
                if (ow[k] == 0xdeadbeefu) throw std::runtime_error("the listing pass left word " + std::to_string(k) + " of its records unwritten");
        }
        if (ow[n_out] != 0xdeadbeefu) throw std::runtime_error("the listing pass wrote past its records");
        arithmetic_audit_from_device(rep, tot.data(), vk::AR_TOT, ow.data(), listed_hard, listed_soft);
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        std::copy(w.begin(), w.end(), out);
        return (int64_t)w.size();
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_arithmetic_audit: %s\n", e.what());
        return -1;
    }
}
}
