// The memory-audit kernels of valida_amd/csrc/kernels/memory_audit.hip — the very source — compiled for the HOST under tools/hipemu and run on
// host traces, driven as Prover::memory_audit drives them and assembled by the same host code into the report's word image
// (tests/test_memory_audit_cpu.py compares it with the host audit): the keys pass with its LDS tile and halo row, the gather, the max-scan over
// blocks, the judge's counting pass, the scan of the findings table and the listing pass.  The radix sort between them is the bus audit's
// (kernels/bus_audit.hip), whose scatter kernel ranks the lanes of a wave and is not emulated (tests/emu/bus_audit_emu.cpp): the (key, id)
// pairs are sorted here with std::stable_sort, after checking that the passes chosen by memory_audit_shifts sort as the full key does.  A
// workgroup has its 256 threads and four waves here; the wave primitives get emulation forms: a ballot and a shuffle go through the wave's LDS
// words between __syncthreads() (every call site is workgroup-uniform).  machine = 0: the BasicMachine; 1: the `ram` machine of
// tests/memory_audit_cases.py; 2: its two-receive variant.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#define HIPEMU_STATIC_SHARED 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include <numeric>

inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_MM_WAVE_PRIMS 1
#include <cstdint>
namespace vk {
inline unsigned long long mm_ballot(bool pred, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) { slot[0] = 0; slot[1] = 0; }
    __syncthreads();
    if (pred) slot[lane >> 5] |= 1u << (lane & 31u);
    __syncthreads();
    const unsigned long long r = (unsigned long long)slot[0] | ((unsigned long long)slot[1] << 32);
    __syncthreads();
    return r;
}
inline uint32_t mm_shfl_up(uint32_t v, uint32_t delta, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    slot[2 + lane] = v;
    __syncthreads();
    const uint32_t r = lane >= delta ? slot[2 + lane - delta] : v;
    __syncthreads();
    return r;
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/memory_audit.hip"
#include "../../valida_amd/csrc/host/memory_audit.hpp"

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
vair::Interaction receive(int base) {
    using V = vair::VirtualCol;
    vair::Interaction it;
    for (int k = 0; k < 8; k++) it.fields.push_back(V::single_main(base + k));
    it.count = V::new_main({{base, 1}, {base + 8, 1}}, 0);
    it.bus_kind = vair::BusKind::Global; it.bus_index = 2; it.type = vair::InteractionType::GlobalReceive;
    return it;
}
MachineDesc machine_of(uint32_t kind) {
    if (kind == 0) return MachineDesc::basic();
    MachineDesc m;
    vair::Dag d;
    d.width = kind == 1 ? 9 : 18; d.prep_width = 0;
    std::vector<vair::Interaction> its = {receive(0)};
    if (kind == 2) its.push_back(receive(9));
    m.airs.push_back(MachineDesc::make_air_from_dag(kind == 1 ? "ram" : "ram2", d, std::move(its)));
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces).  out: the report's word image.  Returns the words written, or -1.
int64_t emu_memory_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                         const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t max_findings, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = machine_of(machine_kind);
        MemoryAuditOpts o;
        o.max_findings = max_findings;
        o = memory_audit_checked_opts(o);
        std::vector<BusShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        BusPlan bus_plan;
        const MemoryPlan plan = memory_audit_plan(machine, ms, chips, ps, prep_slot, o, &bus_plan);
        const size_t NC = machine.airs.size();
        std::vector<std::vector<uint32_t>> cols;
        cols.reserve(2 * NC);
        std::vector<const uint32_t*> mp(NC, nullptr), pp(NC, nullptr);
        std::vector<uint64_t> mst(NC, 0), pst(NC, 0);
        for (size_t i = 0; i < NC; i++) { cols.push_back(working(main[i], heights[i], widths[i])); mp[i] = cols.back().data(); mst[i] = heights[i]; }
        for (size_t i = 0; i < NC; i++)
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; cols.push_back(working(prep[k], ph[k], pw[k])); pp[i] = cols.back().data(); pst[i] = ph[k]; }
        const std::vector<uint32_t> desc = bus_audit_descriptor(machine, bus_plan, mp, mst, pp, pst);
        std::vector<uint32_t> entries;
        const std::vector<uint32_t> mt = memory_audit_mt(plan, entries);
        MemoryReport rep;
        memory_audit_header(rep, plan, o);
        const uint64_t n = plan.n_slots;
        std::vector<unsigned long long> keys(n + 1, 0x5555555555555555ull), tot(vk::MM_KEY_TOT + vk::MM_JUDGE_TOT, 0);
        std::vector<uint32_t> ids(n + 1, 0xdeadbeefu);
        for (size_t e = 0; e < entries.size(); e++)
            vk::launch_mm_keys(nullptr, desc.data(), mt.data(), (uint32_t)e, plan.chips[entries[e]].height, (uint32_t)plan.chips[entries[e]].receives.size(), keys.data(), ids.data(),
                               tot.data());
        const uint64_t n_live = tot[0];
        if (!n_live) {
            memory_audit_from_device(rep, plan, tot.data(), nullptr, nullptr, 0);
        } else {
            // the sort: by the digits memory_audit_shifts chose (what launch_ba_sort is given), checked against the order by the full key
            int shifts[8];
            const int n_shifts = memory_audit_shifts(tot[1], tot[2], n_live < n, shifts);
            std::vector<uint32_t> ord(n), full(n);
            std::iota(ord.begin(), ord.end(), 0u);
            for (int p = 0; p < n_shifts; p++)
                std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return ((keys[a] >> shifts[p]) & 255u) < ((keys[b] >> shifts[p]) & 255u); });
            std::iota(full.begin(), full.end(), 0u);
            std::stable_sort(full.begin(), full.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
            for (uint64_t i = 0; i < n_live; i++)
                if (ord[i] != full[i]) throw std::runtime_error("the chosen radix passes do not sort the live keys");
            std::vector<unsigned long long> skeys(n);
            std::vector<uint32_t> sids(n);
            for (uint64_t i = 0; i < n; i++) { skeys[i] = keys[ord[i]]; sids[i] = ids[ord[i]]; }
            const uint64_t nb = (n_live + 255) / 256;
            std::vector<uint32_t> rec(vk::MM_REC * n_live, 0xdeadbeefu), mark(n_live, 0xdeadbeefu), block_before(vk::memory_audit_scan_blocks(n_live), 0xdeadbeefu), table(nb, 0xdeadbeefu);
            vk::launch_mm_gather(nullptr, desc.data(), mt.data(), skeys.data(), sids.data(), n_live, n_live, rec.data(), mark.data());
            vk::launch_mm_scan(nullptr, mark.data(), n_live, block_before.data());
            unsigned long long* cnt = tot.data() + vk::MM_KEY_TOT;
            vk::launch_mm_judge(nullptr, vk::MM_COUNT, rec.data(), sids.data(), mark.data(), block_before.data(), n_live, n_live, cnt, table.data(), 0, nullptr);
            const uint64_t total = cnt[6] + cnt[7] + cnt[8] + cnt[9];
            const size_t listed = (size_t)std::min<uint64_t>(total, o.max_findings);
            std::vector<uint32_t> ow(listed * vk::MM_OUT + 1, 0xdeadbeefu);
            if (listed) vk::launch_mm_judge(nullptr, vk::MM_LIST, rec.data(), sids.data(), mark.data(), block_before.data(), n_live, n_live, nullptr, table.data(), (uint32_t)listed, ow.data());
            memory_audit_from_device(rep, plan, tot.data(), cnt, ow.data(), listed);
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        std::copy(w.begin(), w.end(), out);
        return (int64_t)w.size();
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_memory_audit: %s\n", e.what());
        return -1;
    }
}
}
