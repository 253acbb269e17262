// The program-audit kernels of valida_amd/csrc/kernels/program_audit.hip — the very source, with the memory audit's one-workgroup scan they
// launch — compiled for the HOST under tools/hipemu and run on host traces, driven as Prover::program_audit drives them and assembled by the
// same host code into the report's word image (tests/test_program_audit_cpu.py compares it with the host audit): the histogram with its LDS
// bins, slices and the uniform-wave shortcut, the judge's counting pass with its halo tile and LDS table copy, the table pass with its two
// halos, the scans of the six workgroup tables and the two listing passes.  A workgroup has its 256 threads and four waves here; the wave
// primitives get emulation forms: a ballot and a shuffle go through the wave's LDS words between __syncthreads() (every call site is
// workgroup-uniform).  The program audit's kernels use dynamic LDS only (one global array here), the memory audit's static arrays: __shared__
// is redefined between the two includes.  The machine is two captured chips of the given widths (fetch_chip 0, table_chip 1).  Test
// infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_PG_WAVE_PRIMS 1
#define VGPU_MM_WAVE_PRIMS 1
#include <cstdint>
namespace vk {
alignas(8) uint32_t pg_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
inline unsigned long long pg_ballot(bool pred, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) { slot[0] = 0; slot[1] = 0; }
    __syncthreads();
    if (pred) slot[lane >> 5] |= 1u << (lane & 31u);
    __syncthreads();
    const unsigned long long r = (unsigned long long)slot[0] | ((unsigned long long)slot[1] << 32);
    __syncthreads();
    return r;
}
inline uint32_t pg_shfl(uint32_t v, uint32_t src, uint32_t* slot) {
    slot[2 + (threadIdx.x & 63u)] = v;
    __syncthreads();
    const uint32_t r = slot[2 + src];
    __syncthreads();
    return r;
}
inline unsigned long long mm_ballot(bool pred, uint32_t* slot) { return pg_ballot(pred, slot); }
inline uint32_t mm_shfl_up(uint32_t v, uint32_t delta, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    slot[2 + lane] = v;
    __syncthreads();
    const uint32_t r = lane >= delta ? slot[2 + lane - delta] : v;
    __syncthreads();
    return r;
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/program_audit.hip"
#undef __shared__
#define __shared__ static
#include "../../valida_amd/csrc/kernels/memory_audit.hip"
#include "../../valida_amd/csrc/host/program_audit.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using namespace vhost;
static_assert(sizeof(ProgramAuditOpts) == 104, "the options cross as the C struct");

namespace {
std::vector<uint32_t> working(const uint32_t* m, uint64_t h, uint64_t w) {  // column-major Montgomery: the prover's working layout
    std::vector<uint32_t> c(h * w);
    for (uint64_t r = 0; r < h; r++)
        for (uint64_t k = 0; k < w; k++) c[k * h + r] = vg::Fp::from_canonical(m[r * w + k]).v;
    return c;
}
AirDesc chip(const char* name, uint64_t width, uint64_t prep_width) {
    vair::Dag d;
    d.width = (int)width; d.prep_width = (int)prep_width;
    return MachineDesc::make_air_from_dag(name, d, {});
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces: the fetching chip's main trace, the table chip's main and
// preprocessed traces).  out: the report's word image.  Returns the words written, or -1.
int64_t emu_program_audit(const uint32_t* fetch, uint64_t fh, uint64_t fw, const uint32_t* tmain, uint64_t th, uint64_t tw, const uint32_t* tprep, uint64_t ph, uint64_t pw,
                          const ProgramAuditOpts* opts, uint32_t* out, uint64_t cap) {
    try {
        const ProgramAuditOpts o = *opts;
        MachineDesc machine;
        machine.airs.push_back(chip("fetcher", fw, 0));
        machine.airs.push_back(chip("table", tw, pw));
        const ProgramPlan plan = program_audit_plan(machine, {{fh, fw}, {th, tw}}, {1}, {{ph, pw}}, o);
        ProgramReport rep;
        program_audit_header(rep, plan, o);
        const uint64_t H = plan.fetches, T = plan.table_rows, nbj = (H + 255) / 256, nbt = (T + 255) / 256;
        const std::vector<uint32_t> fcols = working(fetch, fh, fw), tcols = working(tmain, th, tw), pcols = working(tprep, ph, pw);
        vk::PgArgs a{};
        a.fmain = fcols.data(); a.fstride = fh; a.H = H; a.tmain = tcols.data(); a.tmstride = th; a.tprep = pcols.data(); a.tpstride = ph;
        a.T = (uint32_t)T; a.rom_len = plan.rom_len; a.n_fields = o.n_fields; a.pc_col = o.pc_col; a.key_col = o.key_col; a.mult_col = o.mult_col;
        a.lds_table = vk::program_audit_lds_table(o.n_fields, T) ? 1u : 0u;
        for (int j = 0; j < 8; j++) { a.field_cols[j] = o.field_cols[j]; a.table_cols[j] = o.table_cols[j]; }
        std::vector<unsigned long long> tot(vk::PG_TOT, 0);
        std::vector<uint32_t> counts(T + 1, 0), tabs(2 * nbj + 4 * nbt + 1, 0xdeadbeefu);
        counts[T] = 0xdeadbeefu;
        uint32_t* hard_tab = tabs.data();
        uint32_t* wrap_tab = tabs.data() + nbj;
        uint32_t* ttabs = tabs.data() + 2 * nbj;
        vk::launch_pg_hist(nullptr, a.fmain + (uint64_t)a.pc_col * a.fstride, H, a.T, counts.data());
        vk::launch_pg_judge(nullptr, a, vk::PG_COUNT, tot.data(), hard_tab, wrap_tab, 0, 0, 0, nullptr, nullptr);
        vk::launch_pg_table(nullptr, a, vk::PG_COUNT, counts.data(), tot.data(), ttabs, 0, 0, 0, nullptr, nullptr);
        if (counts[T] != 0xdeadbeefu || tabs.back() != 0xdeadbeefu) throw std::runtime_error("a counting pass wrote past its table");
        const uint64_t n_key = tot[8], n_fetch = tot[3] + tot[4], n_mult = tot[9];
        const size_t listed_hard = (size_t)std::min<uint64_t>(n_key + n_fetch + n_mult, o.max_findings), listed_wrapped = (size_t)std::min<uint64_t>(tot[5], o.max_findings),
                     listed_ranges = (size_t)std::min<uint64_t>(tot[11], o.max_ranges);
        const size_t n_out = (listed_hard + listed_wrapped) * vk::PG_OUT + 2 * listed_ranges;
        std::vector<uint32_t> ow(n_out + 1, 0xdeadbeefu);
        if (n_out) {
            uint32_t* out_wrap = ow.data() + listed_hard * vk::PG_OUT;
            uint32_t* ranges = out_wrap + listed_wrapped * vk::PG_OUT;
            const uint32_t hard_base = (uint32_t)std::min<uint64_t>(n_key, listed_hard), mult_base = (uint32_t)std::min<uint64_t>(n_key + n_fetch, listed_hard);
            if (listed_wrapped || hard_base < listed_hard)
                vk::launch_pg_judge(nullptr, a, vk::PG_LIST, tot.data(), hard_tab, wrap_tab, hard_base, (uint32_t)listed_hard, (uint32_t)listed_wrapped, ow.data(), out_wrap);
            if (listed_ranges || (listed_hard && (n_key || mult_base < listed_hard)))
                vk::launch_pg_table(nullptr, a, vk::PG_LIST, counts.data(), tot.data(), ttabs, mult_base, (uint32_t)listed_hard, (uint32_t)listed_ranges, ow.data(), ranges);
            for (size_t k = 0; k < n_out; k++)
                if (ow[k] == 0xdeadbeefu) throw std::runtime_error("a listing pass left word " + std::to_string(k) + " of its records unwritten");
        }
        if (ow[n_out] != 0xdeadbeefu) throw std::runtime_error("a listing pass wrote past its records");
        program_audit_from_device(rep, tot.data(), ow.data(), listed_hard, listed_wrapped, ow.data() + (listed_hard + listed_wrapped) * vk::PG_OUT, listed_ranges);
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        std::copy(w.begin(), w.end(), out);
        return (int64_t)w.size();
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_program_audit: %s\n", e.what());
        return -1;
    }
}
}
