// The rank-audit kernels of valida_amd/csrc/kernels/rank_audit.hip — the very source — compiled for the HOST under tools/hipemu and run on host
// traces: the counting pass, the scan over workgroups and the listing pass, for the compiled chip templates, the interpreted register program
// and the bus-only chips, driven as Prover::rank_audit drives them and assembled into the report's word image
// (tests/test_rank_audit_cpu.py compares it with the host audit and the reference).  The file's two wave-level helpers, ra_ballot and
// ra_wave_sync, get their emulation forms here: a wave is a 64-thread workgroup, a ballot goes through two LDS words between
// __syncthreads(), a wave sync is __syncthreads().  No other wave intrinsic is defined, and hipemu throws on __shfl and readlane, so the
// elimination's source could not run here if it used one.  A workgroup is ONE wave here (NW = 1), so what the waves of a workgroup exchange in
// the listing pass (their coupled bits, the ranks of the waves before, the running counts) runs with a single wave only: more than one wave per
// workgroup is covered by the GPU tests alone.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
namespace vk {
uint32_t ra_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
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
}  // namespace vk

#include "../../valida_amd/csrc/kernels/rank_audit.hip"
#include "../../valida_amd/csrc/host/rank_audit.hpp"

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
}  // namespace

extern "C" {
// The whole device pass under emulation on the BasicMachine (canonical row-major host traces): interpret = 0 runs the compiled chip templates,
// 1 the register programs; rows_per_wave = 0 keeps ra_shape's rows per wave, another number forces that many (a workgroup is ONE wave here, so
// it is also the rows per workgroup: a small one makes halos, wraps and ranks cross more workgroups).  out: the report's word image.  Returns
// the words written, or -1.
int64_t emu_rank_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                       const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_wave, uint32_t max_entries, uint32_t R, uint32_t chip_mask,
                       uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        RankAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask;
        o = rank_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        rank_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        RankReport rep;
        rep.chips.resize(NC);
        std::vector<vk::RaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC), wr(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::RaArgs& a = args[i];
            a = vk::RaArgs{};
            RankChipStat& cs = rep.chips[i];
            cs.width = air.width; cs.n_constraints = air.program.num_asserts; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = heights[i];
            cs.audited = rank_audit_selected(o, i) ? 1u : 0u;
            cs.loose.assign(air.width, 0); cs.zeros.assign(air.width, 0);
            if (!cs.audited || !air.width) continue;
            a.K = air.program.num_asserts;
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols[i].data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            wr[i] = ra_weight_rows(air);
            a.wr = wr[i].data();
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : air.native_chip);
            vk::ra_shape(a);
            a.NW = 1;  // a wave is a workgroup here
            if (rows_per_wave) a.RPW = rows_per_wave;
            a.T = a.RPW;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            totals[i].assign(vk::ra_totals_words(a) / 2, 0);
            table[i].assign((size_t)a.width * a.NB + 1, 0);
            prefix[i].assign((size_t)a.width * a.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_ra_count(nullptr, a, totals[i].data(), table[i].data());
            cs.nullity = totals[i][0]; cs.zero = totals[i][1]; cs.coupled_rows = totals[i][2]; cs.max_nullity = (uint32_t)totals[i][3];
            for (uint32_t k = 0; k < cs.width; k++) { cs.loose[k] = totals[i][4 + 2 * k]; cs.zeros[k] = totals[i][5 + 2 * k]; }
        }
        rank_audit_finish(rep, o);
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            const vk::RaArgs& a = args[chip];
            const uint32_t c_cut = rep.entries[e1 - 1].column + 1;
            std::vector<uint32_t> rows((size_t)c_cut * R * RA_ROW_WORDS, 0);
            vk::launch_ra_scan(nullptr, a, table[chip].data(), prefix[chip].data(), c_cut);
            vk::launch_ra_list(nullptr, a, table[chip].data(), prefix[chip].data(), c_cut, R, rows.data());
            for (size_t e = e0; e < e1; e++) {
                RankEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.coupled, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = rows.data() + ((size_t)en.column * R + k) * RA_ROW_WORDS;
                    en.rows[k].row = src[0]; en.rows[k].n_support = src[1];
                    for (uint32_t x = 0; x < 2 * RA_TERMS; x++) en.rows[k].terms[x] = src[2 + x];
                }
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "rank_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
