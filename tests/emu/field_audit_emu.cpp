// The field-audit kernels of valida_amd/csrc/kernels/field_audit.hip — the very source — compiled for the HOST under tools/hipemu and run on
// host traces: the counting pass, the scan over workgroups and the listing pass, for the compiled chip templates, the interpreted register
// program and the bus-only chips, driven as Prover::field_audit drives them and assembled into the report's word image
// (tests/test_field_audit_cpu.py compares it with the host audit).  The file's two wave-level helpers, fa_ballot and fa_wave_sync, get their
// emulation forms here: a wave is a 64-thread workgroup, a ballot goes through two LDS words between __syncthreads(), a wave sync is
// __syncthreads().  No other wave intrinsic is defined, and hipemu throws on __shfl and readlane, so the elimination's source could not run
// here if it used one.  The kernel runs one wave per workgroup on the device as well, so nothing it does between waves is left out here;
// what the emulation does not reach is the hardware itself: the real ballot, the wave barrier's fences, the LDS opt-in above 64 KB and the
// launch shapes fa_shape picks for tall traces.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
#define VGPU_FA_WAVE_PRIMS 1
namespace vk {
uint32_t fa_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
inline unsigned long long fa_ballot(bool pred, uint32_t* slot) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) { slot[0] = 0; slot[1] = 0; }
    __syncthreads();
    if (pred) slot[lane >> 5] |= 1u << (lane & 31u);
    __syncthreads();
    const unsigned long long r = (unsigned long long)slot[0] | ((unsigned long long)slot[1] << 32);
    __syncthreads();
    return r;
}
inline void fa_wave_sync() { __syncthreads(); }
}  // namespace vk

#include "../../valida_amd/csrc/kernels/field_audit.hip"
#include "../../valida_amd/csrc/host/field_audit.hpp"

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
// 1 the register programs; rows_per_workgroup = 0 keeps fa_shape's, another number forces that many (a small one makes halos, wraps and ranks
// cross more workgroups).  out: the report's word image.  Returns the words written, or -1.
int64_t emu_field_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                        const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_workgroup, uint32_t max_entries, uint32_t R, uint32_t chip_mask,
                        uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        RankAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask;
        o = field_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        field_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        FieldReport rep;
        rep.chips.resize(NC);
        std::vector<vk::FaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC), wr(NC), slot0(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::FaArgs& a = args[i];
            a = vk::FaArgs{};
            wr[i] = ra_weight_rows(air);
            FieldChipStat& cs = rep.chips[i];
            field_audit_chip_block(cs, air, heights[i], rank_audit_selected(o, i), wr[i]);
            if (!cs.audited || !air.width) continue;
            a.K = air.program.num_asserts;
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols[i].data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            a.wr = wr[i].data();
            a.M = (uint32_t)air.interactions.size();
            for (auto& it : cs.interactions) { slot0[i].push_back(a.NS); a.NS += it.n_fields; a.F = std::max(a.F, it.n_fields); }
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : air.native_chip);
            vk::fa_shape(a);
            if (rows_per_workgroup) a.T = rows_per_workgroup;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            totals[i].assign(vk::fa_totals_words(a) / 2, 0);
            table[i].assign((size_t)a.NS * a.NB + 1, 0);
            prefix[i].assign((size_t)a.NS * a.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_fa_count(nullptr, a, totals[i].data(), table[i].data());
            cs.live_records = totals[i][0]; cs.floating_fields = totals[i][1]; cs.floating_rows = totals[i][2];
            for (size_t m = 0; m < cs.interactions.size(); m++) {
                cs.interactions[m].live_rows = totals[i][3 + m];
                for (uint32_t j = 0; j < cs.interactions[m].n_fields; j++) cs.interactions[m].floating[j] = totals[i][3 + a.M + slot0[i][m] + j];
            }
        }
        field_audit_finish(rep, o);
        auto slot_of = [&](const FieldEntry& e) { return slot0[e.chip][e.interaction] + e.field; };
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            const vk::FaArgs& a = args[chip];
            const uint32_t s_cut = slot_of(rep.entries[e1 - 1]) + 1;
            std::vector<uint32_t> rows((size_t)s_cut * R * RA_ROW_WORDS, 0);
            vk::launch_fa_scan(nullptr, a, table[chip].data(), prefix[chip].data(), s_cut);
            vk::launch_fa_list(nullptr, a, table[chip].data(), prefix[chip].data(), s_cut, R, rows.data());
            for (size_t e = e0; e < e1; e++) {
                FieldEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.floating, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = rows.data() + ((size_t)slot_of(en) * R + k) * RA_ROW_WORDS;
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
        fprintf(stderr, "field_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
