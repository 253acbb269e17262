// The pair-audit kernels of valida_amd/csrc/kernels/pair_audit.hip — the very source — compiled for the HOST under tools/hipemu and run on host
// traces: the counting pass, the scan over workgroups and the listing pass, for the compiled chip templates, the interpreted register program
// and the bus-only chips, driven as Prover::pair_audit drives them and assembled into the report's word image
// (tests/test_pair_audit_cpu.py compares it with the reference).  The file's one wave-level helper, pa_wave_add, is replaced by its contract for
// a wave of ONE lane (the emulator's fibers cannot model a wave); no other wave intrinsic is defined here, so the source would not even compile
// if it used one.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_PA_WAVE_ADD 1
namespace vk {
uint32_t pa_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
inline void pa_wave_add(uint32_t* counter, bool pred) {
    if (pred) atomicAdd(counter, 1u);
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/pair_audit.hip"
#include "../../valida_amd/csrc/host/pair_audit.hpp"

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
// 1 the register programs; block_threads = 0 keeps the launch shape of the device, 64 or 128 makes workgroups smaller so that halos and ranks
// cross more of them; pairs_per_slice = 0 keeps the device's choice (pa_shape), another number forces that many pairs per slice (a large one:
// one slice); bus_walk = 1 evaluates every interaction per mutation instead of the bus masks.  out: the report's word image.  Returns the
// words written, or -1.
int64_t emu_pair_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                       const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t block_threads, uint32_t pairs_per_slice, uint32_t bus_walk, const uint32_t* deltas,
                       uint32_t n_deltas, uint32_t max_entries, uint32_t R, uint32_t chip_mask, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        PairAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.n_deltas = n_deltas; o.chip_mask = chip_mask;
        for (uint32_t i = 0; i < n_deltas && i < MA_MAX_DELTAS; i++) o.deltas[i] = deltas[i];
        o = pair_audit_checked_opts(o, machine.airs.size());
        const uint32_t D = o.n_deltas, DD = D * D;
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        pair_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        PairReport rep;
        rep.chips.resize(NC);
        std::vector<std::vector<uint64_t>> counts(NC), ufree(NC);
        std::vector<vk::PaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC), flags(NC), pairs(NC), pmasks(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::PaArgs& v = args[i];
            v = vk::PaArgs{};
            vk::MaArgs& a = v.m;
            a.K = air.program.num_asserts;
            PairChipStat& cs = rep.chips[i];
            cs.width = air.width; cs.n_constraints = a.K; cs.n_interactions = (uint32_t)air.interactions.size(); cs.height = heights[i];
            cs.audited = pair_audit_selected(o, i) ? 1u : 0u;
            ufree[i].assign(DD, 0);
            if (!cs.audited) continue;
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols[i].data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            flags[i] = ma_column_flags(air);
            bool masks_ok = false;
            const std::vector<uint32_t> bm = ma_bus_masks(air, masks_ok);
            flags[i].insert(flags[i].end(), bm.begin(), bm.end());
            a.flags = flags[i].data();
            a.D = D;
            for (uint32_t k = 0; k < D; k++) a.delta[k] = vg::Fp::from_canonical(o.deltas[k]).v;
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : air.native_chip);
            pairs[i] = pa_coupled_pairs(air, a.n);
            pmasks[i] = pa_bus_masks(air, pairs[i], o.deltas, D, masks_ok);
            a.bus_walk = (bus_walk || !masks_ok) ? 1u : 0u;
            pairs[i].push_back(0);  // (never read: the list is not empty for the pointer's sake)
            v.pairs = pairs[i].data(); v.pmasks = pmasks[i].data();
            v.P = (uint32_t)pairs[i].size() - 1;
            vk::pa_shape(v);
            if (block_threads) { a.T = block_threads; a.NB = (uint32_t)((a.n + a.T - 1) / a.T); }
            if (pairs_per_slice) {
                v.PPS = std::min<uint32_t>(pairs_per_slice, vk::PA_SLICE_ENTRIES / DD);
                a.CY = v.P ? (v.P + v.PPS - 1) / v.PPS : 1;
            }
            const size_t E = (size_t)v.P * DD;
            totals[i].assign(vk::pa_totals_words(v) / 2, 0);
            table[i].assign(E * a.NB + 1, 0);
            prefix[i].assign(E * a.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_pa_count(nullptr, v, totals[i].data(), table[i].data());
            counts[i].assign(totals[i].begin(), totals[i].begin() + 2 * E);
            for (uint32_t q = 0; q < DD; q++) ufree[i][q] = totals[i][2 * E + q] - totals[i][2 * E + 16 + q];
            pairs[i].pop_back();
        }
        pair_audit_finish(rep, pairs, counts, ufree, o);
        auto entry_index = [&](const PairEntry& en) {
            const auto& pl = pairs[en.chip];
            for (size_t k = 0; k < pl.size(); k++)
                if (pl[k] == (en.c1 | (en.c2 << 16))) return (uint64_t)k * DD + en.q;
            throw std::logic_error("an entry of a pair that is not coupled");
        };
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            const vk::PaArgs& v = args[chip];
            const uint32_t e_cut = (uint32_t)entry_index(rep.entries[e1 - 1]) + 1;
            std::vector<uint32_t> rows((size_t)e_cut * R, 0xffffffffu);
            vk::launch_pa_scan(nullptr, v, totals[chip].data(), table[chip].data(), prefix[chip].data(), e_cut);
            vk::launch_pa_list(nullptr, v, table[chip].data(), prefix[chip].data(), e_cut, R, rows.data());
            for (size_t e = e0; e < e1; e++) {
                PairEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.compensated, R);
                const size_t at = (size_t)entry_index(en) * R;
                en.rows.assign(rows.begin() + at, rows.begin() + at + listed);
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "pair_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
