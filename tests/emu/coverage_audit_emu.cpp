// The coverage-audit kernels of valida_amd/csrc/kernels/coverage_audit.hip — the very source, with the evaluation code it shares with the mutation
// audit (mutation_eval.hpp) — compiled for the HOST under tools/hipemu and run on host traces: the audit pass, the merge and the pack, for the compiled chip
// templates, the interpreted register program and the bus-only chips, driven as Prover::coverage_audit drives them and assembled into the
// report's word image (tests/test_coverage_audit_cpu.py compares it with the reference).  The file's three wave-level helpers are replaced by
// their contracts for a wave of ONE lane (the emulator's fibers cannot model a wave); no other wave intrinsic is defined here, so the source
// would not even compile if it used one.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
template <class T> inline T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
inline int __popc(unsigned int x) { return __builtin_popcount(x); }  // per-thread bit operations, not wave intrinsics
inline int __ffs(int x) { return __builtin_ffs(x); }
#define VGPU_MA_WAVE_ADD 1
#define VGPU_COV_WAVE_HELPERS 1
namespace vk {
uint32_t ma_lds[40 * 1024];   // mutation_audit.hip is included for ma_column_slices; its kernels are not run here
uint32_t cov_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
inline void ma_wave_add(uint32_t* counter, bool pred) {
    if (pred) atomicAdd(counter, 1u);
}
inline uint32_t cov_wave_or(uint32_t w) { return w; }
inline void cov_wave_tally(uint32_t* cell, bool pred, bool solo, uint32_t row) {
    if (pred) { atomicAdd(&cell[0], 1u | (solo ? 1u << 16 : 0u)); atomicMin(&cell[1], row); }
    if (pred && solo) atomicMin(&cell[2], row);
}
inline void cov_wave_count(uint32_t* counter, bool pred) {
    if (pred) atomicAdd(counter, 1u);
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/mutation_audit.hip"
#include "../../valida_amd/csrc/kernels/coverage_audit.hip"
#include "../../valida_amd/csrc/host/coverage_audit.hpp"

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
// 1 the register programs; block_threads = 0 keeps the launch shape of the device, 64 or 128 makes the row tiles smaller; column_slices = 0
// keeps the device's choice (cov_shape), another number forces that many; max_workgroups as in the options; bus_walk = 1 evaluates every
// interaction per mutation instead of the bus masks.  out: the report's word image.  Returns the words written, or -1.
int64_t emu_coverage_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                           const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t block_threads, uint32_t column_slices, uint32_t max_workgroups,
                           uint32_t bus_walk, const uint32_t* deltas, uint32_t n_deltas, uint32_t max_cells, uint32_t* out, uint64_t cap_words) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        CoverageAuditOpts o;
        o.max_cells = max_cells; o.n_deltas = n_deltas; o.max_workgroups = max_workgroups;
        for (uint32_t i = 0; i < n_deltas && i < MA_MAX_DELTAS; i++) o.deltas[i] = deltas[i];
        o = coverage_audit_checked_opts(o);
        const uint32_t D = o.n_deltas;
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        coverage_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        CoverageReport rep;
        rep.deltas.assign(o.deltas, o.deltas + D);
        rep.chips.resize(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::CovArgs v{};
            vk::MaArgs& a = v.m;
            a.K = air.program.num_asserts;
            v.M = (uint32_t)air.interactions.size();
            CoverageChipStat& cs = rep.chips[i];
            cs.width = air.width; cs.n_constraints = a.K; cs.n_interactions = v.M; cs.height = heights[i];
            const size_t TDD = (size_t)(a.K + v.M) * D;
            cs.kills.assign(TDD, 0); cs.sole.assign(TDD, 0);
            const std::vector<uint32_t> mcols = working(main[i], heights[i], widths[i]);
            std::vector<uint32_t> pcols;
            a.main = mcols.data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols = working(prep[k], ph[k], pw[k]); a.prep = pcols.data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            std::vector<uint32_t> flags = ma_column_flags(air);
            bool masks_ok = false;
            const std::vector<uint32_t> bm = ma_bus_masks(air, masks_ok);
            flags.insert(flags.end(), bm.begin(), bm.end());
            a.flags = flags.data();
            a.bus_walk = (bus_walk || !masks_ok) ? 1u : 0u;
            a.D = D;
            for (uint32_t k = 0; k < D; k++) a.delta[k] = vg::Fp::from_canonical(o.deltas[k]).v;
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : air.native_chip);
            vk::cov_shape(v, o.max_workgroups);
            if (block_threads) { a.T = block_threads; a.NB = (uint32_t)((a.n + a.T - 1) / a.T); }
            if (column_slices) a.CY = std::min<uint32_t>(column_slices, a.width);
            if (block_threads || column_slices) v.GX = o.max_workgroups ? std::min<uint32_t>(o.max_workgroups, a.NB) : a.NB;
            const uint64_t cells = vk::cov_cells(v), cap = std::min<uint64_t>(cells, o.max_cells);
            std::vector<unsigned long long> counts(2 * cells, 0xdeadbeefdeadbeefull), detected(4, 0);  // the merge must write what the pack reads
            std::vector<uint32_t> rows(2 * cells, 0xdeadbeefu), packed(vk::cov_packed_words(v, cap), 0xdeadbeefu);
            std::vector<uint32_t> wg_tables(4 * cells * v.GX, 0);
            vk::launch_cov_audit(nullptr, v, wg_tables.data(), detected.data());
            vk::launch_cov_merge(nullptr, v, wg_tables.data(), counts.data(), rows.data());
            vk::launch_cov_pack(nullptr, v, counts.data(), rows.data(), (uint32_t)cap, packed.data());
            for (uint32_t k = 0; k < D; k++) cs.detected[k] = detected[k];
            for (size_t k = 0; k < TDD; k++) { cs.kills[k] = ((uint64_t)packed[3 + 4 * k] << 32) | packed[2 + 4 * k]; cs.sole[k] = ((uint64_t)packed[5 + 4 * k] << 32) | packed[4 + 4 * k]; }
            const uint64_t nonzero = packed[0];
            rep.total_cells += nonzero;
            const uint64_t take = std::min<uint64_t>(std::min<uint64_t>(nonzero, cap), o.max_cells - rep.cells.size());
            for (uint64_t k = 0; k < take; k++) {
                const uint32_t* e = &packed[2 + 4 * TDD + 8 * k];
                CoverageCell cell;
                cell.chip = (uint32_t)i; cell.delta = e[0] % D; cell.column = (e[0] / D) % a.width; cell.detector = e[0] / D / a.width;
                cell.kills = ((uint64_t)e[2] << 32) | e[1]; cell.sole = ((uint64_t)e[4] << 32) | e[3]; cell.first_row = e[5]; cell.first_sole_row = e[6];
                rep.cells.push_back(cell);
            }
            coverage_classify(cs, D);
        }
        rep.truncated = rep.total_cells > rep.cells.size();
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap_words) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "coverage_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
