// The constraint-audit kernels of valida_amd/csrc/kernels/constraint_audit.hip — the very source — compiled for the HOST under tools/hipemu and
// run on host traces: the counting pass, the scan over workgroups, the listing pass and the value pass, for the compiled chip templates and for
// the interpreted register program, driven as Prover::constraint_audit drives them and assembled into the report's word image
// (tests/test_constraint_audit_cpu.py compares it with the reference).  The file's one wave-level helper, ca_wave_add, is replaced by its
// contract for a wave of ONE lane (the emulator's fibers cannot model a wave); no other wave intrinsic is defined here, so the source would not
// even compile if it used one.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
#define VGPU_CA_WAVE_ADD 1
namespace vk {
uint32_t ca_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
inline uint32_t ca_wave_add(uint32_t* counter, bool pred) {
    if (pred) atomicAdd(counter, 1u);
    return pred ? 1u : 0u;
}
}  // namespace vk

#include "../../valida_amd/csrc/kernels/constraint_audit.hip"
#include "../../valida_amd/csrc/host/constraint_audit.hpp"

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
// 1 the register programs; block_threads = 0 keeps the launch shape of the device (256 rows per workgroup), another power of two <= 256 makes
// workgroups smaller so that ranks cross more of them.  out: the report's word image.  Returns the words written, or -1.
int64_t emu_constraint_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                             const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t block_threads, uint32_t max_constraints, uint32_t R, uint32_t* out,
                             uint64_t cap) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        ConstraintAuditOpts o;
        o.max_constraints = max_constraints; o.max_rows_per_constraint = R;
        o = constraint_audit_checked_opts(o);
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        constraint_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        ConstraintReport rep;
        rep.chips.resize(NC);
        std::vector<std::vector<uint64_t>> counts(NC);
        std::vector<vk::CaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::CaArgs& a = args[i];
            a = vk::CaArgs{};
            a.K = air.program.num_asserts;
            rep.chips[i].n_constraints = a.K; rep.chips[i].height = heights[i];
            counts[i].assign(a.K, 0);
            if (!a.K) continue;
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols[i].data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.native_chip = interpret ? vk::CA_INTERPRET : air.native_chip;
            a.T = block_threads ? block_threads : vk::ca_block_threads(a);
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            totals[i].assign(a.K + 1, 0);
            table[i].assign((size_t)a.K * a.NB, 0);
            prefix[i].assign((size_t)a.K * a.NB, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_ca_count(nullptr, a, totals[i].data(), table[i].data());
            for (uint32_t k = 0; k < a.K; k++) counts[i][k] = totals[i][k];
            rep.chips[i].failing_rows = totals[i][a.K];
        }
        constraint_audit_finish(rep, counts, o);
        for (size_t e0 = 0; e0 < rep.constraints.size();) {
            const uint32_t chip = rep.constraints[e0].chip;
            size_t e1 = e0;
            vk::CaListed listed{};
            while (e1 < rep.constraints.size() && rep.constraints[e1].chip == chip) { const uint32_t k = rep.constraints[e1].constraint; listed.w[k >> 5] |= 1u << (k & 31u); e1++; }
            const vk::CaArgs& a = args[chip];
            std::vector<uint32_t> rows((size_t)a.K * o.max_rows_per_constraint, 0xffffffffu), values((size_t)a.K * o.max_rows_per_constraint, 0xffffffffu);
            vk::launch_ca_scan(nullptr, a, table[chip].data(), prefix[chip].data(), listed);
            vk::launch_ca_list(nullptr, a, table[chip].data(), prefix[chip].data(), listed, o.max_rows_per_constraint, rows.data());
            vk::launch_ca_values(nullptr, a, totals[chip].data(), listed, o.max_rows_per_constraint, rows.data(), values.data());
            for (size_t e = e0; e < e1; e++) {
                ConstraintEntry& en = rep.constraints[e];
                const uint64_t n_listed = std::min<uint64_t>(en.failing_rows, o.max_rows_per_constraint);
                for (uint64_t j = 0; j < n_listed; j++) en.rows.push_back({rows[(size_t)en.constraint * o.max_rows_per_constraint + j], values[(size_t)en.constraint * o.max_rows_per_constraint + j]});
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "constraint_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
