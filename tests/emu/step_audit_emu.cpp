// The step-audit kernels of valida_amd/csrc/kernels/step_audit.hip — the very source, with rank_elim.hpp and the rank audit's scan kernel —
// compiled for the HOST under tools/hipemu and run on host traces: the counting pass, the scan over workgroups and the listing pass, for the
// compiled chip templates, the interpreted register program and the bus-only chips, driven as Prover::step_audit drives them and assembled
// into the report's word image (tests/test_step_audit_cpu.py compares it with the host audit).  The wave primitives get the emulation forms
// of tests/emu/rank_audit_emu.cpp: a wave is a 64-thread workgroup, a ballot goes through two LDS words between __syncthreads(), a wave sync
// is __syncthreads().  A workgroup is ONE wave here (NW = 1): what the waves of a workgroup exchange in the listing pass runs with a single
// wave only; more than one wave per workgroup is covered by the GPU tests alone.  machine = 0: the BasicMachine; 1: the six analytic AIRs of
// tests/test_rank_audit_cpu.py (sum3, prod, step, bus, square, wide), built here from the same expressions.  Test infrastructure; nothing in
// the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
namespace vk {
uint32_t ra_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
uint32_t sa_lds[40 * 1024];
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
#include "../../valida_amd/csrc/kernels/step_audit.hip"
#include "../../valida_amd/csrc/host/step_audit.hpp"

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

MachineDesc analytic() {
    MachineDesc m;
    auto air = [&](const char* name, int width, auto build, std::vector<vair::Interaction> inter) {
        vair::Dag d;
        d.width = width; d.prep_width = 0;
        build(d);
        m.airs.push_back(MachineDesc::make_air_from_dag(name, d, std::move(inter)));
    };
    air("sum3", 3, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.add(d.var(false, 0, false), d.var(false, 1, false)), d.var(false, 2, false))); }, {});
    air("prod", 3, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.mul(d.var(false, 0, false), d.var(false, 1, false)), d.var(false, 2, false))); }, {});
    air("step", 1, [](vair::Dag& d) {
        const uint32_t step = d.sub(d.sub(d.var(false, 0, true), d.var(false, 0, false)), d.constant(1));
        d.constraints.push_back(d.mul(d.selector(vair::N_TRANS), step));
    }, {});
    vair::Interaction it;
    it.fields.push_back(vair::VirtualCol::new_main({{0, 1}, {1, 1}}, 0));
    it.fields.push_back(vair::VirtualCol::single_main(2));
    it.count = vair::VirtualCol::single_main(3);
    it.bus_kind = vair::BusKind::Local; it.bus_index = 0; it.type = vair::InteractionType::LocalSend;
    air("bus", 4, [](vair::Dag&) {}, {it});
    air("square", 1, [](vair::Dag& d) { d.constraints.push_back(d.mul(d.var(false, 0, false), d.var(false, 0, false))); }, {});
    air("wide", 70, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.add(d.var(false, 0, false), d.var(false, 35, false)), d.var(false, 69, false))); }, {});
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces): interpret = 0 runs the compiled chip templates (machine 0 only),
// 1 the register programs; rows_per_wave = 0 keeps sa_shape's rows per wave, another number forces that many (also the rows per workgroup).
// steps: n_steps canonical values, 0: the default.  out: the report's word image.  Returns the words written, or -1.
int64_t emu_step_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                       const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_wave, uint32_t max_entries, uint32_t R,
                       uint32_t chip_mask, const uint32_t* steps, uint32_t n_steps, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = machine_kind ? analytic() : MachineDesc::basic();
        StepAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask; o.n_steps = n_steps;
        for (uint32_t i = 0; i < n_steps && i < SA_MAX_STEPS; i++) o.steps[i] = steps[i];
        o = step_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        step_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        StepReport rep;
        rep.chips.resize(NC);
        std::vector<vk::SaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC), wr(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            args[i] = vk::SaArgs{};
            vk::RaArgs& a = args[i].r;
            args[i].n_steps = o.n_steps;
            for (uint32_t s = 0; s < SA_MAX_STEPS; s++) args[i].steps[s] = vg::Fp::from_canonical(o.steps[s]).v;
            StepChipStat& cs = rep.chips[i];
            step_audit_chip_block(cs, air, heights[i], step_audit_selected(o, i), o.n_steps);
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
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : ((interpret || machine_kind) ? vk::CA_INTERPRET : air.native_chip);
            vk::sa_shape(args[i]);
            a.NW = 1;  // a wave is a workgroup here
            if (rows_per_wave) a.RPW = rows_per_wave;
            a.T = a.RPW;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            totals[i].assign(vk::sa_totals_words(args[i]) / 2, 0);
            table[i].assign((size_t)a.width * a.NB + 1, 0);
            prefix[i].assign((size_t)a.width * a.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_sa_count(nullptr, args[i], totals[i].data(), table[i].data());
            cs.confirmed_rows = totals[i][0]; cs.refuted_rows = totals[i][1];
            for (uint32_t s = 0; s < SA_MAX_STEPS; s++) cs.passes[s] = totals[i][2 + s];
            for (uint32_t k = 0; k < cs.width; k++) {
                cs.loose[k] = totals[i][6 + 4 * k]; cs.zeros[k] = totals[i][7 + 4 * k]; cs.exact[k] = totals[i][8 + 4 * k]; cs.coupled_exact[k] = totals[i][9 + 4 * k];
            }
        }
        step_audit_finish(rep, o);
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            const vk::SaArgs& sa = args[chip];
            const uint32_t c_cut = rep.entries[e1 - 1].column + 1;
            std::vector<uint32_t> rows((size_t)c_cut * R * SA_ROW_WORDS, 0);
            vk::launch_ra_scan(nullptr, sa.r, table[chip].data(), prefix[chip].data(), c_cut);
            vk::launch_sa_list(nullptr, sa, table[chip].data(), prefix[chip].data(), c_cut, R, rows.data());
            for (size_t e = e0; e < e1; e++) {
                StepEntry& en = rep.entries[e];
                const uint64_t listed = std::min<uint64_t>(en.coupled_exact + en.curved, R);
                en.rows.resize((size_t)listed);
                for (size_t k = 0; k < listed; k++) {
                    const uint32_t* src = rows.data() + ((size_t)en.column * R + k) * SA_ROW_WORDS;
                    en.rows[k].row = src[0]; en.rows[k].pass_mask = src[1]; en.rows[k].zero = src[2]; en.rows[k].n_support = src[3];
                    for (uint32_t x = 0; x < 2 * RA_TERMS; x++) en.rows[k].terms[x] = src[4 + x];
                }
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "step_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
