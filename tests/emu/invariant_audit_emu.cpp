// The invariant-audit kernels of valida_amd/csrc/kernels/invariant_audit.hip — the very source, with rank_elim.hpp and the rank audit's scan
// kernel — compiled for the HOST under tools/hipemu and run on host traces: the streaming elimination per workgroup, the merge, the counting
// pass, the scan over workgroups and the listing pass, driven as Prover::invariant_audit drives them and assembled into the report's word
// image (tests/test_invariant_audit_cpu.py compares it with the host audit).  The wave primitives get the emulation forms of
// tests/emu/rank_audit_emu.cpp: a wave is a 64-thread workgroup, a ballot goes through two LDS words between __syncthreads(), a wave sync is
// __syncthreads().  A workgroup is ONE wave here (NW = 1): what the waves of a workgroup exchange in the listing pass runs with a single wave
// only; more than one wave per workgroup is covered by the GPU tests alone.  machine = 0: the BasicMachine; 1: the six analytic AIRs of
// tests/test_rank_audit_cpu.py; 2: one AIR of widths[0] columns without constraints or interactions ("free"); 3: one AIR of widths[0] columns
// with the one constraint c2 - 3 c0 - 7 ("affine").  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
namespace vk {
uint32_t ra_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
uint32_t ia_lds[40 * 1024];
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
#include "../../valida_amd/csrc/kernels/invariant_audit.hip"
#include "../../valida_amd/csrc/host/invariant_audit.hpp"

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

template <class Build>
void push_air(MachineDesc& m, const char* name, int width, Build build, std::vector<vair::Interaction> inter) {
    vair::Dag d;
    d.width = width; d.prep_width = 0;
    build(d);
    m.airs.push_back(MachineDesc::make_air_from_dag(name, d, std::move(inter)));
}

MachineDesc analytic() {
    MachineDesc m;
    push_air(m, "sum3", 3, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.add(d.var(false, 0, false), d.var(false, 1, false)), d.var(false, 2, false))); }, {});
    push_air(m, "prod", 3, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.mul(d.var(false, 0, false), d.var(false, 1, false)), d.var(false, 2, false))); }, {});
    push_air(m, "step", 1, [](vair::Dag& d) {
        const uint32_t step = d.sub(d.sub(d.var(false, 0, true), d.var(false, 0, false)), d.constant(1));
        d.constraints.push_back(d.mul(d.selector(vair::N_TRANS), step));
    }, {});
    vair::Interaction it;
    it.fields.push_back(vair::VirtualCol::new_main({{0, 1}, {1, 1}}, 0));
    it.fields.push_back(vair::VirtualCol::single_main(2));
    it.count = vair::VirtualCol::single_main(3);
    it.bus_kind = vair::BusKind::Local; it.bus_index = 0; it.type = vair::InteractionType::LocalSend;
    push_air(m, "bus", 4, [](vair::Dag&) {}, {it});
    push_air(m, "square", 1, [](vair::Dag& d) { d.constraints.push_back(d.mul(d.var(false, 0, false), d.var(false, 0, false))); }, {});
    push_air(m, "wide", 70, [](vair::Dag& d) { d.constraints.push_back(d.sub(d.add(d.var(false, 0, false), d.var(false, 35, false)), d.var(false, 69, false))); }, {});
    return m;
}
MachineDesc single(int width, bool affine) {
    MachineDesc m;
    if (affine)
        push_air(m, "affine", width, [](vair::Dag& d) {
            d.constraints.push_back(d.sub(d.sub(d.var(false, 2, false), d.mul(d.constant(3), d.var(false, 0, false))), d.constant(7)));
        }, {});
    else
        push_air(m, "free", width, [](vair::Dag&) {}, {});
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces): interpret = 0 runs the compiled chip templates (machine 0 only),
// 1 the register programs; rows_per_wave = 0 keeps ia_shape's rows per wave, another number forces that many (also the rows per workgroup);
// rows_per_basis = 0 keeps ia_basis_shape's slice of rows per phase-1 workgroup, another number forces that many.  out: the report's word
// image.  Returns the words written, or -1.
int64_t emu_invariant_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                            const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_wave, uint32_t rows_per_basis,
                            uint32_t max_entries, uint32_t R, uint32_t max_terms, uint32_t chip_mask, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = machine_kind == 0 ? MachineDesc::basic() : machine_kind == 1 ? analytic() : single((int)widths[0], machine_kind == 3);
        InvariantAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask; o.max_terms = max_terms;
        o = invariant_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        invariant_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        InvariantReport rep;
        rep.chips.resize(NC);
        std::vector<vk::IaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), table(NC), prefix(NC), wr(NC), inv(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        std::vector<size_t> e_at(NC + 1, 0);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            args[i] = vk::IaArgs{};
            vk::IaArgs& ia = args[i];
            vk::RaArgs& a = ia.r;
            InvariantChipStat& cs = rep.chips[i];
            invariant_audit_chip_block(cs, air, heights[i], invariant_audit_selected(o, i));
            e_at[i] = rep.entries.size();
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
            // phase 1
            vk::ia_basis_shape(ia);
            if (rows_per_basis) { ia.RB = rows_per_basis; ia.NB1 = (uint32_t)((a.n + ia.RB - 1) / ia.RB); }
            std::vector<uint32_t> part((size_t)vk::ia_part_words(ia), 0xdeadbeefu);  // the merge reads only what a workgroup wrote
            inv[i].assign((size_t)vk::ia_inv_words(ia), 0xdeadbeefu);
            vk::launch_ia_basis(nullptr, ia, part.data());
            vk::launch_ia_merge(nullptr, ia, part.data(), inv[i].data());
            const uint32_t AW = a.width + 1, d = inv[i][1];
            if (inv[i][0] + d != AW || d > a.width) throw std::logic_error("the merged basis is inconsistent");
            std::vector<uint8_t> pivot(AW);
            for (uint32_t k = 0; k < AW; k++) pivot[k] = inv[i][2 + k] != 0;
            std::vector<vg::Fp> vec((size_t)d * AW);
            for (size_t k = 0; k < vec.size(); k++) vec[k] = vg::Fp::raw(inv[i][2 + AW + k]);
            invariant_audit_entries(cs, (uint32_t)i, pivot, vec, o.max_terms, rep.entries);
            ia.d = d;
            ia.vec = inv[i].data() + 2 + AW;
            if (!d) continue;
            // phase 2
            vk::ia_shape(ia);
            a.NW = 1;  // a wave is a workgroup here
            if (rows_per_wave) a.RPW = rows_per_wave;
            a.T = a.RPW;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            totals[i].assign(d, 0);
            table[i].assign((size_t)d * a.NB + 1, 0);
            prefix[i].assign((size_t)d * a.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_ia_count(nullptr, ia, totals[i].data(), table[i].data());
            for (uint32_t k = 0; k < d; k++) {
                InvariantEntry& en = rep.entries[e_at[i] + k];
                en.free_rows = totals[i][k];
                en.enforced = cs.height - en.free_rows;
            }
        }
        invariant_audit_finish(rep, o);
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            bool any = false;
            for (size_t e = e0; e < e1; e++) any |= rep.entries[e].free_rows != 0;
            if (any) {
                const vk::IaArgs& ia = args[chip];
                const uint32_t i_cut = (uint32_t)(e1 - e0);
                std::vector<uint32_t> rows((size_t)i_cut * R, 0);
                vk::launch_ra_scan(nullptr, ia.r, table[chip].data(), prefix[chip].data(), i_cut);
                vk::launch_ia_list(nullptr, ia, table[chip].data(), prefix[chip].data(), i_cut, R, rows.data());
                for (size_t e = e0; e < e1; e++) {
                    InvariantEntry& en = rep.entries[e];
                    const size_t listed = (size_t)std::min<uint64_t>(en.free_rows, R);
                    en.rows.assign(rows.begin() + (e - e0) * R, rows.begin() + (e - e0) * R + listed);
                }
            }
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "invariant_audit_emu: %s\n", ex.what());
        return -1;
    }
}
// ia_shape for a chip of the given sizes with d invariants, and what the passes that follow demand of the shape it chose: out = NW, RPW, T,
// NB, the bytes the enforcement kernel is launched with, the rank audit's bytes for the same shape.  Returns 0; 1 when ia_shape refuses the
// chip (std::invalid_argument, the documented refusal); -1 when the shape is accepted and the scan launcher the listing pass goes through
// (launch_ra_scan, here without columns: its checks only) then throws.
int32_t emu_ia_shape(uint32_t width, uint32_t prep_width, uint32_t K, uint32_t n_regs, uint32_t interpret, uint64_t n, uint32_t d, uint64_t* out) {
    vk::IaArgs ia{};
    vk::RaArgs& a = ia.r;
    a.width = width; a.prep_width = prep_width; a.K = K; a.n_regs = n_regs; a.n = n;
    a.native_chip = !K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : (int)vchips::CHIP_CPU);
    ia.d = d;
    try {
        vk::ia_shape(ia);
    } catch (const std::invalid_argument&) {
        return 1;
    }
    out[0] = a.NW; out[1] = a.RPW; out[2] = a.T; out[3] = a.NB;
    out[4] = vk::ia_lds_bytes(ia, a.NW, a.T); out[5] = vk::ra_lds_bytes(a, a.NW, a.T);
    try {
        vk::launch_ra_scan(nullptr, a, nullptr, nullptr, 0);
    } catch (const std::exception& ex) {
        fprintf(stderr, "invariant_audit_emu: w %u K %u d %u: %s\n", width, K, d, ex.what());
        return -1;
    }
    return 0;
}
}
