// The transition-audit kernels of valida_amd/csrc/kernels/transition_audit.hip — the very source, with rank_elim.hpp — compiled for the HOST
// under tools/hipemu and run on host traces: the column flags, the gated streaming elimination (gates over gridDim.y), the merge tree, the
// enforcement pass, the count, the scan and the listing pass, driven as Prover::transition_audit drives them and assembled into the report's
// word image (tests/test_transition_audit_cpu.py compares it with the host audit).  The wave primitives get the emulation forms of
// tests/emu/rank_audit_emu.cpp: a ballot goes through two LDS words between __syncthreads(), a wave sync is __syncthreads().  In the
// elimination and enforcement kernels a workgroup is ONE wave here (NW = 1); the flags kernel runs its four waves (their ballots are called in
// lockstep).  machine = 0: the BasicMachine; 2: one AIR of widths[0] columns without constraints or interactions ("free"); 4: one AIR of
// widths[0] columns with the one constraint when_transition (next.c0 - c0 - 1) ("step").  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
namespace vk {
uint32_t ta_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
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

#include "../../valida_amd/csrc/kernels/transition_audit.hip"
#include "../../valida_amd/csrc/host/transition_audit.hpp"

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

MachineDesc single(int width, bool step) {
    MachineDesc m;
    vair::Dag d;
    d.width = width; d.prep_width = 0;
    if (step) {
        const uint32_t s = d.sub(d.sub(d.var(false, 0, true), d.var(false, 0, false)), d.constant(1));
        d.constraints.push_back(d.mul(d.selector(vair::N_TRANS), s));
    }
    m.airs.push_back(MachineDesc::make_air_from_dag(step ? "step" : "free", d, {}));
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces): interpret = 0 runs the compiled chip templates (machine 0 only),
// 1 the register programs; rows_per_wave = 0 keeps ta_shape's rows per wave, another number forces that many (also the rows per workgroup);
// windows_per_slice = 0 keeps ta_basis_shape's slice, another number forces that many; windows_per_count = 0 keeps ta_shape's windows per
// workgroup of the count and list passes; entries_per_chunk = 0 keeps ta_shape's chunk.  out: the report's word image.  Returns the words
// written, or -1.
int64_t emu_transition_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                             const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_wave, uint32_t windows_per_slice,
                             uint32_t windows_per_count, uint32_t entries_per_chunk, uint32_t max_entries, uint32_t R, uint32_t max_terms, uint32_t min_gate_windows, uint32_t max_gates,
                             uint32_t chip_mask, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = machine_kind == 0 ? MachineDesc::basic() : single((int)widths[0], machine_kind == 4);
        TransitionAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask; o.max_terms = max_terms; o.min_gate_windows = min_gate_windows; o.max_gates = max_gates;
        o = transition_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        transition_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        TransitionReport rep;
        rep.chips.resize(NC);
        std::vector<vk::TaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), wr(NC);
        std::vector<size_t> g_at(NC + 1, 0);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            args[i] = vk::TaArgs{};
            vk::TaArgs& ta = args[i];
            vk::RaArgs& a = ta.r;
            TransitionChipStat& cs = rep.chips[i];
            transition_audit_chip_block(cs, air, heights[i], transition_audit_selected(o, i));
            g_at[i] = rep.gates.size();
            if (!transition_audit_has_windows(cs)) continue;
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
            vk::ta_basis_shape(ta, o.max_gates);
            ta.E = 0;
            vk::ta_shape(ta);
            // the flags
            const uint32_t W = a.width, AW = 2 * W + 1;
            std::vector<uint32_t> fl(AW, 0);
            std::vector<unsigned long long> ones(AW, 0);
            vk::launch_ta_flags(nullptr, ta, fl.data(), ones.data());
            transition_audit_gates(cs, (uint32_t)i, fl, std::vector<uint64_t>(ones.begin(), ones.end()), o, rep.gates);
            // phase 1
            std::vector<uint32_t> gw;
            std::vector<size_t> which;
            for (size_t g = g_at[i]; g < rep.gates.size(); g++) {
                if (!rep.gates[g].audited) continue;
                gw.push_back(rep.gates[g].column); gw.push_back(rep.gates[g].value ? vg::Fp::one().v : 0u);
                which.push_back(g);
            }
            ta.G = (uint32_t)which.size();
            vk::ta_basis_shape(ta, ta.G);
            if (windows_per_slice) { ta.RB = windows_per_slice; ta.NB1 = (uint32_t)((a.n - 1 + ta.RB - 1) / ta.RB); }
            ta.gates = gw.data();
            const uint64_t inv_words = vk::ta_inv_words(ta);
            std::vector<uint32_t> part((size_t)vk::ta_part_words(ta), 0xdeadbeefu), inv((size_t)(ta.G * inv_words), 0xdeadbeefu);  // the merge reads only what a workgroup wrote
            vk::launch_ta_basis(nullptr, ta, part.data());
            vk::launch_ta_merge(nullptr, ta, part.data(), inv.data());
            TransitionBasis b0;
            for (size_t k = 0; k < which.size(); k++) {
                const uint32_t* v = inv.data() + k * inv_words;
                const uint32_t d = v[1];
                if (v[0] + d != AW || d >= AW) throw std::logic_error("the merged basis is inconsistent");
                TransitionBasis b;
                b.pivot.resize(AW);
                for (uint32_t x = 0; x < AW; x++) b.pivot[x] = v[2 + x] != 0;
                b.vec.resize((size_t)d * AW);
                for (size_t x = 0; x < b.vec.size(); x++) b.vec[x] = vg::Fp::raw(v[2 + AW + x]);
                if (k == 0) b0 = b;
                transition_audit_entries(cs, rep.gates[which[k]], b0, b, o.max_terms, rep.entries);
            }
            ta.gates = nullptr;
        }
        g_at[NC] = rep.gates.size();
        transition_audit_cut(rep, o);
        // phase 2
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            vk::TaArgs& ta = args[chip];
            vk::RaArgs& a = ta.r;
            const uint32_t W = a.width, E = (uint32_t)(e1 - e0);
            std::vector<uint32_t> ev((size_t)E * 2 * W), eg((size_t)E * 4, 0);
            std::vector<uint64_t> windows(E, 0);
            for (uint32_t k = 0; k < E; k++) {
                const TransitionEntry& en = rep.entries[e0 + k];
                uint32_t nz = 0;
                for (uint32_t x = 0; x < 2 * W; x++) { ev[(size_t)k * 2 * W + x] = en.l[1 + x].v; if (en.l[1 + x].v) nz |= x < W ? 1u : 2u; }
                eg[4 * (size_t)k] = en.gate_column; eg[4 * (size_t)k + 1] = en.gate_value ? vg::Fp::one().v : 0u; eg[4 * (size_t)k + 2] = nz;
                for (size_t g = g_at[chip]; g < g_at[chip + 1]; g++)
                    if (rep.gates[g].chip == chip && rep.gates[g].column == en.gate_column && rep.gates[g].value == en.gate_value) windows[k] = rep.gates[g].windows;
            }
            ta.E = E;
            vk::ta_shape(ta);
            a.NW = 1;  // a wave is a workgroup here
            if (rows_per_wave) a.RPW = rows_per_wave;
            a.T = a.RPW;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            if (entries_per_chunk) ta.EC = std::min(E, entries_per_chunk);
            if (windows_per_count) { ta.WPB = windows_per_count; ta.NB2 = (uint32_t)((a.n - 1 + ta.WPB - 1) / ta.WPB); }
            ta.evec = ev.data(); ta.egate = eg.data();
            std::vector<uint32_t> bits((size_t)vk::ta_bits_words(ta), 0xdeadbeefu);  // the enforcement pass must write what the count reads
            const uint64_t tab = (uint64_t)E * ta.NB2;
            std::vector<unsigned long long> totals(E, 0);
            std::vector<uint32_t> table((size_t)tab, 0), prefix((size_t)tab, 0xdeadbeefu), rows((size_t)E * R, 0);
            vk::launch_ta_enforce(nullptr, ta, bits.data());
            vk::launch_ta_count(nullptr, ta, bits.data(), totals.data(), table.data());
            bool any = false;
            for (uint32_t k = 0; k < E; k++) {
                TransitionEntry& en = rep.entries[e0 + k];
                en.free_windows = totals[k];
                if (en.free_windows > windows[k]) throw std::logic_error("more free windows than the gate has");
                en.held_windows = windows[k] - en.free_windows;
                any |= en.free_windows != 0;
            }
            if (any) {
                vk::launch_ta_scan(nullptr, ta, table.data(), prefix.data());
                vk::launch_ta_list(nullptr, ta, bits.data(), table.data(), prefix.data(), R, rows.data());
                for (uint32_t k = 0; k < E; k++) {
                    TransitionEntry& en = rep.entries[e0 + k];
                    const size_t listed = (size_t)std::min<uint64_t>(en.free_windows, R);
                    en.rows.assign(rows.begin() + (size_t)k * R, rows.begin() + (size_t)k * R + listed);
                }
            }
            ta.evec = ta.egate = nullptr;
            e0 = e1;
        }
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "transition_audit_emu: %s\n", ex.what());
        return -1;
    }
}
// ta_basis_shape for a chip of `width` columns: 0 accepted, 1 refused (std::invalid_argument, the documented refusal)
int32_t emu_ta_basis_shape(uint32_t width, uint64_t n, uint32_t gates, uint64_t* out) {
    vk::TaArgs ta{};
    ta.r.width = width; ta.r.n = n;
    try {
        vk::ta_basis_shape(ta, gates);
    } catch (const std::invalid_argument&) {
        return 1;
    }
    out[0] = ta.RB; out[1] = ta.NB1; out[2] = vk::ta_basis_lds_bytes(width);
    return 0;
}
}
