// The product-audit kernels of valida_amd/csrc/kernels/product_audit.hip — the very source, with rank_elim.hpp, the invariant audit's basis and
// merge kernels and the rank audit's scan kernel — compiled for the HOST under tools/hipemu and run on host traces: the pivots, the basis rows
// per slice and their ordered merge, the inverse, beta, the prefix sweep, the compaction, the survivor sweep, the gather, the counting pass, the
// scan over workgroups and the listing pass, driven as Prover::product_audit drives them and assembled into the report's word image
// (tests/test_product_audit_cpu.py compares it with the host audit).  The wave primitives get the emulation forms of
// tests/emu/rank_audit_emu.cpp: a wave is a 64-thread workgroup, a ballot goes through two LDS words between __syncthreads(), a wave sync is
// __syncthreads().  A workgroup of the enforcement phase is ONE wave here (NW = 1); more than one wave per workgroup is covered by the GPU tests
// alone.  machine = 0: the BasicMachine; 1: one AIR of widths[0] columns with the constraints c1^2 - c1 and c1 c2 - c3 ("quad"); 2: one AIR of
// widths[0] columns without constraints or interactions ("free").  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
#define VGPU_RA_WAVE_PRIMS 1
namespace vk {
uint32_t ra_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
uint32_t ia_lds[40 * 1024];
uint32_t pq_lds[40 * 1024];
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
#include "../../valida_amd/csrc/kernels/product_audit.hip"
#include "../../valida_amd/csrc/host/product_audit.hpp"

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

MachineDesc single(int width, bool quad) {
    MachineDesc m;
    vair::Dag d;
    d.width = width; d.prep_width = 0;
    if (quad) {
        const uint32_t c1 = d.var(false, 1, false), c2 = d.var(false, 2, false), c3 = d.var(false, 3, false);
        d.constraints.push_back(d.sub(d.mul(c1, c1), c1));
        d.constraints.push_back(d.sub(d.mul(c1, c2), c3));
    }
    m.airs.push_back(MachineDesc::make_air_from_dag(quad ? "quad" : "free", d, {}));
    return m;
}
}  // namespace

extern "C" {
// The whole device pass under emulation (canonical row-major host traces): interpret = 0 runs the compiled chip templates (machine 0 only),
// 1 the register programs; rows_per_wave = 0 keeps pq_shape's rows per wave, another number forces that many (also the rows per workgroup);
// rows_per_slice = 0 keeps the slices of ia_basis_shape and pq_rows_shape, another number forces that many rows per slice in both;
// prefix_rows = 0 keeps the prefix sweep's 256 rows; group_entries / group_words = 0 keep the entry groups' caps.  out: the report's word image.
// stats (8 words, may be null): the most slices of the basis-row phase, the pairs, the survivors of the prefix sweeps, the relations, the most
// groups of a chip.  Returns the words written, or -1.
int64_t emu_product_audit(uint32_t machine_kind, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips,
                          const uint32_t* const* prep, const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_wave, uint32_t rows_per_slice,
                          uint32_t prefix_rows_in, uint32_t group_entries, uint32_t group_words, uint32_t max_entries, uint32_t R, uint32_t max_terms, uint32_t chip_mask, uint32_t* out,
                          uint64_t cap, uint64_t* stats) {
    try {
        const MachineDesc machine = machine_kind == 0 ? MachineDesc::basic() : single((int)widths[0], machine_kind == 1);
        ProductAuditOpts o;
        o.max_entries = max_entries; o.max_rows_per_entry = R; o.chip_mask = chip_mask; o.max_terms = max_terms;
        o = product_audit_checked_opts(o, machine.airs.size());
        std::vector<ConstraintShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        product_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        ProductReport rep;
        rep.chips.resize(NC);
        std::vector<vk::PqArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols_dev(NC), pcols_main(NC), table(NC), prefix(NC), wr(NC);
        std::vector<ProductLists> lists(NC);
        std::vector<std::vector<unsigned long long>> totals(NC);
        std::vector<ProductVec> vecs;
        std::vector<size_t> e_at(NC + 1, 0);
        uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            args[i] = vk::PqArgs{};
            vk::PqArgs& pa = args[i];
            vk::IaArgs ia{};
            vk::RaArgs& a = ia.r;
            ProductChipStat& cs = rep.chips[i];
            product_audit_chip_block(cs, air, heights[i], product_audit_selected(o, i));
            e_at[i] = rep.entries.size();
            if (!cs.audited || !air.width) continue;
            a.K = air.program.num_asserts;
            mcols[i] = working(main[i], heights[i], widths[i]);
            a.main = mcols[i].data(); a.mstride = heights[i]; a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols_main[i] = working(prep[k], ph[k], pw[k]); a.prep = pcols_main[i].data(); a.pstride = ph[k]; }
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            wr[i] = ra_weight_rows(air);
            a.wr = wr[i].data();
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : ((interpret || machine_kind) ? vk::CA_INTERPRET : air.native_chip);
            // (1) the pivots
            vk::ia_basis_shape(ia);
            ia.d = air.width;
            vk::ia_shape(ia);  // the up-front refusal of the device pass
            if (rows_per_slice) { ia.RB = rows_per_slice; ia.NB1 = (uint32_t)((a.n + ia.RB - 1) / ia.RB); }
            std::vector<uint32_t> part((size_t)vk::ia_part_words(ia), 0xdeadbeefu), inv((size_t)vk::ia_inv_words(ia), 0xdeadbeefu);
            vk::launch_ia_basis(nullptr, ia, part.data());
            vk::launch_ia_merge(nullptr, ia, part.data(), inv.data());
            const uint32_t AW = a.width + 1;
            std::vector<uint32_t> pcols;
            for (uint32_t k = 0; k < AW; k++) if (inv[2 + k]) pcols.push_back(k);
            if (inv[0] != pcols.size() || pcols.empty() || pcols[0] != 0) throw std::logic_error("the merged basis is inconsistent");
            product_audit_space(cs, pcols);
            pa.r = a;
            pa.rho = (uint32_t)pcols.size();
            if (pa.rho < 2) continue;
            const uint32_t rho = pa.rho, m = (uint32_t)vk::pq_pairs(rho);
            pcols_dev[i] = pcols;
            pa.pcols = pcols_dev[i].data();
            // (2) the basis rows
            vk::pq_rows_shape(pa);
            if (rows_per_slice) { pa.RS = rows_per_slice; pa.NB2 = (uint32_t)((a.n + pa.RS - 1) / pa.RS); }
            st[0] = std::max<uint64_t>(st[0], pa.NB2);
            std::vector<uint32_t> slots((size_t)vk::pq_rows_words(pa), 0xdeadbeefu), rows(rho + 1, 0), status(1, 0xdeadbeefu), count(1, 0xdeadbeefu);
            vk::launch_pq_rows(nullptr, pa, slots.data());
            vk::launch_pq_rowmerge(nullptr, pa, slots.data(), rows.data());
            if (rows[0] != rho) throw std::logic_error("the merge did not find rho basis rows");
            // (3) the inverse and beta
            std::vector<uint32_t> aug(vk::pq_solve_in_lds(rho) ? 1 : 2 * (size_t)rho * rho, 0xdeadbeefu), G((size_t)rho * rho, 0xdeadbeefu), inverse((size_t)rho * rho, 0xdeadbeefu);
            std::vector<uint32_t> beta((size_t)m * rho, 0xdeadbeefu), flags(m, 0xdeadbeefu), l1(m, 0xdeadbeefu), l2(m, 0xdeadbeefu);
            vk::launch_pq_solve(nullptr, pa, rows.data(), aug.data(), G.data(), inverse.data(), status.data());
            if (status[0] != 0) throw std::logic_error("the basis rows are not independent");
            vk::launch_pq_beta(nullptr, pa, G.data(), inverse.data(), beta.data(), flags.data());
            // (4) the sweeps
            const uint64_t prefix_rows = std::min<uint64_t>(a.n, prefix_rows_in ? prefix_rows_in : vk::PQ_PREFIX_ROWS);
            vk::launch_pq_sweep(nullptr, pa, "k_pq_sweep.prefix", prefix_rows, beta.data(), nullptr, m, flags.data());
            vk::launch_pq_compact(nullptr, flags.data(), nullptr, m, l1.data(), count.data());
            uint32_t n_rel = count[0];
            if (n_rel > m) throw std::logic_error("more survivors than pairs");
            st[1] += m; st[2] += n_rel;
            const uint32_t* rel_dev = l1.data();
            if (n_rel && prefix_rows < a.n) {
                vk::launch_pq_sweep(nullptr, pa, "k_pq_sweep.survivors", a.n, beta.data(), l1.data(), n_rel, flags.data());
                vk::launch_pq_compact(nullptr, flags.data(), l1.data(), n_rel, l2.data(), count.data());
                if (count[0] > n_rel) throw std::logic_error("more relations than survivors");
                n_rel = count[0];
                rel_dev = l2.data();
            }
            st[3] += n_rel;
            if (!n_rel) continue;
            std::vector<uint32_t> rel(rel_dev, rel_dev + n_rel), betas((size_t)n_rel * rho, 0xdeadbeefu);
            vk::launch_pq_gather(nullptr, pa, beta.data(), rel_dev, n_rel, betas.data());
            product_audit_chip_entries(cs, (uint32_t)i, pcols, rel, betas, o.max_terms, rep.entries, vecs);
            // (5) enforcement
            lists[i] = product_audit_lists(vecs.data() + e_at[i], n_rel, group_entries ? group_entries : vk::PQ_GROUP_ENTRIES, group_words ? group_words : vk::PQ_GROUP_WORDS);
            const ProductLists& l = lists[i];
            pa.E = n_rel; pa.G = (uint32_t)l.gstart.size() - 1; pa.GE = l.GE; pa.GW = l.GW;
            pa.eoff = l.eoff.data(); pa.ewords = l.ewords.data(); pa.gstart = l.gstart.data();
            st[4] = std::max<uint64_t>(st[4], pa.G);
            vk::pq_shape(pa);
            pa.r.NW = 1;  // a wave is a workgroup here
            if (rows_per_wave) pa.r.RPW = rows_per_wave;
            pa.r.T = pa.r.RPW;
            pa.r.NB = (uint32_t)((a.n + pa.r.T - 1) / pa.r.T);
            totals[i].assign(2 * (size_t)n_rel, 0);
            table[i].assign((size_t)n_rel * pa.r.NB + 1, 0);
            prefix[i].assign((size_t)n_rel * pa.r.NB + 1, 0xdeadbeefu);  // the scan must write what the listing pass reads
            vk::launch_pq_count(nullptr, pa, totals[i].data(), table[i].data());
            for (uint32_t k = 0; k < n_rel; k++) {
                ProductEntry& en = rep.entries[e_at[i] + k];
                en.free_rows = totals[i][2 * k];
                en.flat_rows = totals[i][2 * k + 1];
                en.enforced = cs.height - en.free_rows;
            }
        }
        product_audit_finish(rep, o);
        for (size_t e0 = 0; e0 < rep.entries.size();) {
            const uint32_t chip = rep.entries[e0].chip;
            size_t e1 = e0;
            while (e1 < rep.entries.size() && rep.entries[e1].chip == chip) e1++;
            bool any = false;
            for (size_t e = e0; e < e1; e++) any |= rep.entries[e].free_rows != 0;
            if (any) {
                const vk::PqArgs& pa = args[chip];
                const uint32_t i_cut = (uint32_t)(e1 - e0);
                std::vector<uint32_t> rows((size_t)i_cut * R, 0);
                vk::launch_ra_scan(nullptr, pa.r, table[chip].data(), prefix[chip].data(), i_cut);
                vk::launch_pq_list(nullptr, pa, table[chip].data(), prefix[chip].data(), i_cut, R, rows.data());
                for (size_t e = e0; e < e1; e++) {
                    ProductEntry& en = rep.entries[e];
                    const size_t listed = (size_t)std::min<uint64_t>(en.free_rows, R);
                    en.rows.assign(rows.begin() + (e - e0) * R, rows.begin() + (e - e0) * R + listed);
                }
            }
            e0 = e1;
        }
        if (stats) for (int k = 0; k < 8; k++) stats[k] = st[k];
        const std::vector<uint32_t> w = rep.words();
        if (w.size() > cap) return -1;
        for (size_t k = 0; k < w.size(); k++) out[k] = w[k];
        return (int64_t)w.size();
    } catch (const std::exception& ex) {
        fprintf(stderr, "product_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
