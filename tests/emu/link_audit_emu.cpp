// The link-audit kernels of valida_amd/csrc/kernels/link_audit.hip — the very source — compiled for the HOST under tools/hipemu together with
// the bus audit's (kernels/bus_audit.hip, whose launchers group the records) and run on host traces: the mask pass for the compiled chip
// templates, the interpreted register programs and the bus-only chips, records, groups, reduce, the exact path after a key collision, join,
// tally, select and report, driven as Prover::link_audit drives them and assembled into the report's word image
// (tests/test_link_audit_cpu.py compares it with the host audit).  The two wave-level helpers of the elimination, fa_ballot and fa_wave_sync,
// get their emulation forms here (a wave is a 64-thread workgroup, a ballot goes through two LDS words between __syncthreads()); the radix
// sort's scatter kernel ranks lanes with __ballot, which fibers cannot model, so the (key, id) pairs are sorted with std::stable_sort, as in
// tests/emu/bus_audit_emu.cpp.  What the emulation does not reach is the hardware itself: the real ballot and wave barrier, the real atomics
// between workgroups, the LDS opt-in above 64 KB and the launch shapes la_shape picks for tall traces.  Test infrastructure; nothing in the
// product links it.
#define HIPEMU_CHECKS 1
#define HIPEMU_STATIC_SHARED 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include <numeric>

inline unsigned long long __ballot(int) { throw std::runtime_error("hipemu: wave intrinsic (__ballot) reached"); }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
template <class T> inline T atomicAnd(T* p, T v) { T o = *p; *p = o & v; return o; }

#include "../../valida_amd/csrc/kernels/bus_audit.hip"  // static __shared__ arrays: one function-local static per kernel

// link_audit.hip keeps all its LDS in one dynamic array: it resolves to the global below
#undef __shared__
#define __shared__
#define VGPU_FA_WAVE_PRIMS 1
namespace vk {
uint32_t la_lds[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
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

#include "../../valida_amd/csrc/kernels/link_audit.hip"
#include "../../valida_amd/csrc/host/link_audit.hpp"

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
// the sort the device does with k_ba_sort_*: stable, by key
void sort_pairs(std::vector<unsigned long long>& keys, std::vector<uint32_t>& ids) {
    const size_t n = keys.size();
    std::vector<uint32_t> ord(n);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<unsigned long long> k2(n);
    std::vector<uint32_t> i2(n);
    for (size_t i = 0; i < n; i++) { k2[i] = keys[ord[i]]; i2[i] = ids[ord[i]]; }
    keys.swap(k2); ids.swap(i2);
}
}  // namespace

extern "C" {
// The whole device pass under emulation on the BasicMachine (canonical row-major host traces): interpret = 0 runs the compiled chip templates,
// 1 the register programs; rows_per_workgroup = 0 keeps la_shape's, another number forces that many (a small one makes halos, wraps and the
// reuse of a bus-only chip's masks cross workgroups).  The masks are computed once, then the records are grouped, joined and reported once per
// entry of hash_bits.  out: the report images one after the other, each preceded by one word: 1 when the exact path ran.  Returns the words
// written, or -1.
int64_t emu_link_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                       const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t interpret, uint32_t rows_per_workgroup, uint32_t max_tuples, uint32_t R,
                       const uint32_t* hash_bits, uint32_t n_hash, uint32_t* out, uint64_t cap) {
    try {
        const MachineDesc machine = MachineDesc::basic();
        std::vector<BusShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        const BusPlan plan = link_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size(), NB = plan.buses.size();
        const uint64_t n = plan.n_slots;
        LinkReport blank;
        link_audit_blocks(blank, machine, plan);
        std::vector<vk::FaArgs> args(NC);
        std::vector<std::vector<uint32_t>> mcols(NC), pcols(NC), wr(NC);
        std::vector<const uint32_t*> mp(NC, nullptr), pp(NC, nullptr);
        std::vector<uint64_t> mst(NC, 0), pst(NC, 0);
        std::vector<uint32_t> lt(4 + NC, 0);
        uint32_t n_fields = 0;
        std::vector<uint32_t> mask(n ? n : 1, 0);
        for (size_t i = 0; i < NC; i++) {
            const AirDesc& air = machine.airs[i];
            vk::FaArgs& a = args[i];
            a = vk::FaArgs{};
            lt[4 + i] = (uint32_t)lt.size();
            for (auto& it : blank.chips[i]) { lt.push_back(n_fields); n_fields += it.n_fields; }
            mcols[i] = working(main[i], heights[i], widths[i]);
            mp[i] = mcols[i].data(); mst[i] = heights[i];
            if (prep_slot[i] >= 0) { const int k = prep_slot[i]; pcols[i] = working(prep[k], ph[k], pw[k]); pp[i] = pcols[i].data(); pst[i] = ph[k]; }
            if (!air.width || air.interactions.empty()) continue;
            wr[i] = ra_weight_rows(air);
            a.K = air.program.num_asserts;
            a.main = mp[i]; a.mstride = mst[i]; a.prep = pp[i]; a.pstride = pst[i];
            a.n = heights[i]; a.width = air.width; a.prep_width = air.prep_width;
            a.prog = air.program.instrs.data();
            a.n_instrs = (uint32_t)air.program.instrs.size();
            a.n_regs = air.program.num_regs;
            a.iw = air.interaction_words.data();
            a.wr = wr[i].data();
            a.M = (uint32_t)air.interactions.size();
            for (auto& it : blank.chips[i]) { a.NS += it.n_fields; a.F = std::max(a.F, it.n_fields); }
            a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret ? vk::CA_INTERPRET : air.native_chip);
            vk::la_shape(a);
            if (rows_per_workgroup) a.T = rows_per_workgroup;
            a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
            vk::launch_la_masks(nullptr, a, (uint32_t)plan.chips[i].first_id, mask.data());
        }
        lt[0] = n_fields;
        const std::vector<uint32_t> desc = bus_audit_descriptor(machine, plan, mp, mst, pp, pst);
        uint32_t total_inter = 0;
        std::vector<uint32_t> inter_base(NC, 0);
        for (size_t i = 0; i < NC; i++) { inter_base[i] = total_inter; total_inter += plan.chips[i].M; }
        const uint64_t tally_words = vk::la_tally_words(n_fields, (uint32_t)NB);
        uint64_t at = 0;
        for (uint32_t hk = 0; hk < n_hash; hk++) {
            LinkAuditOpts o;
            o.max_tuples = max_tuples; o.max_records_per_tuple = R; o.hash_bits = hash_bits[hk];
            o = link_audit_checked_opts(o);
            LinkReport rep = blank;
            std::vector<unsigned long long> keys(n ? n : 1, 0), sums(2 * n + 2, 0), tally(tally_words + 1, 0);
            std::vector<uint32_t> ids(n ? n : 1, 0), cnt(n ? n : 1, 0), gid(n ? n : 1, 0), head_pos(n ? n : 1, 0), nrec(2 * n + 2, 0), counters(8 + NB + total_inter, 0),
                scan_tmp(vk::bus_audit_scan_scratch_words(n ? n : 1), 0), tmask(n ? n : 1, 0);
            for (size_t i = 0; i < NC; i++)
                vk::launch_ba_records(nullptr, desc.data(), (uint32_t)i, plan.chips[i].height, machine.airs[i].width, plan.chips[i].M, o.hash_bits, keys.data(), ids.data(), cnt.data(),
                                      counters.data() + 8 + NB + inter_base[i]);
            keys.resize(n); ids.resize(n);
            sort_pairs(keys, ids);
            vk::launch_ba_groups(nullptr, desc.data(), keys.data(), ids.data(), n, false, gid.data(), head_pos.data(), scan_tmp.data(), counters.data());
            vk::launch_ba_reduce(nullptr, desc.data(), ids.data(), cnt.data(), gid.data(), head_pos.data(), n, true, sums.data(), nrec.data(), counters.data());
            const uint32_t collided = counters[2];
            if (collided) {
                for (size_t k = 1; k < 8 + NB; k++) counters[k] = 0;
                std::fill(sums.begin(), sums.end(), 0ull);
                std::fill(nrec.begin(), nrec.end(), 0u);
                vk::launch_ba_iota(nullptr, ids.data(), n);
                for (int chunk = (int)(plan.wmax + 2) / 2 - 1; chunk >= 0; chunk--) {
                    vk::launch_ba_rekey(nullptr, desc.data(), (uint32_t)chunk, ids.data(), cnt.data(), keys.data(), n);
                    sort_pairs(keys, ids);
                }
                vk::launch_ba_groups(nullptr, desc.data(), keys.data(), ids.data(), n, true, gid.data(), head_pos.data(), scan_tmp.data(), counters.data());
                vk::launch_ba_reduce(nullptr, desc.data(), ids.data(), cnt.data(), gid.data(), head_pos.data(), n, false, sums.data(), nrec.data(), counters.data());
            }
            const uint32_t n_live = counters[0], n_groups = counters[1];
            std::fill(tmask.begin(), tmask.begin() + n_groups, 0xffffffffu);
            vk::launch_la_join(nullptr, ids.data(), mask.data(), gid.data(), n_live, tmask.data());
            vk::launch_la_tally(nullptr, desc.data(), lt.data(), ids.data(), mask.data(), gid.data(), head_pos.data(), tmask.data(), n_live, n_fields, (uint32_t)NB, tally.data());
            uint64_t n_open = 0;
            for (size_t i = 0; i < NC; i++)
                for (size_t m = 0; m < rep.chips[i].size(); m++) {
                    LinkInteractionStat& s = rep.chips[i][m];
                    s.live_rows = counters[8 + NB + inter_base[i] + m];
                    rep.buses[plan.chips[i].bus_slot[m]].live += s.live_rows;
                    const uint32_t slot = lt[lt[4 + i] + m];
                    for (uint32_t j = 0; j < s.n_fields; j++) { s.floating[j] = tally[slot + j]; s.open[j] = tally[(uint64_t)n_fields + slot + j]; }
                }
            for (size_t b = 0; b < NB; b++) {
                LinkBusStat& bs = rep.buses[b];
                const uint64_t bb = 2ull * n_fields + 66ull * b;
                bs.tuples = tally[bb]; bs.open_tuples = tally[bb + 1];
                for (uint32_t j = 0; j < bs.width; j++) { bs.open_in[j] = tally[bb + 2 + j]; bs.open_records[j] = tally[bb + 34 + j]; }
                n_open += bs.open_tuples;
            }
            rep.total_open = n_open;
            if (n_open) {
                const uint32_t n_rep = (uint32_t)std::min<uint64_t>(n_open, o.max_tuples), stride = 8 + plan.wmax + 2 * R;
                std::vector<unsigned long long> uk(n_open);
                std::vector<uint32_t> uv(n_open), rows((size_t)n_rep * stride + 1);
                vk::launch_la_select(nullptr, ids.data(), head_pos.data(), tmask.data(), n_groups, (uint32_t)n_open, uk.data(), uv.data(), counters.data());
                if (counters[4] != n_open) throw std::runtime_error("select and tally disagree on the open tuples");
                sort_pairs(uk, uv);
                vk::launch_la_report(nullptr, desc.data(), ids.data(), mask.data(), head_pos.data(), nrec.data(), tmask.data(), uv.data(), n_rep, R, rows.data());
                for (uint32_t t = 0; t < n_rep; t++) {
                    const uint32_t* e = rows.data() + (size_t)t * stride;
                    const BusStat& bus = plan.buses.at(e[0]);
                    LinkTuple lk;
                    lk.is_global = bus.is_global; lk.bus_index = bus.bus_index; lk.mask = e[2];
                    lk.fields.assign(e + 8, e + 8 + bus.width);
                    lk.n_send = e[3]; lk.n_recv = e[4];
                    for (uint32_t k = 0; k < e[1] && k < R; k++) {
                        const BusRecord r = plan.decode(e[8 + plan.wmax + 2 * k]);
                        lk.records.push_back(LinkRecord{r.chip, r.row, r.interaction, machine.airs[r.chip].interactions[r.interaction].is_send() ? 1u : 0u, e[8 + plan.wmax + 2 * k + 1]});
                    }
                    rep.tuples.push_back(std::move(lk));
                }
            }
            link_audit_finish(rep, o);
            const std::vector<uint32_t> w = rep.words();
            if (at + 1 + w.size() > cap) return -1;
            out[at++] = collided ? 1u : 0u;
            for (size_t k = 0; k < w.size(); k++) out[at++] = w[k];
        }
        return (int64_t)at;
    } catch (const std::exception& ex) {
        fprintf(stderr, "link_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
