// The bus-audit kernels of valida_amd/csrc/kernels/bus_audit.hip — the very source — compiled for the HOST under tools/hipemu and run on host
// traces; checked against the numpy restatement of the contract (tests/test_bus_audit_cpu.py).  Everything runs under emulation — records,
// exact-path keys, heads, the group scan, the LDS-then-atomics reduction, selection, report — except the radix sort's scatter kernel, which
// ranks the lanes of a wave with __ballot: the emulator's fibers cannot model a wave, so the (key, id) pairs are sorted here with
// std::stable_sort (k_ba_sort_count and k_ba_scan_table, the other two thirds of a pass, are run and checked against the sorted keys).
// Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#define HIPEMU_STATIC_SHARED 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include <numeric>

inline unsigned long long __ballot(int) { throw std::runtime_error("hipemu: wave intrinsic (__ballot) reached"); }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call

#include "../../valida_amd/csrc/kernels/bus_audit.hip"
#include "../../valida_amd/csrc/host/bus_audit.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using namespace vhost;

namespace {
struct Emu {
    MachineDesc machine = MachineDesc::basic();
    BusPlan plan;
    std::vector<std::vector<uint32_t>> cols;  // column-major Montgomery copies (the prover's working layout)
    std::vector<uint32_t> desc;
    uint64_t n = 0;
    std::vector<unsigned long long> keys;
    std::vector<uint32_t> ids, cnt, gid, head_pos, nrec, counters, scan_tmp;
    std::vector<unsigned long long> sums;
    size_t NB = 0;

    static std::vector<uint32_t> working(const uint32_t* m, uint64_t h, uint64_t w) {
        std::vector<uint32_t> c(h * w);
        for (uint64_t r = 0; r < h; r++)
            for (uint64_t k = 0; k < w; k++) c[k * h + r] = vg::Fp::from_canonical(m[r * w + k]).v;
        return c;
    }
    void setup(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
               const uint64_t* ph, const uint64_t* pw, uint32_t n_prep) {
        std::vector<BusShape> ms, ps;
        std::vector<int> chips, prep_slot;
        for (uint32_t i = 0; i < n_main; i++) ms.push_back({heights[i], widths[i]});
        for (uint32_t k = 0; k < n_prep; k++) { ps.push_back({ph[k], pw[k]}); chips.push_back((int)prep_chips[k]); }
        plan = bus_audit_plan(machine, ms, chips, ps, prep_slot);
        const size_t NC = machine.airs.size();
        std::vector<const uint32_t*> mp(NC, nullptr), pp(NC, nullptr);
        std::vector<uint64_t> mst(NC, 0), pst(NC, 0);
        for (size_t i = 0; i < NC; i++) {
            cols.push_back(working(main[i], heights[i], widths[i]));
            mp[i] = cols.back().data(); mst[i] = heights[i];
        }
        for (size_t i = 0; i < NC; i++)
            if (prep_slot[i] >= 0) {
                const int k = prep_slot[i];
                cols.push_back(working(prep[k], ph[k], pw[k]));
                pp[i] = cols.back().data(); pst[i] = ph[k];
            }
        desc = bus_audit_descriptor(machine, plan, mp, mst, pp, pst);
        n = plan.n_slots; NB = plan.buses.size();
        uint32_t total_inter = 0;
        for (auto& c : plan.chips) total_inter += c.M;
        keys.assign(n, 0); ids.assign(n, 0); cnt.assign(n, 0); gid.assign(n, 0); head_pos.assign(n, 0); nrec.assign(2 * n, 0); sums.assign(2 * n, 0);
        counters.assign(8 + NB + total_inter, 0);
        scan_tmp.assign(vk::bus_audit_scan_scratch_words(n), 0);
    }
    void records(uint32_t hash_bits) {
        uint32_t base = 0;
        for (size_t i = 0; i < machine.airs.size(); i++) {
            vk::launch_ba_records(nullptr, desc.data(), (uint32_t)i, plan.chips[i].height, machine.airs[i].width, plan.chips[i].M, hash_bits, keys.data(), ids.data(), cnt.data(),
                                  counters.data() + 8 + NB + base);
            base += plan.chips[i].M;
        }
    }
    // the sort the device does with k_ba_sort_*: stable, by key; the digit histogram and its scan run under emulation and must agree
    void sort_pairs() {
        const uint32_t n_blocks = (uint32_t)((n + vk::BA_RS_BLOCK - 1) / vk::BA_RS_BLOCK);
        std::vector<uint32_t> table(256 * (size_t)n_blocks + 4, 0);
        const unsigned long long* kp = keys.data();
        uint32_t* tp = table.data();
        const uint64_t nn = n;
        hipLaunchKernelGGL(vk::k_ba_sort_count, dim3(n_blocks), dim3(256), 0, nullptr, kp, nn, 0, tp, n_blocks);
        hipLaunchKernelGGL(vk::k_ba_scan_table, dim3(1), dim3(1024), 0, nullptr, tp, (uint64_t)256 * n_blocks);
        std::vector<uint32_t> ord(n);
        std::iota(ord.begin(), ord.end(), 0u);
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (uint32_t dg = 0; dg < 256; dg++) {  // table[dg][0] = pairs whose low byte is below dg
            uint64_t below = 0;
            for (uint64_t i = 0; i < n; i++) below += (keys[i] & 255u) < dg;
            if (table[(size_t)dg * n_blocks] != below) throw std::runtime_error("digit table");
        }
        std::vector<unsigned long long> k2(n);
        std::vector<uint32_t> i2(n);
        for (uint64_t i = 0; i < n; i++) { k2[i] = keys[ord[i]]; i2[i] = ids[ord[i]]; }
        keys.swap(k2); ids.swap(i2);
    }
    void group_and_reduce(bool exact) {
        vk::launch_ba_groups(nullptr, desc.data(), keys.data(), ids.data(), n, exact, gid.data(), head_pos.data(), scan_tmp.data(), counters.data());
        vk::launch_ba_reduce(nullptr, desc.data(), ids.data(), cnt.data(), gid.data(), head_pos.data(), n, !exact, sums.data(), nrec.data(), counters.data());
        vk::launch_ba_select(nullptr, desc.data(), ids.data(), head_pos.data(), sums.data(), n, false, 0, nullptr, nullptr, counters.data());
    }
};
}  // namespace

extern "C" {
// Per record slot of the BasicMachine on these host traces (canonical row-major), from k_ba_records and the device's own tuple recomputation
// (ba_ref / ba_next_field, what the report and the exact path read): keys (u64), counts, and per slot [chip, row, interaction, is_send, bus is_global,
// bus index, wmax padded fields] in `tuples` (6 + wmax words a slot; dead slots zero).  Returns the slot count, or -1 when the emulator refused.
int64_t emu_bus_records(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                        const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t hash_bits, uint64_t cap, uint64_t* keys, uint32_t* counts, uint32_t* tuples, uint32_t* wmax_out) {
    try {
        Emu e;
        e.setup(main, heights, widths, n_main, prep_chips, prep, ph, pw, n_prep);
        *wmax_out = e.plan.wmax;
        if (e.n > cap) return (int64_t)e.n;
        e.records(hash_bits);
        const uint32_t stride = 6 + e.plan.wmax;
        for (uint64_t s = 0; s < e.n; s++) {
            keys[s] = e.keys[s]; counts[s] = e.cnt[s];
            if (e.ids[s] != s) return -1;
            uint32_t* o = tuples + s * stride;
            for (uint32_t k = 0; k < stride; k++) o[k] = 0;
            if (!e.cnt[s]) continue;
            vk::BaRef r = vk::ba_ref(e.desc.data(), (uint32_t)s);
            const BusRecord rec = e.plan.decode(s);
            if (rec.row != r.row || rec.interaction != r.m) return -1;
            o[0] = rec.chip; o[1] = r.row; o[2] = r.m; o[3] = r.is_send;
            o[4] = e.plan.buses[r.bus_slot].is_global; o[5] = e.plan.buses[r.bus_slot].bus_index;
            for (uint32_t j = 0; j < r.n_fields; j++) o[6 + j] = vk::ba_next_field(e.desc.data(), r);
        }
        return (int64_t)e.n;
    } catch (const std::exception& ex) {
        fprintf(stderr, "bus_audit_emu: %s\n", ex.what());
        return -1;
    }
}

// The whole pass under emulation (the sort on the host, see the header).  out: [0] live records [1] groups [2] colliding records seen by the key pass
// [3] unbalanced tuples [4] reported [5] stride of a report row [6] 1 when the exact path ran, then n_buses words (unbalanced tuples per bus slot), then the
// rows k_ba_report wrote (its layout).  Returns the words written or -1.
int64_t emu_bus_audit(const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main, const uint32_t* prep_chips, const uint32_t* const* prep,
                      const uint64_t* ph, const uint64_t* pw, uint32_t n_prep, uint32_t hash_bits, uint32_t max_tuples, uint32_t R, uint32_t* out, uint64_t cap) {
    try {
        Emu e;
        e.setup(main, heights, widths, n_main, prep_chips, prep, ph, pw, n_prep);
        e.records(hash_bits);
        e.sort_pairs();
        e.group_and_reduce(false);
        const uint32_t collided = e.counters[2];
        if (collided) {
            for (size_t k = 1; k < 8 + e.NB; k++) e.counters[k] = 0;
            std::fill(e.sums.begin(), e.sums.end(), 0ull);
            std::fill(e.nrec.begin(), e.nrec.end(), 0u);
            vk::launch_ba_iota(nullptr, e.ids.data(), e.n);
            for (int chunk = (int)(e.plan.wmax + 2) / 2 - 1; chunk >= 0; chunk--) {
                vk::launch_ba_rekey(nullptr, e.desc.data(), (uint32_t)chunk, e.ids.data(), e.cnt.data(), e.keys.data(), e.n);
                e.sort_pairs();
            }
            e.group_and_reduce(true);
        }
        const uint32_t n_unb = e.counters[3], n_rep = n_unb < max_tuples ? n_unb : max_tuples, stride = 8 + e.plan.wmax + 2 * R;
        std::vector<unsigned long long> uk(n_unb ? n_unb : 1);
        std::vector<uint32_t> uv(n_unb ? n_unb : 1), rows((size_t)n_rep * stride + 1);
        if (n_unb) {
            vk::launch_ba_select(nullptr, e.desc.data(), e.ids.data(), e.head_pos.data(), e.sums.data(), e.counters[1], true, n_unb, uk.data(), uv.data(), e.counters.data());
            std::vector<uint32_t> ord(n_unb), v2(n_unb);
            std::iota(ord.begin(), ord.end(), 0u);
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return uk[a] < uk[b]; });
            for (uint32_t i = 0; i < n_unb; i++) v2[i] = uv[ord[i]];
            vk::launch_ba_report(nullptr, e.desc.data(), e.ids.data(), e.cnt.data(), e.head_pos.data(), e.sums.data(), e.nrec.data(), v2.data(), n_rep, R, rows.data());
        }
        const uint64_t need = 7 + e.NB + (uint64_t)n_rep * stride;
        if (need > cap) return -1;
        out[0] = e.counters[0]; out[1] = e.counters[1]; out[2] = collided; out[3] = n_unb; out[4] = n_rep; out[5] = stride; out[6] = collided ? 1u : 0u;
        for (size_t b = 0; b < e.NB; b++) out[7 + b] = e.counters[8 + b];
        for (uint64_t k = 0; k < (uint64_t)n_rep * stride; k++) out[7 + e.NB + k] = rows[k];
        return (int64_t)need;
    } catch (const std::exception& ex) {
        fprintf(stderr, "bus_audit_emu: %s\n", ex.what());
        return -1;
    }
}
}
