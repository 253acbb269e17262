// Domain audit on the device (host/domain_audit.hpp: the contract; Prover::domain_audit drives these), per chip, wave64.
//   scan      k_da_scan, grid (S, NV), 256 threads: workgroup (x, y) streams the rows of slice x (TPS tiles of 256 rows) of virtual column y: a
//             main column (column-major: lane <-> row, coalesced) or a field vcol gated by its interaction's count, evaluated per row from its
//             terms.  Lane-local min / max / counts are reduced by wave shuffles, then over the four waves through LDS: one atomicMax (~min),
//             one atomicMax (max) and one atomicAdd per count and workgroup into the slot's totals.  A value < 2^16 sets a bit of an 8 KB LDS
//             bitmap by atomicOr; a wave whose live lanes all hold one value (one ballot compare against the first live lane's value) lets that
//             lane alone set it: a constant or flag column would otherwise serialise 64 lanes on one bank.  At the end the workgroup ORs its
//             non-zero bitmap words into the slot's 2048-word bitmap in device memory.  With 9.1 KB of LDS and 4 waves a workgroup, the 8 waves
//             per SIMD of 256-thread workgroups (8 workgroups per CU, 73 KB of its 160 KB) bound the occupancy, not the LDS.
//   classify  k_da_classify, one workgroup per slot: the popcount of its bitmap, dense, bits, the class and the narrow flag.
//   guard     k_da_guard, one thread per row, 256 rows per workgroup: the chip's guard table is staged in LDS once per workgroup; per column with
//             items (or narrow) the thread evaluates each item's count vcol and forms the row's guarded / sent / received / mixed bit and
//             "unguarded and non-zero"; counts go per wave by ballots into LDS counters, then one atomicAdd per non-zero counter and workgroup.
//             MA_COUNT also writes table[column][workgroup] for narrow columns; MA_LIST (after launch_ra_scan) writes the rows whose rank in
//             the column (prefix + waves before + lanes before) is below R: no atomic admits a row.
// The only atomics are integer OR, max and add: the result does not depend on their order.  Every index is bounded by what the host computed:
// rows by `n` (a lane past the last row evaluates nothing), columns by the plan (host/domain_audit.hpp checks every term against the widths),
// slots by the slot count, bitmap words by v < 2^16, ranks by R.
// An emulation without waves defines VGPU_DA_WAVE_PRIMS before including this file and supplies da_ballot and da_shfl itself.
#include <stdexcept>
#include <string>
#include "launch.hpp"
#include "interactions.hpp"

namespace vk {

#ifndef VGPU_DA_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from workgroup-uniform control flow only.  (slot: LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long da_ballot(bool pred, uint32_t*) { return __ballot(pred); }
// the value of `v` on lane `src` of this wave
__device__ __forceinline__ uint32_t da_shfl(uint32_t v, uint32_t src, uint32_t*) { return (uint32_t)__shfl((int)v, (int)src, 64); }
#endif

constexpr uint32_t DA_SLOT_WORDS = 4 * 66;  // per wave 66 words for the emulation's primitives

__global__ void __launch_bounds__(256) k_da_scan(const DaArgs a, unsigned long long* __restrict__ tot, uint32_t* __restrict__ bitmaps) {
    extern __shared__ uint32_t da_lds[];  // bitmap [2048], red [4][5], slot [4][66]
    uint32_t* bm = da_lds;
    uint32_t* red = da_lds + DA_BITMAP_WORDS;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t* slot = red + 20 + wave * 66u;
    const uint32_t y = blockIdx.y;
    const uint32_t kind = a.vt[4 * y], x0 = a.vt[4 * y + 1], cpos = a.vt[4 * y + 2], sl = a.vt[4 * y + 3];
    for (uint32_t k = t; k < DA_BITMAP_WORDS; k += 256u) bm[k] = 0;
    __syncthreads();
    uint32_t mn = 0xffffffffu, mx = 0, nz = 0, wd = 0, lv = 0;
    for (uint32_t tile = 0; tile < a.TPS; tile++) {
        const uint64_t base = ((uint64_t)blockIdx.x * a.TPS + tile) * DA_TILE;
        if (base >= a.n) break;  // workgroup-uniform
        const uint64_t r = base + t;
        const bool in = r < a.n;
        bool live = in;
        uint32_t v = 0;
        if (kind == 0) {
            if (in) v = vg::Fp::raw(a.main[(uint64_t)x0 * a.mstride + r]).canonical();
        } else if (in) {
            uint32_t pos = cpos;
            live = !eval_vcol(a.iw, pos, a.main, a.mstride, a.prep, a.pstride, r).is_zero();
            if (live) { pos = x0; v = eval_vcol(a.iw, pos, a.main, a.mstride, a.prep, a.pstride, r).canonical(); }
        }
        if (live) {
            mn = v < mn ? v : mn; mx = v > mx ? v : mx;
            nz += v != 0; wd += (v >> 16) != 0; lv++;
        }
        const unsigned long long mask = da_ballot(live, slot);
        const uint32_t first = mask ? (uint32_t)__builtin_ctzll(mask) : 0u;
        const uint32_t v0 = da_shfl(v, first, slot);
        const bool same = da_ballot(live && v == v0, slot) == mask;
        if (live && !(v >> 16) && (!same || lane == first)) atomicOr(&bm[v >> 5], 1u << (v & 31u));
    }
    // the wave's lanes by shuffles, the four waves through LDS
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        const uint32_t src = lane + d < 64u ? lane + d : lane;
        const uint32_t omn = da_shfl(mn, src, slot), omx = da_shfl(mx, src, slot), onz = da_shfl(nz, src, slot), owd = da_shfl(wd, src, slot), olv = da_shfl(lv, src, slot);
        if (lane + d < 64u) { mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; nz += onz; wd += owd; lv += olv; }
    }
    if (lane == 0) { red[wave * 5] = mn; red[wave * 5 + 1] = mx; red[wave * 5 + 2] = nz; red[wave * 5 + 3] = wd; red[wave * 5 + 4] = lv; }
    __syncthreads();
    if (t == 0) {
        for (uint32_t w = 1; w < 4; w++) {
            mn = red[w * 5] < mn ? red[w * 5] : mn; mx = red[w * 5 + 1] > mx ? red[w * 5 + 1] : mx;
            nz += red[w * 5 + 2]; wd += red[w * 5 + 3]; lv += red[w * 5 + 4];
        }
        if (lv) {
            unsigned long long* o = tot + (uint64_t)sl * DA_TOT;
            atomicMax(&o[0], (unsigned long long)(~mn));
            atomicMax(&o[1], (unsigned long long)mx);
            if (nz) atomicAdd(&o[2], (unsigned long long)nz);
            if (wd) atomicAdd(&o[3], (unsigned long long)wd);
            atomicAdd(&o[4], (unsigned long long)lv);
        }
    }
    uint32_t* out = bitmaps + (uint64_t)sl * DA_BITMAP_WORDS;
    for (uint32_t k = t; k < DA_BITMAP_WORDS; k += 256u)
        if (bm[k]) atomicOr(&out[k], bm[k]);
}

__global__ void __launch_bounds__(256) k_da_classify(const unsigned long long* __restrict__ tot, const uint32_t* __restrict__ bitmaps, uint32_t* __restrict__ cls, uint32_t max_bits) {
    extern __shared__ uint32_t da_lds[];  // [256] partial popcounts, [16] their sums
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t* b = bitmaps + (uint64_t)s * DA_BITMAP_WORDS;
    uint32_t pc = 0;
    for (uint32_t k = t; k < DA_BITMAP_WORDS; k += 256u) pc += (uint32_t)__builtin_popcount(b[k]);
    da_lds[t] = pc;
    __syncthreads();
    if (t < 16) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i < 16; i++) sum += da_lds[t * 16 + i];
        da_lds[256 + t] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    uint32_t distinct = 0;
    for (uint32_t i = 0; i < 16; i++) distinct += da_lds[256 + i];
    const unsigned long long* o = tot + (uint64_t)s * DA_TOT;
    uint32_t* c = cls + (uint64_t)s * DA_CLS;
    const bool any = o[4] != 0;
    const uint32_t mn = any ? ~(uint32_t)o[0] : 0u, mx = any ? (uint32_t)o[1] : 0u;
    const uint32_t cl = mn == mx ? 0u : mx <= 1u ? 1u : mx < 256u ? 2u : mx < 65536u ? 3u : 4u;
    c[0] = distinct; c[1] = cl;
    c[2] = (any && !o[3] && distinct == mx - mn + 1u) ? 1u : 0u;
    c[3] = mx ? 32u - (uint32_t)__builtin_clz(mx) : 0u;
    c[4] = ((cl == 2u || cl == 3u) && mx < (1u << max_bits)) ? 1u : 0u;
    c[5] = mn; c[6] = mx; c[7] = 0;
}

__global__ void __launch_bounds__(256) k_da_guard(const DaArgs a, uint32_t mode, const uint32_t* __restrict__ cls, unsigned long long* __restrict__ gtot, uint32_t* __restrict__ table,
                                                  const uint32_t* __restrict__ prefix, uint32_t c_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t da_lds[];  // gt [GW], cnt [5 W + A], wcnt [4], slot [4][66] (DA_SLOT_WORDS) behind them
    const uint32_t W = a.width, NCNT = 5u * W + a.A;
    uint32_t* tb = da_lds;
    uint32_t* cnt = tb + a.GW;
    uint32_t* wcnt = cnt + NCNT;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t* slot = wcnt + 4 + wave * 66u;
    for (uint32_t k = t; k < a.GW; k += 256u) tb[k] = a.gt[k];
    for (uint32_t k = t; k < NCNT; k += 256u) cnt[k] = 0;
    __syncthreads();
    const uint32_t* item_at = tb + 2;
    const uint32_t* items = tb + 2 + W + 1;
    const uint64_t r = (uint64_t)blockIdx.x * DA_TILE + t;
    const bool in = r < a.n;
    for (uint32_t c = 0; c < W; c++) {  // every test on c below is workgroup-uniform
        const uint32_t i0 = item_at[c], i1 = item_at[c + 1];
        const bool narrow = cls[(uint64_t)(a.slot0 + c) * DA_CLS + 4] != 0;
        if (i0 == i1 && !narrow) continue;
        if (mode == MA_LIST && (c >= c_cut || !narrow || !table[(uint64_t)c * a.NB + blockIdx.x] || prefix[(uint64_t)c * a.NB + blockIdx.x] >= R)) continue;
        uint32_t fm = 0;
        for (uint32_t i = i0; i < i1; i++) {
            uint32_t pos = items[3 * i];
            const uint32_t kind = items[3 * i + 1], app = items[3 * i + 2];
            const bool live = in && !eval_vcol(a.iw, pos, a.main, a.mstride, a.prep, a.pstride, r).is_zero();
            fm |= live ? 1u << kind : 0u;
            if (mode == MA_COUNT && app != 0xffffffffu) {
                const unsigned long long m = da_ballot(live, slot);
                if (lane == 0 && m) atomicAdd(&cnt[5u * W + app], (uint32_t)__builtin_popcountll(m));
            }
        }
        const uint32_t cell = in ? a.main[(uint64_t)c * a.mstride + r] : 0u;  // Montgomery: zero iff the canonical value is
        const bool ung = in && !(fm & 1u) && cell != 0;
        if (mode == MA_COUNT) {
            for (uint32_t k = 0; k < 4; k++) {
                const unsigned long long m = da_ballot((fm >> k) & 1u, slot);
                if (lane == 0 && m) atomicAdd(&cnt[5u * c + k], (uint32_t)__builtin_popcountll(m));
            }
            const unsigned long long m = da_ballot(ung, slot);
            if (lane == 0 && m) atomicAdd(&cnt[5u * c + 4], (uint32_t)__builtin_popcountll(m));
        } else {
            const unsigned long long m = da_ballot(ung, slot);
            if (lane == 0) wcnt[wave] = (uint32_t)__builtin_popcountll(m);
            __syncthreads();
            uint32_t rank = prefix[(uint64_t)c * a.NB + blockIdx.x];
            for (uint32_t w = 0; w < wave; w++) rank += wcnt[w];
            rank += (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (ung && rank < R) {
                uint32_t* o = rows + ((uint64_t)c * R + rank) * 2;
                o[0] = (uint32_t)r; o[1] = vg::Fp::raw(cell).canonical();
            }
            __syncthreads();
        }
    }
    if (mode != MA_COUNT) return;
    __syncthreads();
    for (uint32_t k = t; k < NCNT; k += 256u) {
        if (!cnt[k]) continue;
        atomicAdd(&gtot[k], (unsigned long long)cnt[k]);
        if (k < 5u * W && k % 5u == 4u && cls[(uint64_t)(a.slot0 + k / 5u) * DA_CLS + 4]) table[(uint64_t)(k / 5u) * a.NB + blockIdx.x] = cnt[k];
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
void da_shape(DaArgs& a, uint32_t max_slices) {
    if (a.n == 0 || (a.n & (a.n - 1)) || max_slices == 0) throw std::logic_error("domain_audit: heights are powers of two");
    const uint64_t tiles = (a.n + DA_TILE - 1) / DA_TILE;
    const uint64_t s = tiles < max_slices ? tiles : max_slices;
    a.TPS = (uint32_t)((tiles + s - 1) / s);
    a.S = (uint32_t)((tiles + a.TPS - 1) / a.TPS);
    a.NB = (uint32_t)tiles;
}

RaArgs da_scan_args(const DaArgs& a) {
    RaArgs r{};
    r.n = a.NB; r.width = 1; r.K = 0; r.native_chip = MA_BUS_ONLY;
    r.NW = 1; r.RPW = 1; r.T = 1; r.NB = a.NB;  // one table word per workgroup of the guard pass
    return r;
}

static void da_check(const DaArgs& a) {
    const uint64_t tiles = (a.n + DA_TILE - 1) / DA_TILE;
    if (a.n == 0 || (a.n & (a.n - 1)) || !a.TPS || !a.S || a.S > 65535u || (uint64_t)a.TPS * a.S < tiles || a.NB != tiles) throw std::logic_error("domain_audit: inconsistent launch shape");
}

void launch_da_scan(hipStream_t st, const DaArgs& a, unsigned long long* tot, uint32_t* bitmaps) {
    da_check(a);
    if (!a.NV) return;
    if (a.NV > 65535u) throw std::logic_error("domain_audit: at most 65535 virtual columns per chip");
    ProfScope ps("k_da_scan", st, 4.0 * (double)a.n * a.NV, (double)a.n * a.NV);
    VK_LAUNCH(k_da_scan, dim3(a.S, a.NV), dim3(256), (DA_BITMAP_WORDS + 20 + DA_SLOT_WORDS) * 4, st, a, tot, bitmaps);
}

void launch_da_classify(hipStream_t st, const unsigned long long* tot, const uint32_t* bitmaps, uint32_t* cls, uint32_t n_slots, uint32_t max_bits) {
    if (!n_slots) return;
    if (max_bits == 0 || max_bits > 16) throw std::logic_error("domain_audit: max_bits is 1 to 16");
    ProfScope ps("k_da_classify", st, 4.0 * DA_BITMAP_WORDS * (double)n_slots);
    VK_LAUNCH(k_da_classify, dim3(n_slots), dim3(256), (256 + 16) * 4, st, tot, bitmaps, cls, max_bits);
}

void launch_da_guard(hipStream_t st, const DaArgs& a, uint32_t mode, const uint32_t* cls, unsigned long long* gtot, uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R,
                     uint32_t* rows) {
    da_check(a);
    if (!a.width) return;
    if (da_guard_lds_words(a) + DA_SLOT_WORDS > DA_GUARD_LDS_WORDS) throw std::logic_error("domain_audit: the guard table does not fit the LDS");
    if (mode == MA_LIST && (!c_cut || c_cut > a.width || !R)) throw std::logic_error("domain_audit: nothing to list");
    ProfScope ps(mode == MA_COUNT ? "k_da_guard" : "k_da_list", st, 4.0 * (double)a.n * a.width);
    VK_LAUNCH(k_da_guard, dim3(a.NB), dim3(256), (size_t)(da_guard_lds_words(a) + DA_SLOT_WORDS) * 4, st, a, mode, cls, gtot, table, prefix, c_cut, R, rows);
}

}  // namespace vk
