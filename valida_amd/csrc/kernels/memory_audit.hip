// Memory audit on the device (host/memory_audit.hpp states the contract): the receives of one bus replayed as a memory.
//
//   keys      thread per row of a chip, one descriptor walk per receive as k_ba_records does it (kernels/bus_records.hpp, so the compiled and
//             the interpreting machine give the same words): key = addr << 32 | clk << 1 | !static of a live slot, ~0 of a dead one, id = slot.
//             Per workgroup: live slots, the OR of the live keys and of their complements (the bits in which live keys differ), and the layout
//             descents, the next row's key read from an LDS tile with one halo row.
//   sort      launch_ba_sort (kernels/bus_audit.hip), unchanged, over the key bytes in which some live key differs; dead slots sink to the end.
//   gather    order position -> a packed record (addr, clk, flags, v0..v3) in arrays of their own: the later passes read coalesced.  It also
//             writes mark[i] = i + 1 if record i is a write or the first of its address, else 0.
//   scan      inclusive max-scan of the marks inside blocks of MM_SCAN_BLOCK (per thread, over wave shuffles, across waves in LDS), then an
//             exclusive max-scan of the block maxima by one workgroup.  Every first record marks: no maximum crosses an address, and a first
//             record that is a read stands for "nothing written".
//   judge     per position the last write, the expected value, the kind and reason; counts by ballots, then LDS, then one atomic per counter
//             and workgroup; the findings of a workgroup go to a table, count -> scan -> list: no atomic admits a listed record.
// The only atomics are integer add, or and max: every word is the same run after run.  Every index is bounded by what the host computed (slot
// counts, descriptor offsets checked in bus_audit_plan, n_live read back from the keys pass).  An emulation without waves defines
// VGPU_MM_WAVE_PRIMS before including this file and supplies mm_ballot and mm_shfl_up itself (tests/emu/memory_audit_emu.cpp).
#include "bus_records.hpp"

namespace vk {

#ifndef VGPU_MM_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from workgroup-uniform control flow only.  (slot: LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long mm_ballot(bool pred, uint32_t*) { return __ballot(pred); }
// the value of `v` on lane (own - delta) of this wave; the own value on the first `delta` lanes
__device__ __forceinline__ uint32_t mm_shfl_up(uint32_t v, uint32_t delta, uint32_t*) { return (uint32_t)__shfl_up((int)v, delta, 64); }
#endif

constexpr unsigned long long MM_DEAD = ~0ull;

struct MmEntry { uint32_t chip, first_slot, R; const uint32_t* list; };
__device__ __forceinline__ MmEntry mm_entry(const uint32_t* __restrict__ mt, uint32_t e) {
    const uint32_t* w = mt + 1 + 4 * e;
    return MmEntry{w[0], w[1], w[2], mt + w[3]};
}
// the entry a slot belongs to: the last one whose first slot is <= slot
__device__ __forceinline__ uint32_t mm_entry_of(const uint32_t* __restrict__ mt, uint32_t slot) {
    const uint32_t ne = mt[0];
    uint32_t e = 0;
    while (e + 1 < ne && mt[1 + 4 * (e + 1) + 1] <= slot) e++;
    return e;
}
__device__ __forceinline__ unsigned long long mm_key(uint32_t addr, uint32_t clk, uint32_t is_static) {
    return ((unsigned long long)addr << 32) | ((unsigned long long)clk << 1) | (is_static == 1 ? 0ull : 1ull);
}
// the key of (chip, interaction m, row): count, is_read, clk, addr, is_static in the order of the descriptor's vcols
__device__ __forceinline__ unsigned long long mm_key_of(const uint32_t* __restrict__ d, const BaChip& c, uint32_t m, uint32_t row) {
    uint32_t pos = d[c.table + 4 * m];
    if (!eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical()) return MM_DEAD;
    (void)eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row);
    const uint32_t clk = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    const uint32_t addr = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    const uint32_t is_static = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    return mm_key(addr, clk, is_static);
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------
// tot (u64, zeroed): [0] live slots [1] OR of the live keys [2] OR of their complements [3] layout descents [4] max of ~(chip << 32 | row)
// over the descents (0: none)
__global__ void __launch_bounds__(256) k_mm_keys(const uint32_t* __restrict__ d, const uint32_t* __restrict__ mt, uint32_t entry, unsigned long long* __restrict__ keys,
                                                 uint32_t* __restrict__ ids, unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long s_key[MM_TILE + 1];
    __shared__ unsigned long long s_red[MM_KEY_TOT];
    __shared__ uint32_t s_slot[4 * 66];
    const MmEntry en = mm_entry(mt, entry);
    const BaChip c = ba_chip(d, en.chip);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x * MM_TILE + tid;
    uint32_t* slot = s_slot + 66 * (tid >> 6);
    if (tid < MM_KEY_TOT) s_red[tid] = 0;
    for (uint32_t k = 0; k < en.R; k++) {
        const uint32_t m = en.list[k];
        const unsigned long long key = row < c.height ? mm_key_of(d, c, m, row) : MM_DEAD;
        s_key[tid] = key;
        if (tid == 0) {  // the halo row: the first row of the next tile
            const uint32_t next = (blockIdx.x + 1) * MM_TILE;
            s_key[MM_TILE] = next < c.height ? mm_key_of(d, c, m, next) : MM_DEAD;
        }
        __syncthreads();
        const bool live = key != MM_DEAD;
        const unsigned long long below = s_key[tid + 1];
        const bool descent = live && below != MM_DEAD && key > below;
        if (row < c.height) {
            const uint32_t s = en.first_slot + row * en.R + k;
            keys[s] = key; ids[s] = s;
        }
        const unsigned long long lb = mm_ballot(live, slot), db = mm_ballot(descent, slot);
        if (lane == 0 && lb) atomicAdd(&s_red[0], (unsigned long long)__popcll(lb));
        if (lane == 0 && db) atomicAdd(&s_red[3], (unsigned long long)__popcll(db));
        if (live) { atomicOr(&s_red[1], key); atomicOr(&s_red[2], ~key); }
        if (descent) atomicMax(&s_red[4], ~(((unsigned long long)en.chip << 32) | row));
        __syncthreads();
    }
    __syncthreads();
    if (tid < MM_KEY_TOT && s_red[tid]) {
        if (tid == 0 || tid == 3) atomicAdd(&tot[tid], s_red[tid]);
        else if (tid == 4) atomicMax(&tot[tid], s_red[tid]);
        else atomicOr(&tot[tid], s_red[tid]);
    }
}

// ---- gather -------------------------------------------------------------------------------------------------------------------------------
// rec: [MM_REC][n] u32 = addr, clk, flags, v0..v3; flags: bit 0 READ, bit 1 STATIC, bit 2 the first record of its address, bits 8..12 the
// malformed reason.  mark[i] = i + 1 for a write or a first record, else 0.
__global__ void __launch_bounds__(256) k_mm_gather(const uint32_t* __restrict__ d, const uint32_t* __restrict__ mt, const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ ids, uint64_t n_live, uint64_t n, uint32_t* __restrict__ rec, uint32_t* __restrict__ mark) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_live) return;
    const uint32_t id = ids[i];
    const MmEntry en = mm_entry(mt, mm_entry_of(mt, id));
    const BaChip c = ba_chip(d, en.chip);
    const uint32_t off = id - en.first_slot, row = off / en.R, m = en.list[off % en.R];
    uint32_t pos = d[c.table + 4 * m];
    uint32_t f[1 + MM_NFIELDS];  // count, is_read, clk, addr, is_static, v0..v3
    for (uint32_t j = 0; j < 1 + MM_NFIELDS; j++) f[j] = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    const bool read = f[1] == 1, is_static = f[4] == 1;
    uint32_t reason = 0;
    if (f[0] != 1) reason |= 1u;
    if (f[1] > 1) reason |= 2u;
    if (f[4] > 1) reason |= 4u;
    if (is_static && (read || f[2] != 0)) reason |= 8u;
    if (f[5] >= 256 || f[6] >= 256 || f[7] >= 256 || f[8] >= 256) reason |= 16u;
    const bool first = i == 0 || (uint32_t)(keys[i - 1] >> 32) != f[3];
    rec[i] = f[3]; rec[n + i] = f[2];
    rec[2 * n + i] = (read ? 1u : 0u) | (is_static ? 2u : 0u) | (first ? 4u : 0u) | (reason << 8);
    for (uint32_t j = 0; j < 4; j++) rec[(3 + j) * n + i] = f[5 + j];
    mark[i] = (!read || first) ? (uint32_t)i + 1u : 0u;
}

// ---- the max-scan of the marks --------------------------------------------------------------------------------------------------------------
// in place: the inclusive maximum inside blocks of MM_SCAN_BLOCK elements; block maxima to block_max
__global__ void __launch_bounds__(256) k_mm_scan_local(uint32_t* __restrict__ a, uint64_t n, uint32_t* __restrict__ block_max) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_slot[4 * 66];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* slot = s_slot + 66 * wave;
    const uint64_t base = (uint64_t)blockIdx.x * MM_SCAN_BLOCK + (uint64_t)tid * MM_SCAN_ITEMS;
    uint32_t v[MM_SCAN_ITEMS], run = 0;
    for (uint32_t u = 0; u < MM_SCAN_ITEMS; u++) { const uint32_t x = base + u < n ? a[base + u] : 0u; run = x > run ? x : run; v[u] = run; }
    uint32_t incl = run;  // the inclusive maximum over the lanes of the wave up to this one
    for (uint32_t delta = 1; delta < 64; delta <<= 1) {
        const uint32_t o = mm_shfl_up(incl, delta, slot);
        if (lane >= delta && o > incl) incl = o;
    }
    if (lane == 63) s_wave[wave] = incl;
    const uint32_t excl_lane = mm_shfl_up(incl, 1, slot);
    __syncthreads();
    uint32_t before = lane ? excl_lane : 0u;
    for (uint32_t w = 0; w < wave; w++) before = s_wave[w] > before ? s_wave[w] : before;
    for (uint32_t u = 0; u < MM_SCAN_ITEMS; u++)
        if (base + u < n) a[base + u] = v[u] > before ? v[u] : before;
    if (tid == 255) block_max[blockIdx.x] = incl > before ? incl : before;
}
// in-place EXCLUSIVE scan of `total` words by one workgroup (a contiguous chunk per thread): the maximum (is_max) or the sum
__global__ void __launch_bounds__(256) k_mm_scan_blocks(uint32_t* __restrict__ a, uint64_t total, int is_max) {
    __shared__ uint32_t s[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t chunk = (total + 255) / 256, lo = (uint64_t)tid * chunk < total ? (uint64_t)tid * chunk : total, hi = lo + chunk < total ? lo + chunk : total;
    uint32_t acc = 0;
    for (uint64_t i = lo; i < hi; i++) acc = is_max ? (a[i] > acc ? a[i] : acc) : acc + a[i];
    s[tid] = acc;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        uint32_t t = s[tid];
        if (tid >= off) t = is_max ? (s[tid - off] > t ? s[tid - off] : t) : t + s[tid - off];
        __syncthreads();
        s[tid] = t;
        __syncthreads();
    }
    uint32_t run = tid ? s[tid - 1] : 0u;
    for (uint64_t i = lo; i < hi; i++) { const uint32_t x = a[i]; a[i] = run; run = is_max ? (x > run ? x : run) : run + x; }
}

// ---- judge --------------------------------------------------------------------------------------------------------------------------------
// cnt (u64, zeroed): [0] reads [1] writes [2] statics [3] addresses [4] uninit zero reads [5] same-cycle pairs [6 .. 9] findings of kind 1 .. 4
// [10] dummy reads clk [11] dummy reads addr [12] max clk [13] max clk gap [14] min addr [15] max addr.  mode MM_COUNT: the counters and
// table[workgroup] = its findings; MM_LIST: prefix[workgroup] = the findings before it, the first max_findings go to out [MM_OUT] words each:
// kind, reason, slot, addr, clk, value[4], expected[4], the last write's slot or ~0, position, 0.
__global__ void __launch_bounds__(256) k_mm_judge(int mode, const uint32_t* __restrict__ rec, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ incl,
                                                  const uint32_t* __restrict__ block_before, uint64_t n_live, uint64_t n, unsigned long long* __restrict__ cnt,
                                                  uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix, uint32_t max_findings, uint32_t* __restrict__ out) {
    __shared__ unsigned long long s_cnt[MM_JUDGE_TOT];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_slot[4 * 66];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* slot = s_slot + 66 * wave;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + tid;
    const bool in = i < n_live;
    if (tid < MM_JUDGE_TOT) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t addr = 0, clk = 0, flags = 0, v[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0}, w_at = 0xffffffffu, kind = 0;
    bool c_uz = false, c_pair = false;
    unsigned long long d_clk = 0, d_addr = 0;
    uint32_t gap = 0;
    if (in) {
        addr = rec[i]; clk = rec[n + i]; flags = rec[2 * n + i];
        for (uint32_t j = 0; j < 4; j++) v[j] = rec[(3 + j) * n + i];
        const bool read = flags & 1u, is_static = flags & 2u, first = flags & 4u;
        if (!first) {
            const uint32_t local = i % MM_SCAN_BLOCK ? incl[i - 1] : 0u, far = block_before[i / MM_SCAN_BLOCK];
            const uint32_t mx = local > far ? local : far;  // >= 1 and <= i: the first record of this address marks
            const uint32_t j = mx - 1u;
            if (mx && j < i && !(rec[2 * n + j] & 1u)) {
                w_at = j;
                for (uint32_t k = 0; k < 4; k++) e[k] = rec[(3 + k) * n + j];
            }
            const uint32_t pclk = rec[n + i - 1], pflags = rec[2 * n + i - 1];
            gap = clk - pclk;
            if (gap > n_live) d_clk = gap / n_live;
            c_pair = pclk == clk && !is_static && !(pflags & 2u) && (!read || !(pflags & 1u));
            if (is_static && (pflags & 2u)) kind = 2;
        } else if (i) {
            const uint32_t diff = addr - rec[i - 1];
            if (diff > n_live) d_addr = diff / n_live;
        }
        const bool has = w_at != 0xffffffffu, nonzero = (v[0] | v[1] | v[2] | v[3]) != 0;
        const bool differs = has && (v[0] != e[0] || v[1] != e[1] || v[2] != e[2] || v[3] != e[3]);
        c_uz = read && !has && !nonzero;
        if (flags >> 8) kind = 1;
        else if (kind == 2) kind = 2;
        else if (read && differs) kind = 3;
        else if (read && !has && nonzero) kind = 4;
    }
    if (mode == MM_COUNT) {
        const bool preds[10] = {in && (flags & 1u), in && !(flags & 1u), in && (flags & 2u), in && (flags & 4u), c_uz, c_pair, kind == 1, kind == 2, kind == 3, kind == 4};
        for (uint32_t k = 0; k < 10; k++) {
            const unsigned long long b = mm_ballot(preds[k], slot);
            if (lane == 0 && b) atomicAdd(&s_cnt[k], (unsigned long long)__popcll(b));
        }
        if (d_clk) atomicAdd(&s_cnt[10], d_clk);
        if (d_addr) atomicAdd(&s_cnt[11], d_addr);
        if (in && clk) atomicMax(&s_cnt[12], (unsigned long long)clk);
        if (gap) atomicMax(&s_cnt[13], (unsigned long long)gap);
        if (in && i == 0) s_cnt[14] = addr;
        if (in && i + 1 == n_live) s_cnt[15] = addr;
        __syncthreads();
        if (tid < MM_JUDGE_TOT && s_cnt[tid]) {
            if (tid == 12 || tid == 13) atomicMax(&cnt[tid], s_cnt[tid]);
            else atomicAdd(&cnt[tid], s_cnt[tid]);  // [14] and [15] have one writer each in the whole grid
        }
        if (tid == 0) table[blockIdx.x] = (uint32_t)(s_cnt[6] + s_cnt[7] + s_cnt[8] + s_cnt[9]);
    } else {
        const unsigned long long b = mm_ballot(kind != 0, slot);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t at = prefix[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; w++) at += s_wave[w];
        if (kind && at < max_findings) {
            uint32_t* o = out + (uint64_t)at * MM_OUT;
            o[0] = kind; o[1] = flags >> 8; o[2] = ids[i]; o[3] = addr; o[4] = clk;
            for (uint32_t k = 0; k < 4; k++) { o[5 + k] = v[k]; o[9 + k] = e[k]; }
            o[13] = w_at == 0xffffffffu ? 0xffffffffu : ids[w_at]; o[14] = (uint32_t)i; o[15] = 0;
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
static unsigned mm_blocks(uint64_t n, uint64_t per = 256) { return (unsigned)((n + per - 1) / per); }

size_t memory_audit_scan_blocks(uint64_t n) { return (size_t)((n + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK); }

void launch_mm_keys(hipStream_t st, const uint32_t* desc, const uint32_t* mt, uint32_t entry, uint64_t height, uint32_t R, unsigned long long* keys, uint32_t* ids,
                    unsigned long long* tot) {
    if (!R || !height) return;
    ProfScope ps("k_mm_keys", st, 20.0 * height * R + 12.0 * height * R);
    VK_LAUNCH(k_mm_keys, dim3(mm_blocks(height, MM_TILE)), dim3(256), 0, st, desc, mt, entry, keys, ids, tot);
}
void launch_mm_gather(hipStream_t st, const uint32_t* desc, const uint32_t* mt, const unsigned long long* keys, const uint32_t* ids, uint64_t n_live, uint64_t n, uint32_t* rec,
                      uint32_t* mark) {
    if (!n_live) return;
    ProfScope ps("k_mm_gather", st, (12.0 + 36.0 + 4.0 * (MM_REC + 1)) * n_live);
    VK_LAUNCH(k_mm_gather, dim3(mm_blocks(n_live)), dim3(256), 0, st, desc, mt, keys, ids, n_live, n, rec, mark);
}
// mark [n_live] -> in place the inclusive maxima inside scan blocks; block_before [memory_audit_scan_blocks(n_live)]: the maximum before each block
void launch_mm_scan(hipStream_t st, uint32_t* mark, uint64_t n_live, uint32_t* block_before) {
    if (!n_live) return;
    ProfScope ps("k_mm_scan", st, 8.0 * n_live);
    const unsigned nb = mm_blocks(n_live, MM_SCAN_BLOCK);
    VK_LAUNCH(k_mm_scan_local, dim3(nb), dim3(256), 0, st, mark, n_live, block_before);
    VK_LAUNCH(k_mm_scan_blocks, dim3(1), dim3(256), 0, st, block_before, (uint64_t)nb, 1);
}
void launch_mm_scan_words(hipStream_t st, uint32_t* a, uint64_t total, int is_max) {
    if (!total) return;
    VK_LAUNCH(k_mm_scan_blocks, dim3(1), dim3(256), 0, st, a, total, is_max);
}
void launch_mm_judge(hipStream_t st, uint32_t mode, const uint32_t* rec, const uint32_t* ids, const uint32_t* incl, const uint32_t* block_before, uint64_t n_live, uint64_t n,
                     unsigned long long* cnt, uint32_t* table, uint32_t max_findings, uint32_t* out) {
    if (!n_live) return;
    const unsigned nb = mm_blocks(n_live);
    if (mode == MM_COUNT) {
        ProfScope ps("k_mm_judge", st, 4.0 * (MM_REC + 2) * n_live);
        VK_LAUNCH(k_mm_judge, dim3(nb), dim3(256), 0, st, (int)MM_COUNT, rec, ids, incl, block_before, n_live, n, cnt, table, (const uint32_t*)nullptr, 0u, (uint32_t*)nullptr);
    } else {
        ProfScope ps("k_mm_list", st, 4.0 * (MM_REC + 2) * n_live);
        VK_LAUNCH(k_mm_scan_blocks, dim3(1), dim3(256), 0, st, table, (uint64_t)nb, 0);  // the table becomes its own exclusive prefix
        VK_LAUNCH(k_mm_judge, dim3(nb), dim3(256), 0, st, (int)MM_LIST, rec, ids, incl, block_before, n_live, n, (unsigned long long*)nullptr, (uint32_t*)nullptr,
                  (const uint32_t*)table, max_findings, out);
    }
}

}  // namespace vk
