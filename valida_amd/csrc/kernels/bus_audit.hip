// Bus audit on the device (host/bus_audit.hpp states the contract and the descriptor layout): which LogUp tuples of a witness are unbalanced,
// exactly — the challenge-free form of check_cumulative_sums (basic/src/lib.rs:373-375) over Chip::all_interactions (machine/src/chip.rs:40-63).
//
//   records   thread per row and chip: every interaction's count (VirtualPairCol, kernels/interactions.hpp); a live record gets a 64-bit key =
//             a fixed mix of (bus, canonical fields) in which a zero field contributes nothing (zero-padding is invisible, as it is to the
//             permutation argument, machine/src/chip.rs:121-208), a dead one the key ~0.  Slot = record id, so ids ascend in the input.
//   sort      stable 8-bit LSD radix sort of (u64 key, u32 id): the structure of tracegen.hip's k_rs_* over 64-bit keys; dead slots sink to the end.
//   groups    heads (key differs from the predecessor's), a scan numbers the groups, one pass records each group's head position.
//   reduce    per group send / receive sums (u64 of canonical counts: order-independent) and record counts.  A workgroup first reduces its 256
//             consecutive records in LDS (they span consecutive groups), then issues one global atomic per group it touches: the range bus's
//             groups of 10^4..10^6 records cost one atomic per 256 records, not one per record.  Every record's recomputed (bus, tuple) is
//             compared with its group head's: a mismatch is a key collision.
//   exact     only after a collision: the same pipeline with the records sorted by their FULL padded tuples (two words per radix sort, least
//             significant first), heads by full comparison with the predecessor.  Correct, not fast; with 64 key bits it does not run.
//   report    unbalanced groups are compacted, sorted by first record id, the first max_tuples get their tuple recomputed and their first records
//             gathered.  Only that crosses PCIe.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (slot counts, descriptor offsets, column indices
// checked against the trace widths in bus_audit_plan).  No wave intrinsic outside the sort's scatter kernel (tests/emu/bus_audit_emu.cpp).
#include "bus_records.hpp"

namespace vk {

constexpr unsigned long long BA_DEAD = ~0ull;

__host__ __device__ __forceinline__ unsigned long long ba_fmix(unsigned long long x) {  // 0 -> 0
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
__host__ __device__ __forceinline__ unsigned long long ba_key_seed(uint32_t bus_slot) { return ba_fmix(0x243F6A8885A308D3ULL + bus_slot); }
// field j's share of the key; a zero field adds nothing
__host__ __device__ __forceinline__ unsigned long long ba_key_term(uint32_t j, uint32_t canonical) {
    const unsigned long long cj = ba_fmix((unsigned long long)(j + 1) * 0x9E3779B97F4A7C15ULL) | 1ull;
    return ba_fmix((unsigned long long)canonical * cj);
}
__host__ __device__ __forceinline__ unsigned long long ba_key_finish(unsigned long long h, uint32_t hash_bits) {
    h = ba_fmix(h);
    if (hash_bits < 64) h &= (1ull << hash_bits) - 1ull;
    return h == BA_DEAD ? BA_DEAD - 1ull : h;
}

// ---- records ---------------------------------------------------------------------------------------------------------------------------
// live_out: live records per interaction of the chip (the first 256 interactions are counted in LDS, one global atomic per block each)
__global__ void __launch_bounds__(256) k_ba_records(const uint32_t* __restrict__ d, uint32_t chip, uint32_t hash_bits, unsigned long long* __restrict__ keys,
                                                    uint32_t* __restrict__ ids, uint32_t* __restrict__ cnt, uint32_t* __restrict__ live_out) {
    __shared__ uint32_t s_live[256];
    const BaChip c = ba_chip(d, chip);
    s_live[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row < c.height) {
        for (uint32_t m = 0; m < c.M; m++) {
            const uint32_t* ie = d + c.table + 4 * m;
            uint32_t pos = ie[0];
            const uint32_t count = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
            unsigned long long key = BA_DEAD;
            if (count) {
                unsigned long long h = ba_key_seed(ie[2]);
                const uint32_t nf = ie[3];
                for (uint32_t j = 0; j < nf; j++) h += ba_key_term(j, eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical());
                key = ba_key_finish(h, hash_bits);
                if (m < 256) atomicAdd(&s_live[m], 1u);
                else atomicAdd(&live_out[m], 1u);
            }
            const uint32_t slot = c.first_id + row * c.M + m;
            keys[slot] = key; ids[slot] = slot; cnt[slot] = count;
        }
    }
    __syncthreads();
    if (threadIdx.x < c.M && s_live[threadIdx.x]) atomicAdd(&live_out[threadIdx.x], s_live[threadIdx.x]);
}

__global__ void __launch_bounds__(256) k_ba_iota(uint32_t* __restrict__ ids, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ids[i] = (uint32_t)i;
}

// exact path: key = words (2 chunk, 2 chunk + 1) of [bus slot, field 0, field 1, ...] (zero beyond the interaction's fields); dead slots keep ~0
__global__ void __launch_bounds__(256) k_ba_rekey(const uint32_t* __restrict__ d, uint32_t chunk, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cnt,
                                                  unsigned long long* __restrict__ keys, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    unsigned long long key = BA_DEAD;
    if (cnt[id]) {
        BaRef r = ba_ref(d, id);
        uint32_t w[2] = {0, 0};
        for (uint32_t k = 0; k <= 2 * chunk + 1; k++) {  // word 0: the bus slot; word k >= 1: field k - 1
            const uint32_t v = k == 0 ? r.bus_slot : (k - 1 < r.n_fields ? ba_next_field(d, r) : 0u);
            if (k >= 2 * chunk) w[k - 2 * chunk] = v;
        }
        key = ((unsigned long long)w[0] << 32) | w[1];
    }
    keys[i] = key;
}

// ---- stable LSD radix sort of (u64 key, u32 value) pairs, 8 bits a pass (tracegen.hip's k_rs_* over 64-bit keys) ------------------------
constexpr int BA_RS_ITEMS = 16, BA_RS_BLOCK = BA_RS_ITEMS * 256;

__global__ void __launch_bounds__(256) k_ba_sort_count(const unsigned long long* __restrict__ keys, uint64_t n, int shift, uint32_t* __restrict__ counts, uint32_t n_blocks) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * BA_RS_BLOCK;
    for (int u = 0; u < BA_RS_ITEMS; u++) {
        const uint64_t i = base + u * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// in-place exclusive scan of `total` counters by one 1024-thread block (contiguous chunk per thread)
__global__ void __launch_bounds__(1024) k_ba_scan_table(uint32_t* __restrict__ counts, uint64_t total) {
    __shared__ uint32_t sums[1024];
    const uint64_t chunk = (total + 1023) / 1024, lo = (uint64_t)threadIdx.x * chunk < total ? (uint64_t)threadIdx.x * chunk : total, hi = lo + chunk < total ? lo + chunk : total;
    uint32_t s = 0;
    for (uint64_t i = lo; i < hi; i++) s += counts[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        uint32_t t = sums[threadIdx.x];
        if ((int)threadIdx.x >= off) t += sums[threadIdx.x - off];
        __syncthreads();
        sums[threadIdx.x] = t;
        __syncthreads();
    }
    uint32_t run = sums[threadIdx.x] - s;
    for (uint64_t i = lo; i < hi; i++) { const uint32_t c = counts[i]; counts[i] = run; run += c; }
}

__global__ void __launch_bounds__(256) k_ba_sort_scatter(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t n, int shift,
                                                         const uint32_t* __restrict__ counts, uint32_t n_blocks, unsigned long long* __restrict__ keys_out,
                                                         uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t base[256], wcount[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    base[threadIdx.x] = counts[(uint64_t)threadIdx.x * n_blocks + blockIdx.x];
    const uint64_t first = (uint64_t)blockIdx.x * BA_RS_BLOCK;
    for (int u = 0; u < BA_RS_ITEMS; u++) {
        for (int w = 0; w < 4; w++) wcount[w][threadIdx.x] = 0;
        __syncthreads();
        const uint64_t i = first + u * 256 + threadIdx.x;
        const bool live = i < n;
        const unsigned long long key = live ? keys[i] : 0ull;
        const uint32_t val = live ? vals[i] : 0u, dg = (uint32_t)(key >> shift) & 255u;
        unsigned long long peers = __ballot(live);  // lanes of this wave holding a live pair with the same digit
        for (int b = 0; b < 8; b++) { const unsigned long long bal = __ballot((dg >> b) & 1u); peers &= ((dg >> b) & 1u) ? bal : ~bal; }
        const uint32_t rank_in_wave = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (live && rank_in_wave == 0) wcount[wave][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (live) {
            uint32_t before = 0;
            for (int w = 0; w < 4; w++) if (w < wave) before += wcount[w][dg];
            const uint32_t pos = base[dg] + before + rank_in_wave;  // < n: the table's prefix sums count exactly the n pairs
            keys_out[pos] = key;
            vals_out[pos] = val;
        }
        __syncthreads();
        base[threadIdx.x] += wcount[0][threadIdx.x] + wcount[1][threadIdx.x] + wcount[2][threadIdx.x] + wcount[3][threadIdx.x];
        __syncthreads();
    }
}

// ---- groups -----------------------------------------------------------------------------------------------------------------------------
// counters: [0] live records [1] groups [2] records whose tuple differs from their group head's [3] unbalanced groups [4] append cursor
//           [8 + b] unbalanced groups of bus slot b
__global__ void __launch_bounds__(256) k_ba_heads(const uint32_t* __restrict__ d, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ ids, uint64_t n, int exact,
                                                  uint32_t* __restrict__ flag, uint32_t* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const bool live = k != BA_DEAD;
    uint32_t f = 0;
    if (live) {
        if (i == 0) f = 1;
        else if (!exact) f = keys[i - 1] != k;
        else f = !ba_same_tuple(d, ids[i], ids[i - 1]);  // the predecessor is live: dead slots sort behind every live one
        if (i + 1 == n || keys[i + 1] == BA_DEAD) counters[0] = (uint32_t)(i + 1);
    }
    flag[i] = f;
}

constexpr int BA_SCAN_ITEMS = 8, BA_SCAN_BLOCK = BA_SCAN_ITEMS * 256;
// inclusive scan inside blocks of BA_SCAN_BLOCK elements; block totals to block_sums
__global__ void __launch_bounds__(256) k_ba_scan_local(uint32_t* __restrict__ a, uint64_t n, uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t s[256];
    const uint64_t base = (uint64_t)blockIdx.x * BA_SCAN_BLOCK + (uint64_t)threadIdx.x * BA_SCAN_ITEMS;
    uint32_t v[BA_SCAN_ITEMS], sum = 0;
    for (int u = 0; u < BA_SCAN_ITEMS; u++) { sum += base + u < n ? a[base + u] : 0u; v[u] = sum; }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t t = s[threadIdx.x];
        if ((int)threadIdx.x >= off) t += s[threadIdx.x - off];
        __syncthreads();
        s[threadIdx.x] = t;
        __syncthreads();
    }
    const uint32_t before = s[threadIdx.x] - sum;
    for (int u = 0; u < BA_SCAN_ITEMS; u++) if (base + u < n) a[base + u] = v[u] + before;
    if (threadIdx.x == 255) block_sums[blockIdx.x] = s[255];
}
__global__ void __launch_bounds__(256) k_ba_scan_add(uint32_t* __restrict__ a, uint64_t n, const uint32_t* __restrict__ block_sums) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] += block_sums[i / BA_SCAN_BLOCK];
}
// gid[i] = 1 + group number of sorted position i (inclusive scan of the head flags); head_pos[g] = position of group g's first record
__global__ void __launch_bounds__(256) k_ba_group_heads(const uint32_t* __restrict__ gid, uint32_t* __restrict__ head_pos, uint32_t* __restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t n_live = counters[0];
    if (i >= n_live) return;
    const uint32_t g = gid[i];
    if (i == 0 || gid[i - 1] != g) head_pos[g - 1] = (uint32_t)i;
    if (i + 1 == n_live) counters[1] = g;
}

// sums[2 g] / sums[2 g + 1]: send / receive sums of canonical counts; nrec[2 g] / nrec[2 g + 1]: send / receive records
__global__ void __launch_bounds__(256) k_ba_reduce(const uint32_t* __restrict__ d, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ gid,
                                                   const uint32_t* __restrict__ head_pos, int check, unsigned long long* __restrict__ sums, uint32_t* __restrict__ nrec,
                                                   uint32_t* __restrict__ counters) {
    __shared__ unsigned long long s_sum[2][256];
    __shared__ uint32_t s_n[2][256];
    const uint32_t n_live = counters[0];
    const uint64_t first = (uint64_t)blockIdx.x * 256, i = first + threadIdx.x;
    s_sum[0][threadIdx.x] = 0; s_sum[1][threadIdx.x] = 0; s_n[0][threadIdx.x] = 0; s_n[1][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t g0 = first < n_live ? gid[first] - 1 : 0u;  // the block's 256 records span groups g0 .. g0 + 255 at most
    if (i < n_live) {
        const uint32_t id = ids[i], g = gid[i] - 1, l = g - g0;
        const BaRef r = ba_ref(d, id);
        const int side = r.is_send ? 0 : 1;
        atomicAdd(&s_sum[side][l], (unsigned long long)cnt[id]);
        atomicAdd(&s_n[side][l], 1u);
        if (check) {
            const uint32_t hp = head_pos[g];
            if (hp != (uint32_t)i && !ba_same_tuple(d, id, ids[hp])) atomicAdd(&counters[2], 1u);
        }
    }
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (s_n[0][l] | s_n[1][l]) {
        const uint64_t g = (uint64_t)g0 + l;
        if (s_n[0][l]) { atomicAdd(&sums[2 * g], s_sum[0][l]); atomicAdd(&nrec[2 * g], s_n[0][l]); }
        if (s_n[1][l]) { atomicAdd(&sums[2 * g + 1], s_sum[1][l]); atomicAdd(&nrec[2 * g + 1], s_n[1][l]); }
    }
}

__device__ __forceinline__ bool ba_unbalanced(const unsigned long long* __restrict__ sums, uint64_t g) {
    return (uint32_t)(sums[2 * g] % vg::P) != (uint32_t)(sums[2 * g + 1] % vg::P);
}
// collect = 0: count the unbalanced groups (all and per bus); 1: append (first record id, group) for at most cap of them
__global__ void __launch_bounds__(256) k_ba_select(const uint32_t* __restrict__ d, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ head_pos,
                                                   const unsigned long long* __restrict__ sums, int collect, uint32_t cap, unsigned long long* __restrict__ ukeys,
                                                   uint32_t* __restrict__ uvals, uint32_t* __restrict__ counters) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= counters[1] || !ba_unbalanced(sums, g)) return;
    const uint32_t id = ids[head_pos[g]];
    if (!collect) {
        atomicAdd(&counters[3], 1u);
        atomicAdd(&counters[8 + ba_ref(d, id).bus_slot], 1u);
    } else {
        const uint32_t at = atomicAdd(&counters[4], 1u);
        if (at < cap) { ukeys[at] = id; uvals[at] = (uint32_t)g; }
    }
}

// out, per reported tuple t (stride = 8 + wmax + 2 R words): [0] bus slot [1] group size listed [2,3] send sum [4,5] receive sum [6] send records
// [7] receive records, wmax padded fields, then R x (record id, count)
__global__ void __launch_bounds__(64) k_ba_report(const uint32_t* __restrict__ d, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cnt,
                                                  const uint32_t* __restrict__ head_pos, const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ nrec,
                                                  const uint32_t* __restrict__ uvals, uint32_t n_rep, uint32_t R, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_rep) return;
    const uint32_t wmax = d[2], stride = 8 + wmax + 2 * R;
    uint32_t* o = out + (uint64_t)t * stride;
    const uint64_t g = uvals[t];
    const uint32_t hp = head_pos[g];
    BaRef r = ba_ref(d, ids[hp]);
    const uint64_t size = (uint64_t)nrec[2 * g] + nrec[2 * g + 1];
    const uint32_t listed = size < R ? (uint32_t)size : R;
    o[0] = r.bus_slot; o[1] = listed;
    o[2] = (uint32_t)sums[2 * g]; o[3] = (uint32_t)(sums[2 * g] >> 32); o[4] = (uint32_t)sums[2 * g + 1]; o[5] = (uint32_t)(sums[2 * g + 1] >> 32);
    o[6] = nrec[2 * g]; o[7] = nrec[2 * g + 1];
    for (uint32_t j = 0; j < wmax; j++) o[8 + j] = j < r.n_fields ? ba_next_field(d, r) : 0u;
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t id = k < listed ? ids[hp + k] : 0u;
        o[8 + wmax + 2 * k] = id; o[8 + wmax + 2 * k + 1] = k < listed ? cnt[id] : 0u;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
static unsigned ba_blocks(uint64_t n, uint64_t per = 256) { return (unsigned)((n + per - 1) / per); }

size_t bus_audit_sort_scratch_words(uint64_t n) { return (size_t)256 * ((n + BA_RS_BLOCK - 1) / BA_RS_BLOCK) + 4; }
size_t bus_audit_scan_scratch_words(uint64_t n) { return (size_t)((n + BA_SCAN_BLOCK - 1) / BA_SCAN_BLOCK) + 4; }

void launch_ba_records(hipStream_t st, const uint32_t* desc, uint32_t chip, uint64_t height, uint32_t width, uint32_t M, uint32_t hash_bits, unsigned long long* keys, uint32_t* ids,
                       uint32_t* cnt, uint32_t* live_out) {
    if (!M || !height) return;
    ProfScope ps("k_ba_records", st, 4.0 * height * width + 16.0 * height * M);
    VK_LAUNCH(k_ba_records, dim3(ba_blocks(height)), dim3(256), 0, st, desc, chip, hash_bits, keys, ids, cnt, live_out);
}
void launch_ba_iota(hipStream_t st, uint32_t* ids, uint64_t n) {
    if (!n) return;
    ProfScope ps("k_ba_exact_keys", st, 4.0 * n);
    VK_LAUNCH(k_ba_iota, dim3(ba_blocks(n)), dim3(256), 0, st, ids, n);
}
void launch_ba_rekey(hipStream_t st, const uint32_t* desc, uint32_t chunk, const uint32_t* ids, const uint32_t* cnt, unsigned long long* keys, uint64_t n) {
    if (!n) return;
    ProfScope ps("k_ba_exact_keys", st, 16.0 * n);
    VK_LAUNCH(k_ba_rekey, dim3(ba_blocks(n)), dim3(256), 0, st, desc, chunk, ids, cnt, keys, n);
}
// keys2 / vals2: [2 n] each, the input in half `half`; one pass per entry of shifts; returns the half that holds the result
int launch_ba_sort(hipStream_t st, unsigned long long* keys2, uint32_t* vals2, uint64_t n, uint32_t* counts, const int* shifts, int n_shifts, int half) {
    if (!n) return half;
    ProfScope ps("k_ba_sort", st, 24.0 * n * n_shifts + 8.0 * n * n_shifts);
    const uint32_t n_blocks = ba_blocks(n, BA_RS_BLOCK);
    for (int p = 0; p < n_shifts; p++, half ^= 1) {
        const unsigned long long* kin = keys2 + (uint64_t)half * n;
        const uint32_t* vin = vals2 + (uint64_t)half * n;
        VK_LAUNCH(k_ba_sort_count, dim3(n_blocks), dim3(256), 0, st, kin, n, shifts[p], counts, n_blocks);
        VK_LAUNCH(k_ba_scan_table, dim3(1), dim3(1024), 0, st, counts, (uint64_t)256 * n_blocks);
        VK_LAUNCH(k_ba_sort_scatter, dim3(n_blocks), dim3(256), 0, st, kin, vin, n, shifts[p], (const uint32_t*)counts, n_blocks, keys2 + (uint64_t)(half ^ 1) * n,
                  vals2 + (uint64_t)(half ^ 1) * n);
    }
    return half;
}
void launch_ba_groups(hipStream_t st, const uint32_t* desc, const unsigned long long* keys, const uint32_t* ids, uint64_t n, bool exact, uint32_t* gid, uint32_t* head_pos,
                      uint32_t* scan_tmp, uint32_t* counters) {
    if (!n) return;
    ProfScope ps("k_ba_groups", st, 12.0 * n + 16.0 * n);
    const unsigned nb = ba_blocks(n, BA_SCAN_BLOCK);
    VK_LAUNCH(k_ba_heads, dim3(ba_blocks(n)), dim3(256), 0, st, desc, keys, ids, n, exact ? 1 : 0, gid, counters);
    VK_LAUNCH(k_ba_scan_local, dim3(nb), dim3(256), 0, st, gid, n, scan_tmp);
    VK_LAUNCH(k_ba_scan_table, dim3(1), dim3(1024), 0, st, scan_tmp, (uint64_t)nb);
    VK_LAUNCH(k_ba_scan_add, dim3(ba_blocks(n)), dim3(256), 0, st, gid, n, (const uint32_t*)scan_tmp);
    VK_LAUNCH(k_ba_group_heads, dim3(ba_blocks(n)), dim3(256), 0, st, (const uint32_t*)gid, head_pos, counters);
}
void launch_ba_reduce(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* cnt, const uint32_t* gid, const uint32_t* head_pos, uint64_t n, bool check,
                      unsigned long long* sums, uint32_t* nrec, uint32_t* counters) {
    if (!n) return;
    ProfScope ps("k_ba_reduce", st, 16.0 * n);
    VK_LAUNCH(k_ba_reduce, dim3(ba_blocks(n)), dim3(256), 0, st, desc, ids, cnt, gid, head_pos, check ? 1 : 0, sums, nrec, counters);
}
void launch_ba_select(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* head_pos, const unsigned long long* sums, uint64_t n_groups_max, bool collect,
                      uint32_t cap, unsigned long long* ukeys, uint32_t* uvals, uint32_t* counters) {
    if (!n_groups_max) return;
    ProfScope ps("k_ba_select", st, 16.0 * n_groups_max);
    VK_LAUNCH(k_ba_select, dim3(ba_blocks(n_groups_max)), dim3(256), 0, st, desc, ids, head_pos, sums, collect ? 1 : 0, cap, ukeys, uvals, counters);
}
void launch_ba_report(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* cnt, const uint32_t* head_pos, const unsigned long long* sums, const uint32_t* nrec,
                      const uint32_t* uvals, uint32_t n_rep, uint32_t R, uint32_t* out) {
    if (!n_rep) return;
    ProfScope ps("k_ba_report", st, 64.0 * n_rep);
    VK_LAUNCH(k_ba_report, dim3(ba_blocks(n_rep, 64)), dim3(64), 0, st, desc, ids, cnt, head_pos, sums, nrec, uvals, n_rep, R, out);
}

}  // namespace vk
