// Program audit on the device (host/program_audit.hpp states the contract): the fetches of one chip held against the preprocessed table of
// another, read straight from the working layout (column-major Montgomery; every value is made canonical where it is read).
//
//   hist      the fetch counts c[i].  Grid (row runs, bin slices): a workgroup owns min(table height, PG_SLICE) u32 bins in LDS (128 KB of
//             gfx950's 160 KB at the most; a small table takes little and keeps occupancy), walks PG_HIST_RUN contiguous rows in coalesced
//             steps of 256, skips the rows whose pc falls outside its slice, and adds its non-zero bins to the table in device memory.  A wave
//             whose live lanes all hold one pc adds their number from one lane (padding rows are all one pc); any other wave uses one LDS
//             atomicAdd without a return value per live lane.
//   judge     one thread per fetch row: pc and the fields, W[pc] from an LDS copy of the table's word columns when it is small enough to be
//             worth staging per workgroup, else from device memory; the kind and mask; the next row's pc from an LDS tile with one halo row.
//             Counters by ballots, then LDS, then one atomic per counter and workgroup.  The hard and the wrapped findings of a workgroup go to
//             two tables: count -> scan -> list.
//   table     one thread per table row: key, multiplicity, the fetched flag; a range of unfetched words starts where the word before is
//             fetched (or at 0) and ends where the word after is (or at rom_len), both seen through a tile with a halo on either side: the
//             k-th start and the k-th end are one range, so starts and ends are listed by two scans and no thread walks a range.  The hottest
//             word is a maximum of count << 32 | ~pc.
// The only atomics are integer add and max: every word is the same run after run.  No atomic admits a listed record.  Every index is bounded
// by what the host checked (columns inside their traces, rom_len <= table height, both heights <= 2^30); a pc is used as an index only after it
// is compared with the slice or with rom_len.  An emulation without waves defines VGPU_PG_WAVE_PRIMS before including this file and supplies
// pg_ballot and pg_shfl itself (tests/emu/program_audit_emu.cpp).
#include "launch.hpp"
#include "../field.hpp"

namespace vk {

#ifndef VGPU_PG_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from workgroup-uniform control flow only.  (slot: LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long pg_ballot(bool pred, uint32_t*) { return __ballot(pred); }
// the value of `v` on lane `src` of this wave
__device__ __forceinline__ uint32_t pg_shfl(uint32_t v, uint32_t src, uint32_t*) { return (uint32_t)__shfl((int)v, (int)src, 64); }
#endif

constexpr uint32_t PG_SLOT_WORDS = 4 * 66;                        // per wave 66 words for the emulation's primitives
constexpr uint32_t PG_TWO32_MOD_P = vg::R_MOD_P;                 // 2^32 mod p
constexpr uint32_t PG_JUDGE_HEAD = PG_SLOT_WORDS + 260 + 8 + 8;  // slot, pc tile [257] (padded), counters [8], wave counts [2][4]
constexpr uint32_t PG_TABLE_HEAD = PG_SLOT_WORDS + 260 + 8 + 16; // slot, count tile [258] (padded), counters [4] + the hottest (u64), wave counts [4][4]

__device__ __forceinline__ uint32_t pg_cell(const uint32_t* __restrict__ m, uint64_t stride, uint32_t col, uint64_t row) {
    return vg::Fp::raw(m[(uint64_t)col * stride + row]).canonical();
}

// ---- hist -----------------------------------------------------------------------------------------------------------------------------------
// counts [T] u32, zeroed.  LDS: slot, then `bins` words.
__global__ void __launch_bounds__(256) k_pg_hist(const uint32_t* __restrict__ pc_col, uint64_t H, uint32_t T, uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t pg_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* slot = pg_lds + 66u * wave;
    uint32_t* bin = pg_lds + PG_SLOT_WORDS;
    const uint32_t lo = blockIdx.y * PG_SLICE;  // < T: the grid has ceil(T / PG_SLICE) slices
    const uint32_t nb = T - lo < PG_SLICE ? T - lo : PG_SLICE;
    for (uint32_t k = tid; k < nb; k += 256u) bin[k] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PG_HIST_RUN;
    for (uint32_t it = 0; it < PG_HIST_RUN / 256u; it++) {
        const uint64_t r0 = base + (uint64_t)it * 256u;
        if (r0 >= H) break;  // workgroup-uniform
        const uint64_t r = r0 + tid;
        const uint32_t pc = r < H ? vg::Fp::raw(pc_col[r]).canonical() : 0xffffffffu;
        const bool live = pc >= lo && pc - lo < nb;  // a row past the end is all ones: >= p > every bin
        const unsigned long long mask = pg_ballot(live, slot);
        const uint32_t first = mask ? (uint32_t)__builtin_ctzll(mask) : 0u;
        const uint32_t pc0 = pg_shfl(pc, first, slot);
        const bool same = pg_ballot(live && pc == pc0, slot) == mask;
        if (same) {
            if (live && lane == first) atomicAdd(&bin[pc - lo], (uint32_t)__popcll(mask));
        } else if (live) {
            atomicAdd(&bin[pc - lo], 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < nb; k += 256u)
        if (bin[k]) atomicAdd(&counts[lo + k], bin[k]);
}

// ---- judge ----------------------------------------------------------------------------------------------------------------------------------
// tot (u64, zeroed): [0] sequential [1] stay [2] jumps [3] pc out of rom [4] wrong instruction [5] wrapped operand [6] first pc [7] last pc
// (the table pass: [8] table key [9] multiplicity [10] fetched words [11] unfetched ranges [12] max of count << 32 | ~pc).  mode PG_COUNT: the
// counters, hard_tab[workgroup] and wrap_tab[workgroup]; PG_LIST: the tables hold their exclusive prefixes; a hard finding goes to record
// hard_base + its rank, a wrapped one to record out_wrap + its rank, each below its limit.  A record is PG_OUT words: kind, mask, row, pc,
// found[8], expected[8].  LDS: PG_JUDGE_HEAD words, then (a.lds_table) the table's word columns [n_fields][T], canonical.
__global__ void __launch_bounds__(256) k_pg_judge(const PgArgs a, uint32_t mode, unsigned long long* __restrict__ tot, uint32_t* __restrict__ hard_tab, uint32_t* __restrict__ wrap_tab,
                                                  uint32_t hard_base, uint32_t max_hard, uint32_t max_wrapped, uint32_t* __restrict__ out_hard, uint32_t* __restrict__ out_wrap) {
    extern __shared__ uint32_t pg_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* slot = pg_lds + 66u * wave;
    uint32_t* tile = pg_lds + PG_SLOT_WORDS;
    uint32_t* s_cnt = tile + 260;
    uint32_t* s_wave = s_cnt + 8;
    uint32_t* tab = pg_lds + PG_JUDGE_HEAD;
    const uint64_t r = (uint64_t)blockIdx.x * 256u + tid;
    const bool in = r < a.H;
    const uint32_t pc = in ? pg_cell(a.fmain, a.fstride, a.pc_col, r) : 0u;
    tile[tid] = pc;
    if (tid == 0) {  // the halo row: the first row of the next tile
        const uint64_t next = ((uint64_t)blockIdx.x + 1u) * 256u;
        tile[256] = next < a.H ? pg_cell(a.fmain, a.fstride, a.pc_col, next) : 0u;
    }
    if (tid < 8) s_cnt[tid] = 0;
    if (a.lds_table) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (j < a.n_fields)
                for (uint32_t i = tid; i < a.T; i += 256u) tab[j * a.T + i] = pg_cell(a.tprep, a.tpstride, a.table_cols[j], i);
    }
    __syncthreads();
    uint32_t kind = 0, mask = 0, f[8], w[8];
    bool hard = false;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) { f[j] = 0; w[j] = 0; }
    if (in) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (j < a.n_fields) f[j] = pg_cell(a.fmain, a.fstride, a.field_cols[j], r);
        if (pc >= a.rom_len) {
            kind = 2;
        } else {  // pc < rom_len <= T
#pragma unroll
            for (uint32_t j = 0; j < 8; j++)
                if (j < a.n_fields) {
                    w[j] = a.lds_table ? tab[j * a.T + pc] : pg_cell(a.tprep, a.tpstride, a.table_cols[j], pc);
                    if (f[j] != w[j]) {
                        mask |= 1u << j;
                        const uint32_t d = f[j] >= w[j] ? f[j] - w[j] : f[j] + (vg::P - w[j]);
                        hard = hard || d != PG_TWO32_MOD_P;
                    }
                }
            kind = !mask ? 0u : hard ? 3u : 4u;
        }
    }
    const bool is_hard = kind == 2 || kind == 3, is_wrapped = kind == 4;
    if (mode == PG_COUNT) {
        const bool has_next = in && r + 1 < a.H;
        const uint32_t nx = tile[tid + 1];
        const bool seq = has_next && nx == (pc + 1u == vg::P ? 0u : pc + 1u), stay = has_next && nx == pc;
        const bool preds[6] = {seq, stay, has_next && !seq && !stay, kind == 2, kind == 3, kind == 4};
#pragma unroll
        for (uint32_t k = 0; k < 6; k++) {
            const unsigned long long b = pg_ballot(preds[k], slot);
            if (lane == 0 && b) atomicAdd(&s_cnt[k], (uint32_t)__popcll(b));
        }
        if (in && r == 0) tot[6] = pc;  // one writer each in the whole grid
        if (in && r + 1 == a.H) tot[7] = pc;
        __syncthreads();
        if (tid < 6 && s_cnt[tid]) atomicAdd(&tot[tid], (unsigned long long)s_cnt[tid]);
        if (tid == 0) { hard_tab[blockIdx.x] = s_cnt[3] + s_cnt[4]; wrap_tab[blockIdx.x] = s_cnt[5]; }
    } else {
        const unsigned long long hb = pg_ballot(is_hard, slot), wb = pg_ballot(is_wrapped, slot);
        if (lane == 0) { s_wave[wave] = (uint32_t)__popcll(hb); s_wave[4 + wave] = (uint32_t)__popcll(wb); }
        __syncthreads();
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t at = is_hard ? hard_base + hard_tab[blockIdx.x] + (uint32_t)__popcll(hb & below) : wrap_tab[blockIdx.x] + (uint32_t)__popcll(wb & below);
        for (uint32_t v = 0; v < wave; v++) at += s_wave[(is_hard ? 0u : 4u) + v];
        if ((is_hard && at < max_hard) || (is_wrapped && at < max_wrapped)) {
            uint32_t* o = (is_hard ? out_hard : out_wrap) + (uint64_t)at * PG_OUT;
            o[0] = kind; o[1] = mask; o[2] = (uint32_t)r; o[3] = pc;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) { o[4 + j] = f[j]; o[12 + j] = w[j]; }
        }
    }
}

// ---- table ----------------------------------------------------------------------------------------------------------------------------------
// tabs: four tables of NB = ceil(T / 256) words: table key, multiplicity, range starts, range ends (PG_COUNT writes them, PG_LIST reads their
// exclusive prefixes).  A TABLE_KEY record goes to its rank, a MULTIPLICITY record to mult_base + its rank, below max_hard; range k to
// ranges[2 k] (its start writes lo) and ranges[2 k + 1] (its end writes hi), below max_ranges.  LDS: PG_TABLE_HEAD words.
__global__ void __launch_bounds__(256) k_pg_table(const PgArgs a, uint32_t mode, const uint32_t* __restrict__ counts, unsigned long long* __restrict__ tot, uint32_t* __restrict__ tabs,
                                                  uint32_t NB, uint32_t mult_base, uint32_t max_hard, uint32_t max_ranges, uint32_t* __restrict__ out_hard, uint32_t* __restrict__ ranges) {
    extern __shared__ uint32_t pg_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t* slot = pg_lds + 66u * wave;
    uint32_t* cs = pg_lds + PG_SLOT_WORDS;  // cs[1 + t]: the count of this tile's row t; cs[0], cs[257]: the rows before and after the tile
    uint32_t* s_cnt = cs + 260;
    unsigned long long* s_hot = (unsigned long long*)(s_cnt + 4);  // 8-byte aligned: PG_SLOT_WORDS + 264 is even
    uint32_t* s_wave = s_cnt + 8;
    const uint32_t first_row = blockIdx.x * 256u, i = first_row + tid;  // T <= 2^30
    const bool in = i < a.T;
    const uint32_t c = in ? counts[i] : 0u;
    cs[1 + tid] = c;
    if (tid == 0) {
        cs[0] = first_row ? counts[first_row - 1] : 0u;
        cs[257] = first_row + 256u < a.T ? counts[first_row + 256u] : 0u;
        *s_hot = 0;
    }
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t K = in ? pg_cell(a.tprep, a.tpstride, a.key_col, i) : 0u, m = in ? pg_cell(a.tmain, a.tmstride, a.mult_col, i) : 0u;
    const bool key_bad = in && K != i, mult_bad = in && m != c;  // c <= 2^30 < p: c mod p is c
    const bool in_rom = in && i < a.rom_len, fetched = in_rom && c != 0, unfetched = in_rom && c == 0;
    const bool starts = unfetched && (i == 0 || cs[tid] != 0), ends = unfetched && (i + 1 == a.rom_len || cs[tid + 2] != 0);
    const bool preds[4] = {key_bad, mult_bad, starts, ends};
    if (mode == PG_COUNT) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const unsigned long long b = pg_ballot(k == 3 ? fetched : preds[k], slot);  // [3] counts the fetched words; ends are as many as starts
            if (lane == 0 && b) atomicAdd(&s_cnt[k], (uint32_t)__popcll(b));
        }
        if (in && c) atomicMax(s_hot, ((unsigned long long)c << 32) | (unsigned long long)(~i));
        const unsigned long long eb = pg_ballot(ends, slot);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(eb);
        __syncthreads();
        if (tid == 0) {
            if (s_cnt[0]) atomicAdd(&tot[8], (unsigned long long)s_cnt[0]);
            if (s_cnt[1]) atomicAdd(&tot[9], (unsigned long long)s_cnt[1]);
            if (s_cnt[3]) atomicAdd(&tot[10], (unsigned long long)s_cnt[3]);
            if (s_cnt[2]) atomicAdd(&tot[11], (unsigned long long)s_cnt[2]);
            if (*s_hot) atomicMax(&tot[12], *s_hot);
            tabs[blockIdx.x] = s_cnt[0]; tabs[NB + blockIdx.x] = s_cnt[1]; tabs[2 * NB + blockIdx.x] = s_cnt[2];
            tabs[3 * NB + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        }
    } else {
        unsigned long long b[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            b[k] = pg_ballot(preds[k], slot);
            if (lane == 0) s_wave[4 * k + wave] = (uint32_t)__popcll(b[k]);
        }
        __syncthreads();
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (!preds[k]) continue;
            uint32_t at = tabs[k * NB + blockIdx.x] + (uint32_t)__popcll(b[k] & below);
            for (uint32_t v = 0; v < wave; v++) at += s_wave[4 * k + v];
            if (k < 2) {
                at += k ? mult_base : 0u;
                if (at >= max_hard) continue;
                uint32_t* o = out_hard + (uint64_t)at * PG_OUT;
                o[0] = k ? 5u : 1u; o[1] = 0; o[2] = i; o[3] = i;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) { o[4 + j] = 0; o[12 + j] = 0; }
                o[4] = k ? m : K; o[12] = k ? c : i;
                if (k) o[13] = c;
            } else if (at < max_ranges) {
                ranges[2 * at + (k - 2)] = k == 2 ? i : i + 1u;
            }
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
static unsigned pg_blocks(uint64_t n, uint64_t per = 256) { return (unsigned)((n + per - 1) / per); }
static uint32_t pg_hist_bins(uint32_t T) { return T < PG_SLICE ? T : PG_SLICE; }

bool program_audit_lds_table(uint32_t n_fields, uint64_t T) { return (uint64_t)(n_fields + 1) * T <= PG_LDS_TABLE_WORDS; }

void launch_pg_hist(hipStream_t st, const uint32_t* pc_col, uint64_t H, uint32_t T, uint32_t* counts) {
    if (!H || !T) return;
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)k_pg_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((PG_SLOT_WORDS + PG_SLICE) * 4)); attr = true; }
    const unsigned slices = pg_blocks(T, PG_SLICE);
    ProfScope ps("k_pg_hist", st, 4.0 * (double)H * slices + 4.0 * T);
    VK_LAUNCH(k_pg_hist, dim3(pg_blocks(H, PG_HIST_RUN), slices), dim3(256), (PG_SLOT_WORDS + pg_hist_bins(T)) * 4, st, pc_col, H, T, counts);
}
void launch_pg_judge(hipStream_t st, const PgArgs& a, uint32_t mode, unsigned long long* tot, uint32_t* hard_tab, uint32_t* wrap_tab, uint32_t hard_base, uint32_t max_hard,
                     uint32_t max_wrapped, uint32_t* out_hard, uint32_t* out_wrap) {
    if (!a.H) return;
    const unsigned nb = pg_blocks(a.H);
    const size_t lds = (PG_JUDGE_HEAD + (a.lds_table ? a.n_fields * a.T : 0u)) * 4;
    ProfScope ps(mode == PG_COUNT ? "k_pg_judge" : "k_pg_judge_list", st, 4.0 * (double)a.H * (1 + 2 * a.n_fields));
    if (mode == PG_LIST) {  // the tables become their own exclusive prefixes
        launch_mm_scan_words(st, hard_tab, nb, 0);
        launch_mm_scan_words(st, wrap_tab, nb, 0);
    }
    VK_LAUNCH(k_pg_judge, dim3(nb), dim3(256), lds, st, a, mode, tot, hard_tab, wrap_tab, hard_base, max_hard, max_wrapped, out_hard, out_wrap);
}
void launch_pg_table(hipStream_t st, const PgArgs& a, uint32_t mode, const uint32_t* counts, unsigned long long* tot, uint32_t* tabs, uint32_t mult_base, uint32_t max_hard,
                     uint32_t max_ranges, uint32_t* out_hard, uint32_t* ranges) {
    if (!a.T) return;
    const unsigned nb = pg_blocks(a.T);
    ProfScope ps(mode == PG_COUNT ? "k_pg_table" : "k_pg_table_list", st, 16.0 * (double)a.T);
    if (mode == PG_LIST)
        for (uint32_t k = 0; k < 4; k++) launch_mm_scan_words(st, tabs + (uint64_t)k * nb, nb, 0);
    VK_LAUNCH(k_pg_table, dim3(nb), dim3(256), PG_TABLE_HEAD * 4, st, a, mode, counts, tot, tabs, (uint32_t)nb, mult_base, max_hard, max_ranges, out_hard, ranges);
}

}  // namespace vk
