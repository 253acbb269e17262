// Arithmetic audit on the device (host/arithmetic_audit.hpp states the contract): the records of one bus recomputed as 32-bit arithmetic, read
// straight from the working layout through the bus audit's descriptor (kernels/bus_records.hpp, so the compiled and the interpreting machine
// give the same words).
//
//   judge     one launch per entry, one thread per row: one descriptor walk (the count; for a live slot the opcode and the twelve bytes), the rule
//             of kernels/arithmetic_rule.hpp in plain integer code, one packed verdict word per slot.  Counters by ballots and __popcll per wave,
//             then LDS, then one integer atomicAdd per counter and workgroup into the entry's totals; the hard and the soft findings of a
//             workgroup go to two tables indexed by the workgroup's number in slot order.
//   list      after the memory audit's one-workgroup scan has made both tables their exclusive prefixes: one thread per row reads its verdict
//             word; a finding below its list's limit walks the descriptor again and writes its record in the report's own layout.  Launched
//             for the entries that have a finding.
// The only atomics are integer add: every word is the same run after run.  No atomic admits a listed record.  Every index is bounded by what the
// host computed (heights, first slots, workgroup numbers, descriptor offsets checked in bus_audit_plan, at least 13 fields per entry).  An
// emulation without waves defines VGPU_AR_WAVE_PRIMS before including this file and supplies ar_ballot itself
// (tests/emu/arithmetic_audit_emu.cpp).
#include "bus_records.hpp"
#include "arithmetic_rule.hpp"

namespace vk {

#ifndef VGPU_AR_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from workgroup-uniform control flow only.  (slot: LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long ar_ballot(bool pred, uint32_t*) { return __ballot(pred); }
#endif

// the record of (chip, interaction m, row): the count, then, for a live slot, the opcode and f[0..11]
__device__ __forceinline__ uint32_t ar_record(const uint32_t* __restrict__ d, const BaChip& c, uint32_t m, uint32_t row, uint32_t& opcode, uint32_t* f) {
    uint32_t pos = d[c.table + 4 * m];
    const uint32_t count = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    if (!count) return 0;
    opcode = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
#pragma unroll
    for (uint32_t j = 0; j < 12; j++) f[j] = eval_vcol(d, pos, c.main, c.mstride, c.prep, c.pstride, row).canonical();
    return count;
}

// ---- judge ----------------------------------------------------------------------------------------------------------------------------------
// tot (AR_TOT u64 of this entry, zeroed): [0] live [1] judged [2] other [3 .. 7] kinds 1 .. 5 [8] mulhs sign matters [9 .. 11] undefined reasons
// 1 .. 3 [12 .. 30] the opcodes.  verdict[first_slot + row]; hard_tab / soft_tab[block_base + workgroup].
__global__ void __launch_bounds__(256) k_ar_judge(const uint32_t* __restrict__ d, uint32_t chip, uint32_t m, uint32_t first_slot, uint32_t block_base, uint32_t* __restrict__ verdict,
                                                  unsigned long long* __restrict__ tot, uint32_t* __restrict__ hard_tab, uint32_t* __restrict__ soft_tab) {
    __shared__ uint32_t s_cnt[AR_TOT];
    __shared__ uint32_t s_slot[4 * 66];
    const BaChip c = ba_chip(d, chip);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x * 256u + tid;
    uint32_t* slot = s_slot + 66 * (tid >> 6);
    if (tid < AR_TOT) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t word = 0;
    if (row < c.height) {
        uint32_t opcode = 0, f[12], expected;
        const uint32_t count = ar_record(d, c, m, row, opcode, f);
        if (count) word = ar_judge(count, opcode, f, &expected);
        verdict[first_slot + row] = word;
    }
    const bool live = word & AR_LIVE, judged = word & AR_JUDGED;
    const uint32_t kind = ar_kind(word), idx = ar_index(word), reason = kind == AR_UNDEFINED ? ar_mask(word) : 0u;
    const bool preds[12] = {live, judged, live && !judged, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, (word & AR_SIGN_MATTERS) != 0, reason == 1, reason == 2, reason == 3};
#pragma unroll
    for (uint32_t k = 0; k < 12; k++) {
        const unsigned long long b = ar_ballot(preds[k], slot);
        if (lane == 0 && b) atomicAdd(&s_cnt[k], (uint32_t)__popcll(b));
    }
    for (uint32_t k = 0; k < AR_OPCODES; k++) {
        const unsigned long long b = ar_ballot(judged && idx == k, slot);
        if (lane == 0 && b) atomicAdd(&s_cnt[12 + k], (uint32_t)__popcll(b));
    }
    __syncthreads();
    if (tid < AR_TOT && s_cnt[tid]) atomicAdd(&tot[tid], (unsigned long long)s_cnt[tid]);
    if (tid == 0) { hard_tab[block_base + blockIdx.x] = s_cnt[3] + s_cnt[4] + s_cnt[5]; soft_tab[block_base + blockIdx.x] = s_cnt[6] + s_cnt[7]; }
}

// ---- list -----------------------------------------------------------------------------------------------------------------------------------
// hard_pre / soft_pre: the tables' exclusive prefixes.  A hard finding goes to record its rank of out_hard below max_hard, a soft one to its rank of
// out_soft below max_soft.  A record is AR_OUT words, the report's: kind, mask or reason, chip, interaction, row, opcode, x[4], y[4], z[4],
// the expected word (0 for kinds 1 and 2), count, is_send, 0, 0, 0.
__global__ void __launch_bounds__(256) k_ar_list(const uint32_t* __restrict__ d, uint32_t chip, uint32_t m, uint32_t is_send, uint32_t first_slot, uint32_t block_base,
                                                 const uint32_t* __restrict__ verdict, const uint32_t* __restrict__ hard_pre, const uint32_t* __restrict__ soft_pre, uint32_t max_hard,
                                                 uint32_t max_soft, uint32_t* __restrict__ out_hard, uint32_t* __restrict__ out_soft) {
    __shared__ uint32_t s_wave[8];
    __shared__ uint32_t s_slot[4 * 66];
    const BaChip c = ba_chip(d, chip);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, row = blockIdx.x * 256u + tid;
    uint32_t* slot = s_slot + 66 * wave;
    const uint32_t word = row < c.height ? verdict[first_slot + row] : 0u;
    const bool is_hard = ar_is_hard(word), is_soft = ar_is_soft(word);
    const unsigned long long hb = ar_ballot(is_hard, slot), sb = ar_ballot(is_soft, slot);
    if (lane == 0) { s_wave[wave] = (uint32_t)__popcll(hb); s_wave[4 + wave] = (uint32_t)__popcll(sb); }
    __syncthreads();
    if (!is_hard && !is_soft) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t at = is_hard ? hard_pre[block_base + blockIdx.x] + (uint32_t)__popcll(hb & below) : soft_pre[block_base + blockIdx.x] + (uint32_t)__popcll(sb & below);
    for (uint32_t v = 0; v < wave; v++) at += s_wave[(is_hard ? 0u : 4u) + v];
    if (at >= (is_hard ? max_hard : max_soft)) return;
    uint32_t opcode = 0, f[12], expected;
    const uint32_t count = ar_record(d, c, m, row, opcode, f);  // live: the verdict says so
    (void)ar_judge(count, opcode, f, &expected);
    uint32_t* o = (is_hard ? out_hard : out_soft) + (uint64_t)at * AR_OUT;
    o[0] = ar_kind(word); o[1] = ar_mask(word); o[2] = chip; o[3] = m; o[4] = row; o[5] = opcode;
#pragma unroll
    for (uint32_t j = 0; j < 12; j++) o[6 + j] = f[j];
    o[18] = ar_kind(word) <= AR_UNDEFINED ? 0u : expected; o[19] = count; o[20] = is_send; o[21] = 0; o[22] = 0; o[23] = 0;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
static unsigned ar_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

void launch_ar_judge(hipStream_t st, const uint32_t* desc, uint32_t chip, uint32_t m, uint64_t height, uint32_t first_slot, uint32_t block_base, uint32_t* verdict,
                     unsigned long long* tot, uint32_t* hard_tab, uint32_t* soft_tab) {
    if (!height) return;
    ProfScope ps("k_ar_judge", st, 4.0 * 15.0 * (double)height);
    VK_LAUNCH(k_ar_judge, dim3(ar_blocks(height)), dim3(256), 0, st, desc, chip, m, first_slot, block_base, verdict, tot, hard_tab, soft_tab);
}
void launch_ar_scan(hipStream_t st, uint32_t* hard_tab, uint32_t* soft_tab, uint64_t n_blocks) {
    ProfScope ps("k_ar_scan", st, 16.0 * (double)n_blocks);
    launch_mm_scan_words(st, hard_tab, n_blocks, 0);
    launch_mm_scan_words(st, soft_tab, n_blocks, 0);
}
void launch_ar_list(hipStream_t st, const uint32_t* desc, uint32_t chip, uint32_t m, uint32_t is_send, uint64_t height, uint32_t first_slot, uint32_t block_base,
                    const uint32_t* verdict, const uint32_t* hard_pre, const uint32_t* soft_pre, uint32_t max_hard, uint32_t max_soft, uint32_t* out_hard, uint32_t* out_soft) {
    if (!height) return;
    ProfScope ps("k_ar_list", st, 4.0 * (double)height);
    VK_LAUNCH(k_ar_list, dim3(ar_blocks(height)), dim3(256), 0, st, desc, chip, m, is_send, first_slot, block_base, verdict, hard_pre, soft_pre, max_hard, max_soft, out_hard, out_soft);
}

}  // namespace vk
