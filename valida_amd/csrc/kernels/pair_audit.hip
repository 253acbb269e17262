// Pair audit on the device (host/pair_audit.hpp states the contract): which two cells of one row could be changed together without any AIR
// constraint or bus record noticing although one of the two changes alone is noticed.  The design is the mutation audit's
// (mutation_audit.hip), whose fail mask, interaction walk and launch arguments it shares (mutation_eval.hpp): one launch family per chip, one
// thread per trace row r, the workgroup's T rows plus halo and wrap staged once in LDS as [column][T + 2] (a thread's reads of a column are
// consecutive words: no bank conflict), one inlined copy of the chip per kernel.
//   eval     the BasicMachine chips: vchips::eval_chip<CHIP> over a folder whose main(col, next) adds a delta at TWO wave-uniform columns (two
//            scalar compare-selects per main-column read, no scratch); captured AIRs: the register program interpreted with its register file in
//            LDS (CA_INTERPRET); a chip without constraints (MA_BUS_ONLY) evaluates nothing.
//   singles  per row first the w D single mutations of the mutation audit (the folder's second column set to none); each thread keeps its
//            detected bits in LDS words [word][T] (its own lane's word: no conflict, no atomics).  A slice evaluates only the columns its
//            pairs name (`sneed`); slice 0 evaluates all, because it also sums, per q, the pairs c1 < c2 whose singles are both free on the
//            row (one pass over the columns with D running counts): the uncoupled pairs' exact `free` is that sum minus the same sum over
//            the coupled pairs, which the pair walk accumulates.
//   pairs    then the host's list of coupled pairs x D^2 delta pairs of the slice, in the same loop as the baselines and the singles.  The
//            evaluation at row r is skipped when neither column is read as local, the one at row r - 1 when neither is read as next (the
//            flags of the compiled Program, wave-uniform).  Bus rule: per (pair, q) the host's two masks over the interactions (pa_bus_masks:
//            count changes / some field changes, from the affine weights) against `live`, the row's interactions that are records; a chip
//            of more than 32 interactions walks every interaction with both cells changed instead.
//   slices   the pairs are cut into gridDim.y slices of PPS pairs (pa_shape): at most PA_SLICE_ENTRIES entries per slice, which bounds the
//            LDS accumulators, and about 2048 workgroups per launch, so that a chip of height 1 does not run its thousands of evaluations on
//            one thread.  Every slice stages the tile and evaluates the baselines and its columns' singles again.
//   count    per entry the free / compensated rows are reduced per wave (ballot + population count), then per workgroup in LDS; one integer
//            atomic per non-zero (entry, kind, workgroup); the compensated count also goes into the table [entry][workgroup].
//   scan     exclusive prefix of the table over workgroups, per listed entry.
//   list     workgroups that hold a compensated row of rank < R of a listed entry run the evaluation again for those entries (and their
//            columns' singles) alone, keep one bit per (entry, row) in LDS, and one thread per entry walks the bits in row order: rank =
//            prefix + position.  No atomic admits a row.
// LDS (u32 words): 1 + accumulators (count: 2 EM + 32, list: EM (T / 32 + 1), EM = PPS D^2 <= 1024) + w (sneed) + ceil(w D / 32) T (single
// bits) + (w + prep w)(T + 2) (tile) + registers x T (interpreted).  cpu at T = 256, D = 2: 36 KB of list accumulators + 4 KB of bits + 52.6 KB
// of tile = 93 KB, one workgroup more per CU in the counting pass (65 KB); bitwise (79 columns) 123 KB.  T halves down to 64 until the listing
// pass fits 160 KB.  Scratch from the pool: 16 bytes per entry + 8 bytes per (entry, workgroup) + 4 R bytes per listed entry slot.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, columns of programs,
// interactions and pairs are below the width, rows written by `list` are below n and ranks below R).
#include <mutex>
#include <stdexcept>
#include <string>
#include "mutation_eval.hpp"

namespace vk {

#ifndef VGPU_PA_WAVE_ADD
// Adds the number of lanes of this wave whose `pred` holds to *counter (LDS) with one atomic.  Called from wave-uniform control flow only.
__device__ __forceinline__ void pa_wave_add(uint32_t* counter, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (pred && (b & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) atomicAdd(counter, (uint32_t)__popcll(b));  // the lowest lane that has it
}
#endif

constexpr uint32_t PA_NONE = 0xffffffffu;

// One evaluation with up to two mutated main columns c1, c2 (PA_NONE: none) of the same row: the deltas where the cell is read as local
// (dl) and as next (dn) — zero where that copy of the row is not the mutated one.
struct PaRow {
    const uint32_t *lp, *np, *plp, *pnp;
    uint32_t S, c1, c2;
    Fp dl1, dn1, dl2, dn2, first, last, trans;
};

struct PairFolder {
    using Expr = Fp;
    PaRow r;
    uint32_t k;
    MaMask mask;
    __device__ __forceinline__ Fp constant(uint32_t v) const { return Fp::from_canonical(v); }
    __device__ __forceinline__ Fp main(int col, bool next) const {
        const Fp v = Fp::raw((next ? r.np : r.lp)[(uint32_t)col * r.S]);
        const uint32_t d1 = (next ? r.dn1 : r.dl1).v, d2 = (next ? r.dn2 : r.dl2).v;
        return v + Fp::raw((uint32_t)col == r.c1 ? d1 : ((uint32_t)col == r.c2 ? d2 : 0u));  // c1, c2 are wave-uniform: scalar selects
    }
    __device__ __forceinline__ Fp preprocessed(int col, bool next) const { return Fp::raw((next ? r.pnp : r.plp)[(uint32_t)col * r.S]); }
    __device__ __forceinline__ Fp is_first_row() const { return r.first; }
    __device__ __forceinline__ Fp is_last_row() const { return r.last; }
    __device__ __forceinline__ Fp is_transition() const { return r.trans; }
    __device__ __forceinline__ void assert_zero(const Fp& e) { mask.set(k, !e.is_zero()); k++; }
};

template <int CHIP>
__device__ __forceinline__ MaMask pa_eval(const MaArgs& a, const PaRow& r, uint32_t* regs, uint32_t T) {
    if (CHIP >= 0) {
        PairFolder f;
        f.r = r; f.k = 0;
        f.mask.clear();
        vchips::eval_chip(CHIP, f);  // CHIP is a compile-time constant: the switch folds to the one chip
        return f.mask;
    }
    MaMask mask;
    mask.clear();
    uint32_t k = 0;
#define PA_GET(i) (regs[(uint32_t)(i) * T])
#define PA_SET(i, v) (regs[(uint32_t)(i) * T] = (v))
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: PA_SET(in.dst, (uint32_t)in.a | ((uint32_t)in.b << 16)); break;
            case vair::OP_LOAD_MAIN: {
                const Fp v = Fp::raw((in.flag ? r.np : r.lp)[(uint32_t)in.a * r.S]);
                const uint32_t d1 = (in.flag ? r.dn1 : r.dl1).v, d2 = (in.flag ? r.dn2 : r.dl2).v;
                PA_SET(in.dst, (v + Fp::raw((uint32_t)in.a == r.c1 ? d1 : ((uint32_t)in.a == r.c2 ? d2 : 0u))).v);
            } break;
            case vair::OP_LOAD_PREP: PA_SET(in.dst, (in.flag ? r.pnp : r.plp)[(uint32_t)in.a * r.S]); break;
            case vair::OP_SEL_FIRST: PA_SET(in.dst, r.first.v); break;
            case vair::OP_SEL_LAST: PA_SET(in.dst, r.last.v); break;
            case vair::OP_SEL_TRANS: PA_SET(in.dst, r.trans.v); break;
            case vair::OP_ADD: { const uint32_t x = PA_GET(in.a), y = PA_GET(in.b); PA_SET(in.dst, (Fp::raw(x) + Fp::raw(y)).v); } break;
            case vair::OP_SUB: { const uint32_t x = PA_GET(in.a), y = PA_GET(in.b); PA_SET(in.dst, (Fp::raw(x) - Fp::raw(y)).v); } break;
            case vair::OP_MUL: { const uint32_t x = PA_GET(in.a), y = PA_GET(in.b); PA_SET(in.dst, (Fp::raw(x) * Fp::raw(y)).v); } break;
            case vair::OP_NEG: { const uint32_t x = PA_GET(in.a); PA_SET(in.dst, (-Fp::raw(x)).v); } break;
            case vair::OP_ASSERT: { const Fp x = Fp::raw(PA_GET(in.a)); mask.set(k, !x.is_zero()); k++; } break;
            default: break;  // OP_NOP padding
        }
    }
#undef PA_GET
#undef PA_SET
    return mask;
}

// eval_vcol (interactions.hpp) on a row of the LDS tile, before (v0) and after (v1) main columns c1 / c2 got d1 / d2 added; advances pos.
__device__ __forceinline__ void pa_vcol3(const uint32_t* __restrict__ w, uint32_t& pos, const uint32_t* lp, const uint32_t* plp, uint32_t S, uint32_t c1, Fp d1, uint32_t c2, Fp d2, Fp& v0, Fp& v1) {
    const uint32_t nt = w[pos];
    Fp a0 = Fp::raw(w[pos + 1]), a1 = a0;
    pos += 2;
    for (uint32_t t = 0; t < nt; t++, pos += 2) {
        const uint32_t cw = w[pos], col = cw & 0x7fffffffu;
        const Fp wt = Fp::raw(w[pos + 1]);
        const Fp x0 = Fp::raw((cw >> 31) ? plp[col * S] : lp[col * S]);
        const Fp x1 = cw == c1 ? x0 + d1 : (cw == c2 ? x0 + d2 : x0);  // cw == c: a main column (bit 31 clear) and a mutated one
        a0 += wt.v == vg::R_MOD_P ? x0 : x0 * wt;
        a1 += wt.v == vg::R_MOD_P ? x1 : x1 * wt;
    }
    v0 = a0; v1 = a1;
}

// Bus-detected by the definition, both cells changed (the walk a chip of more than 32 interactions gets: MaArgs::bus_walk)
__device__ __forceinline__ bool pa_bus_detected(const uint32_t* __restrict__ iw, const uint32_t* lp, const uint32_t* plp, uint32_t S, uint32_t c1, Fp d1, uint32_t c2, Fp d2) {
    const uint32_t M = iw[0];
    bool det = false;
    for (uint32_t m = 0; m < M; m++) {
        uint32_t pos = iw[2 + m];
        const uint32_t nf = iw[pos + 1];
        pos += 2;
        Fp x0, x1;
        pa_vcol3(iw, pos, lp, plp, S, c1, d1, c2, d2, x0, x1);
        if (x0 != x1) det = true;
        else if (!x0.is_zero())
            for (uint32_t j = 0; j < nf; j++) {
                Fp f0, f1;
                pa_vcol3(iw, pos, lp, plp, S, c1, d1, c2, d2, f0, f1);
                if (f0 != f1) det = true;
            }
    }
    return det;
}

// LDS of k_pa_audit (dynamic, one array): [0] the listing pass's flag, the accumulators (count: [EM][2] counters and [32] sums; list:
// [EM][T / 32] bits and [EM] need flags; EM = PPS D^2), sneed [width], the single bits [ceil(width D / 32)][T], the main tile
// [width][T + 2], the preprocessed tile [prep_width][T + 2], the interpreter's register file [n_regs][T]
__host__ __device__ inline uint32_t pa_acc_words(uint32_t EM, uint32_t T, uint32_t mode) { return mode == MA_LIST ? EM * (T >> 5) + EM : 2u * EM + 32u; }

// Workgroup (x, y): rows [x T, x T + T) and the pairs of slice y.  mode MA_COUNT: totals (launch.hpp: PaArgs) and table[e * NB + x] =
// compensated rows; mode MA_LIST: rows[e * R + rank] = the rank-th compensated row of entry e < e_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_pa_audit(PaArgs v, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                  uint32_t e_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t pa_lds[];
    const MaArgs& a = v.m;
    const uint32_t T = blockDim.x, t = threadIdx.x, S = T + 2, D = a.D, DD = D * D, TW = T >> 5;
    const uint32_t p_lo = blockIdx.y * v.PPS < v.P ? blockIdx.y * v.PPS : v.P, p_hi = p_lo + v.PPS < v.P ? p_lo + v.PPS : v.P;
    const uint32_t e_lo = p_lo * DD, e_hi = p_hi * DD;
    const uint32_t EL = e_hi < e_cut ? e_hi : e_cut;  // the slice's entries that are listed at all: [e_lo, EL)
    const uint32_t EM = v.PPS * DD, SW = (a.width * D + 31u) >> 5;
    const uint32_t n_acc = pa_acc_words(EM, T, mode);
    uint32_t* acc = pa_lds + 1;
    uint32_t* need = acc + EM * TW;  // list: local entry e - e_lo is walked in this workgroup
    uint32_t* sums = acc + 2 * EM;   // count: [0, 16) all pairs, [16, 32) coupled pairs: rows where both singles are free, per q
    uint32_t* sneed = acc + n_acc;   // the singles of this column are evaluated
    uint32_t* sbits = sneed + a.width;
    uint32_t* tm = sbits + SW * T;
    uint32_t* tp = tm + a.width * S;
    uint32_t* regs = tp + a.prep_width * S + t;
    if (t == 0) pa_lds[0] = 0;
    for (uint32_t x = t; x < n_acc + a.width + SW * T; x += T) acc[x] = 0;
    __syncthreads();
    if (mode == MA_LIST) {
        // entry e belongs to thread (e - e_lo) mod T; it is walked here when it has a compensated row in this workgroup and ranks below R left
        for (uint32_t e = e_lo + t; e < EL; e += T)
            if (table[(uint64_t)e * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)e * a.NB + blockIdx.x] < R) {
                const uint32_t pw = v.pairs[e / DD];
                need[e - e_lo] = 1; sneed[pw & 0xffffu] = 1; sneed[pw >> 16] = 1; pa_lds[0] = 1;
            }
        __syncthreads();
        if (!pa_lds[0]) return;  // the whole workgroup
    } else {
        if (blockIdx.y == 0)
            for (uint32_t c = t; c < a.width; c += T) sneed[c] = 1;
        for (uint32_t p = p_lo + t; p < p_hi; p += T) { const uint32_t pw = v.pairs[p]; sneed[pw & 0xffffu] = 1; sneed[pw >> 16] = 1; }
    }
    // the tile: word j of a column is row (base + j - 1) mod n, j = 0 .. rows_here + 1
    const uint64_t base = (uint64_t)blockIdx.x * T;
    const uint32_t rows_here = a.n - base < T ? (uint32_t)(a.n - base) : T;
    for (uint32_t col = 0; col < a.width; col++)
        for (uint32_t j = t; j < rows_here + 2; j += T) tm[col * S + j] = a.main[(uint64_t)col * a.mstride + ((base + j + a.n - 1) & (a.n - 1))];
    for (uint32_t col = 0; col < a.prep_width; col++)
        for (uint32_t j = t; j < rows_here + 2; j += T) tp[col * S + j] = a.prep[(uint64_t)col * a.pstride + ((base + j + a.n - 1) & (a.n - 1))];
    __syncthreads();

    const uint64_t r = base + t, rp = (r + a.n - 1) & (a.n - 1);
    const bool active = r < a.n, single_row = a.n == 1;
    const Fp one = Fp::one(), zero = Fp::zero();
    uint32_t live = 0;  // the interactions of row r that are records (count != 0): bit m
    if (active && !a.bus_walk) {
        const uint32_t M = a.iw[0];
        for (uint32_t m = 0; m < M; m++) {
            uint32_t pos = a.iw[2 + m] + 2;
            Fp c0, c1;
            ma_vcol2(a.iw, pos, tm + t + 1, tp + t + 1, S, PA_NONE, zero, c0, c1);
            live |= c0.is_zero() ? 0u : 1u << m;
        }
    }
    MaMask base0, base1;
    base0.clear(); base1.clear();
    bool air = false;
    // iterations 0, 1: the baselines of rows r and r - 1; then two per single (column, delta): the cell as local, the cell as next; then two
    // per entry (pair, q) of the slice: both cells as local, both as next
    const uint32_t n_s = a.width * D, n_it = 2 + 2 * n_s + 2 * (e_hi - e_lo);
    uint32_t sc = 0, si = 0, pl = 0, qi = 0, qj = 0;
    for (uint32_t it = 0; it < n_it; it++) {
        const bool is_base = it < 2, is_single = !is_base && it < 2 + 2 * n_s;
        const uint32_t which = it & 1u;
        uint32_t c1 = PA_NONE, c2 = PA_NONE, fl = 3u, d1 = 0, d2 = 0;
        bool wanted = true;
        if (is_single) {
            c1 = sc; fl = a.flags[sc]; d1 = a.delta[si];
            wanted = sneed[sc] != 0;  // LDS, wave-uniform
        } else if (!is_base) {
            const uint32_t pw = v.pairs[p_lo + pl];
            c1 = pw & 0xffffu; c2 = pw >> 16;
            fl = a.flags[c1] | a.flags[c2];
            d1 = a.delta[qi]; d2 = a.delta[qj];
            if (mode == MA_LIST) wanted = need[pl * DD + qi * D + qj] != 0;
        }
        if (CHIP != MA_BUS_ONLY) {
            const bool run = wanted && (single_row ? (which == 0 && (fl & 3u)) : (which == 0 ? (fl & 1u) : (fl & 2u)));  // wave-uniform
            if (run && active) {
                // which = 0: the evaluation at row r (the cells are local; for n = 1 also next), 1: at row r - 1 (the cells are next)
                const uint32_t off = which ? 0u : 1u;
                const uint64_t qr = which ? rp : r;
                PaRow q;
                q.lp = tm + t + off; q.np = q.lp + 1; q.plp = tp + t + off; q.pnp = q.plp + 1;
                q.S = S;
                q.first = qr == 0 ? one : zero; q.last = qr == a.n - 1 ? one : zero; q.trans = qr == a.n - 1 ? zero : one;
                q.c1 = c1; q.c2 = c2;
                const bool as_next = which == 1 || single_row;
                q.dl1 = Fp::raw(which == 0 ? d1 : 0u); q.dn1 = Fp::raw(as_next ? d1 : 0u);
                q.dl2 = Fp::raw(which == 0 ? d2 : 0u); q.dn2 = Fp::raw(as_next ? d2 : 0u);
                const MaMask m = pa_eval<CHIP>(a, q, regs, T);
                if (is_base) { if (which) base1 = m; else base0 = m; }
                else air = air || m.newly(which ? base1 : base0);
            }
        }
        if (is_base || which == 0) continue;
        if (is_single) {
            // the single is complete: its bus rule, then its detected bit
            bool bus = false;
            if ((fl & 4u) && active && wanted) {
                if (a.bus_walk) bus = ma_bus_detected(a.iw, tm + t + 1, tp + t + 1, S, sc, Fp::raw(d1));
                else bus = a.flags[a.width + 2 * sc] != 0 || (a.flags[a.width + 2 * sc + 1] & live) != 0;
            }
            const uint32_t b = sc * D + si;
            if (active && (air || bus)) sbits[(b >> 5) * T + t] |= 1u << (b & 31u);
            air = false;
            if (++si == D) { si = 0; sc++; }
            continue;
        }
        // the entry is complete: the bus, then its counts
        const uint32_t q = qi * D + qj, el = pl * DD + q;
        bool bus = false;
        if ((fl & 4u) && active && wanted) {
            if (a.bus_walk) bus = pa_bus_detected(a.iw, tm + t + 1, tp + t + 1, S, c1, Fp::raw(d1), c2, Fp::raw(d2));
            else bus = v.pmasks[2 * (uint64_t)(e_lo + el)] != 0 || (v.pmasks[2 * (uint64_t)(e_lo + el) + 1] & live) != 0;
        }
        const uint32_t b1 = c1 * D + qi, b2 = c2 * D + qj;
        const bool s1 = (sbits[(b1 >> 5) * T + t] >> (b1 & 31u)) & 1u, s2 = (sbits[(b2 >> 5) * T + t] >> (b2 & 31u)) & 1u;
        const bool free_ = active && !air && !bus, comp = free_ && (s1 || s2);
        if (mode == MA_COUNT) {
            pa_wave_add(&acc[2 * el], free_);
            pa_wave_add(&acc[2 * el + 1], comp);
            pa_wave_add(&sums[16 + q], active && !s1 && !s2);
        } else if (comp && wanted) {
            atomicOr(&acc[el * TW + (t >> 5)], 1u << (t & 31u));
        }
        air = false;
        if (++qj == D) { qj = 0; if (++qi == D) { qi = 0; pl++; } }
    }
    if (mode == MA_COUNT && blockIdx.y == 0 && active) {
        // per q = (i, j): the pairs c1 < c2 with single (c1, i) and single (c2, j) both free on this row
        uint32_t cnt[4] = {0, 0, 0, 0}, A[16];
#pragma unroll
        for (int x = 0; x < 16; x++) A[x] = 0;
        for (uint32_t c = 0; c < a.width; c++) {
            uint32_t f[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                f[i] = 0;
                if ((uint32_t)i < D) { const uint32_t b = c * D + i; f[i] = ((sbits[(b >> 5) * T + t] >> (b & 31u)) & 1u) ^ 1u; }
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) A[i * 4 + j] += f[j] ? cnt[i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; i++) cnt[i] += f[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if ((uint32_t)i < D && (uint32_t)j < D && A[i * 4 + j]) atomicAdd(&sums[i * D + j], A[i * 4 + j]);
    }
    __syncthreads();
    if (mode == MA_COUNT) {
        for (uint32_t x = t; x < 2 * (e_hi - e_lo); x += T) {
            const uint32_t c = acc[x];
            if (!c) continue;
            atomicAdd(&totals[2 * (uint64_t)e_lo + x], (unsigned long long)c);
            if (x & 1u) table[(uint64_t)(e_lo + (x >> 1)) * a.NB + blockIdx.x] = c;
        }
        if (t < 32 && sums[t]) atomicAdd(&totals[2 * (uint64_t)v.P * DD + t], (unsigned long long)sums[t]);
        return;
    }
    for (uint32_t e = e_lo + t; e < EL; e += T) {
        if (!need[e - e_lo]) continue;
        uint32_t rank = prefix[(uint64_t)e * a.NB + blockIdx.x];
        const uint32_t* bits = acc + (e - e_lo) * TW;  // LDS
        for (uint32_t j = 0; j < rows_here && rank < R; j++)
            if ((bits[j >> 5] >> (j & 31u)) & 1u) rows[(uint64_t)e * R + rank++] = (uint32_t)(base + j);
    }
}

// scan: block e of the grid handles entry e (when listed and not empty): prefix[e][w] = sum of table[e][w' < w]
__global__ void __launch_bounds__(256) k_pa_scan(const unsigned long long* __restrict__ totals, const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB, uint32_t e_cut) {
    extern __shared__ uint32_t pa_lds[];  // [256] partial sums
    const uint32_t e = blockIdx.x, t = threadIdx.x;
    if (e >= e_cut || totals[2 * e + 1] == 0) return;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)e * NB;
    uint32_t s = 0;
    for (uint32_t w = lo; w < hi; w++) s += row[w];
    pa_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = pa_lds[i]; pa_lds[i] = run; run += x; }
    }
    __syncthreads();
    uint32_t run = pa_lds[t];
    uint32_t* out = prefix + (uint64_t)e * NB;
    for (uint32_t w = lo; w < hi; w++) { out[w] = run; run += row[w]; }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static size_t pa_lds_bytes(const MaArgs& a, uint32_t EM, uint32_t T, uint32_t mode) {
    const size_t SW = ((size_t)a.width * a.D + 31) / 32;
    return 4 * (1 + (size_t)pa_acc_words(EM, T, mode) + a.width + SW * T + ((size_t)a.width + a.prep_width) * (T + 2) + (a.native_chip == CA_INTERPRET ? (size_t)a.n_regs * T : 0));
}

void pa_shape(PaArgs& v) {
    MaArgs& a = v.m;
    const uint32_t DD = a.D * a.D;
    const uint32_t cap = PA_SLICE_ENTRIES / DD;  // pairs per slice at most (64 .. 1024)
    const uint32_t em_max = (v.P < cap ? (v.P ? v.P : 1u) : cap) * DD;
    uint32_t T = 256;
    while (T > 64 && pa_lds_bytes(a, em_max, T, MA_LIST) > 160 * 1024) T >>= 1;
    if (pa_lds_bytes(a, em_max, T, MA_LIST) > 160 * 1024 || pa_lds_bytes(a, em_max, T, MA_COUNT) > 160 * 1024)
        throw std::invalid_argument("pair_audit: the row tile of a chip of " + std::to_string(a.width + a.prep_width) + " columns and " + std::to_string(a.n_regs) +
                                    " program registers does not fit a workgroup's LDS (" + std::to_string(pa_lds_bytes(a, em_max, 64, MA_LIST)) + " bytes for 64 rows, 163840 at most)");
    a.T = T;
    a.NB = (uint32_t)((a.n + T - 1) / T);
    const uint32_t want = a.NB >= 2048 ? 1u : 2048u / a.NB;  // slices wanted: about 2048 workgroups per launch
    uint32_t pps = v.P ? (v.P + want - 1) / want : 1u;
    if (pps > cap) pps = cap;
    v.PPS = pps;
    const uint64_t cy = v.P ? ((uint64_t)v.P + pps - 1) / pps : 1;
    if (cy > 65535) throw std::invalid_argument("pair_audit: the device audit handles up to " + std::to_string(65535ull * cap) + " coupled pairs per chip at " + std::to_string(a.D) + " deltas (got " + std::to_string(v.P) + ")");
    a.CY = (uint32_t)cy;
}

#define PA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void pa_check(const PaArgs& v, uint32_t mode) {
    const MaArgs& a = v.m;
    if (a.K > CA_MAX_CONSTRAINTS) throw std::invalid_argument("pair_audit: the device audit handles up to " + std::to_string(CA_MAX_CONSTRAINTS) + " constraints per chip");
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("pair_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    // the workgroup's u32 sums over pairs hold at most T w (w - 1) / 2 <= 2^31 at 4096 columns; the LDS tile (below) admits about 620 at 64 rows
    if (a.D == 0 || a.D > 4 || a.width == 0 || a.width > 4096) throw std::logic_error("pair_audit: 1 to 4 deltas, 1 to 4096 columns");
    if (v.PPS == 0 || v.PPS * a.D * a.D > PA_SLICE_ENTRIES || a.CY == 0 || a.CY > 65535 || (uint64_t)a.CY * v.PPS < v.P) throw std::logic_error("pair_audit: the slices do not cover the pairs");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.T < 64 || a.T > 256 || (a.T & (a.T - 1)) || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("pair_audit: inconsistent launch shape");
    if (pa_lds_bytes(a, v.PPS * a.D * a.D, a.T, mode) > 160 * 1024) throw std::logic_error("pair_audit: the launch shape does not fit the LDS");
    // the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("pair_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
#define PA_X(C) (void)hipFuncSetAttribute((const void*)k_pa_audit<vchips::C>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    PA_CHIPS(PA_X)
#undef PA_X
    (void)hipFuncSetAttribute((const void*)k_pa_audit<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)k_pa_audit<MA_BUS_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (dev < 64) done |= 1ull << dev;
}

static void pa_launch(hipStream_t st, const PaArgs& v, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows) {
    const dim3 grid(v.m.NB, v.m.CY), block(v.m.T);
    const size_t lds = pa_lds_bytes(v.m, v.PPS * v.m.D * v.m.D, v.m.T, mode);
    switch (v.m.native_chip) {
#define PA_X(C) case vchips::C: VK_LAUNCH((k_pa_audit<vchips::C>), grid, block, lds, st, v, mode, totals, table, prefix, e_cut, R, rows); break;
        PA_CHIPS(PA_X)
#undef PA_X
        case CA_INTERPRET: VK_LAUNCH((k_pa_audit<CA_INTERPRET>), grid, block, lds, st, v, mode, totals, table, prefix, e_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_pa_audit<MA_BUS_ONLY>), grid, block, lds, st, v, mode, totals, table, prefix, e_cut, R, rows); break;
        default: throw std::logic_error("pair_audit: a native chip id without constraints");
    }
}

void launch_pa_count(hipStream_t st, const PaArgs& v, unsigned long long* totals, uint32_t* table) {
    pa_check(v, MA_COUNT);
    static const char* names[14] = {"k_pa_count.cpu", "k_pa_count.program", "k_pa_count.mem", "k_pa_count.add", "k_pa_count.sub", "k_pa_count.mul", "k_pa_count.div", "k_pa_count.shift",
                                    "k_pa_count.lt", "k_pa_count.com", "k_pa_count.bitwise", "k_pa_count.output", "k_pa_count.range", "k_pa_count.static_data"};
    const int id = v.m.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_pa_count.bus" : "k_pa_count");
    ProfScope ps(name, st, 4.0 * (double)v.m.n * (v.m.width + v.m.prep_width) * v.m.CY, v.m.evaluations);  // the profile's per-chip split: row evaluations as its ops
    pa_launch(st, v, MA_COUNT, totals, table, nullptr, 0xffffffffu, 0, nullptr);
}

void launch_pa_scan(hipStream_t st, const PaArgs& v, const unsigned long long* totals, const uint32_t* table, uint32_t* prefix, uint32_t e_cut) {
    pa_check(v, MA_COUNT);
    if (!e_cut) return;
    ProfScope ps("k_pa_scan", st, 8.0 * (double)v.m.NB);
    VK_LAUNCH(k_pa_scan, dim3(e_cut), dim3(256), 256 * 4, st, totals, table, prefix, v.m.NB, e_cut);
}

void launch_pa_list(hipStream_t st, const PaArgs& v, const uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows) {
    pa_check(v, MA_LIST);
    ProfScope ps("k_pa_list", st, 0);
    pa_launch(st, v, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, e_cut, R, rows);
}

}  // namespace vk
