// The evaluation code that the mutation audit (mutation_audit.hip) and the coverage audit (coverage_audit.hip) share: one Air::eval of a row of
// the workgroup's LDS tile with one main cell changed, reduced to the row's fail mask, for the compiled chip templates and for the interpreted
// register program; and the chip's interactions on that row before and after the change.  Both audits evaluate the same mutations on the same
// domain (host/mutation_audit.hpp); they differ in what they keep of the result.
#pragma once
#include "launch.hpp"
#include "interactions.hpp"
#include "../chips/basic_machine.hpp"

namespace vk {

struct MaMask {
    uint32_t w[CA_MASK_WORDS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < (int)CA_MASK_WORDS; i++) w[i] = 0;
    }
    __device__ __forceinline__ void set(uint32_t k, bool on) {
        const uint32_t b = on ? 1u << (k & 31u) : 0u;  // selects, not w[k >> 5]: a run-time k would put the mask in scratch
        w[0] |= k < 32u ? b : 0u;
        w[1] |= (k >= 32u && k < 64u) ? b : 0u;
        w[2] |= k >= 64u ? b : 0u;
    }
    // some constraint fails here that did not fail in `base`
    __device__ __forceinline__ bool newly(const MaMask& base) const {
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < (int)CA_MASK_WORDS; i++) o |= w[i] & ~base.w[i];
        return o != 0;
    }
};

// One evaluation: local / next rows in the LDS tile (lp / np: the row's word of column 0; column stride S), the mutated column c (0xffffffff:
// none) with the delta to add where it is read as local (dl) and as next (dn) — zero where that copy of the cell is not the mutated one.
struct MaRow {
    const uint32_t *lp, *np, *plp, *pnp;
    uint32_t S, c;
    Fp dl, dn, first, last, trans;
};

struct MutationFolder {
    using Expr = Fp;
    MaRow r;
    uint32_t k;
    MaMask mask;
    __device__ __forceinline__ Fp constant(uint32_t v) const { return Fp::from_canonical(v); }
    __device__ __forceinline__ Fp main(int col, bool next) const {
        const Fp v = Fp::raw((next ? r.np : r.lp)[(uint32_t)col * r.S]);
        return v + Fp::raw((uint32_t)col == r.c ? (next ? r.dn : r.dl).v : 0u);  // r.c is wave-uniform: a scalar select
    }
    __device__ __forceinline__ Fp preprocessed(int col, bool next) const { return Fp::raw((next ? r.pnp : r.plp)[(uint32_t)col * r.S]); }
    __device__ __forceinline__ Fp is_first_row() const { return r.first; }
    __device__ __forceinline__ Fp is_last_row() const { return r.last; }
    __device__ __forceinline__ Fp is_transition() const { return r.trans; }
    __device__ __forceinline__ void assert_zero(const Fp& e) { mask.set(k, !e.is_zero()); k++; }
};

// The fail mask of one evaluation.  CHIP: a vchips::ChipId, or CA_INTERPRET for the register program (regs: this thread's slot of the LDS
// register file, slot stride T).
template <int CHIP>
__device__ __forceinline__ MaMask ma_eval(const MaArgs& a, const MaRow& r, uint32_t* regs, uint32_t T) {
    if (CHIP >= 0) {
        MutationFolder f;
        f.r = r; f.k = 0;
        f.mask.clear();
        vchips::eval_chip(CHIP, f);  // CHIP is a compile-time constant: the switch folds to the one chip
        return f.mask;
    }
    MaMask mask;
    mask.clear();
    uint32_t k = 0;
#define MA_GET(i) (regs[(uint32_t)(i) * T])
#define MA_SET(i, v) (regs[(uint32_t)(i) * T] = (v))
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: MA_SET(in.dst, (uint32_t)in.a | ((uint32_t)in.b << 16)); break;
            case vair::OP_LOAD_MAIN: {
                const Fp v = Fp::raw((in.flag ? r.np : r.lp)[(uint32_t)in.a * r.S]);
                MA_SET(in.dst, (v + Fp::raw((uint32_t)in.a == r.c ? (in.flag ? r.dn : r.dl).v : 0u)).v);
            } break;
            case vair::OP_LOAD_PREP: MA_SET(in.dst, (in.flag ? r.pnp : r.plp)[(uint32_t)in.a * r.S]); break;
            case vair::OP_SEL_FIRST: MA_SET(in.dst, r.first.v); break;
            case vair::OP_SEL_LAST: MA_SET(in.dst, r.last.v); break;
            case vair::OP_SEL_TRANS: MA_SET(in.dst, r.trans.v); break;
            case vair::OP_ADD: { const uint32_t x = MA_GET(in.a), y = MA_GET(in.b); MA_SET(in.dst, (Fp::raw(x) + Fp::raw(y)).v); } break;
            case vair::OP_SUB: { const uint32_t x = MA_GET(in.a), y = MA_GET(in.b); MA_SET(in.dst, (Fp::raw(x) - Fp::raw(y)).v); } break;
            case vair::OP_MUL: { const uint32_t x = MA_GET(in.a), y = MA_GET(in.b); MA_SET(in.dst, (Fp::raw(x) * Fp::raw(y)).v); } break;
            case vair::OP_NEG: { const uint32_t x = MA_GET(in.a); MA_SET(in.dst, (-Fp::raw(x)).v); } break;
            case vair::OP_ASSERT: { const Fp x = Fp::raw(MA_GET(in.a)); mask.set(k, !x.is_zero()); k++; } break;
            default: break;  // OP_NOP padding
        }
    }
#undef MA_GET
#undef MA_SET
    return mask;
}

// eval_vcol (interactions.hpp) on a row of the LDS tile, before (v0) and after (v1) column c of the main trace got d added; advances pos.
__device__ __forceinline__ void ma_vcol2(const uint32_t* __restrict__ w, uint32_t& pos, const uint32_t* lp, const uint32_t* plp, uint32_t S, uint32_t c, Fp d, Fp& v0, Fp& v1) {
    const uint32_t nt = w[pos];
    Fp a0 = Fp::raw(w[pos + 1]), a1 = a0;
    pos += 2;
    for (uint32_t t = 0; t < nt; t++, pos += 2) {
        const uint32_t cw = w[pos], col = cw & 0x7fffffffu;
        const Fp wt = Fp::raw(w[pos + 1]);
        const Fp x0 = Fp::raw((cw >> 31) ? plp[col * S] : lp[col * S]);
        const Fp x1 = cw == c ? x0 + d : x0;  // cw == c: a main column (bit 31 clear) and the mutated one
        a0 += wt.v == vg::R_MOD_P ? x0 : x0 * wt;
        a1 += wt.v == vg::R_MOD_P ? x1 : x1 * wt;
    }
    v0 = a0; v1 = a1;
}

// Bus-detected by the definition: the record (count, fields) of some interaction of the row differs; an interaction of count 0 is no record.
// Field elements are compared in Montgomery form (a bijection of the canonical values; 0 is 0).  This walk of every interaction per mutation
// is what a chip of more than 32 interactions gets (MaArgs::bus_walk).  Otherwise the kernel uses what the descriptors prove: a virtual column
// is affine with constant weights, so adding d != 0 to column c changes it by d times the sum of c's weights in it — it changes iff that sum is
// non-zero, whatever the row holds.  Per column the host gives two masks over the interactions (ma_bus_masks): A, those whose count changes,
// and B, those with a field that changes; per row the kernel evaluates the counts once (`live`: the interactions that are records); the
// mutation is bus-detected iff A != 0 or (B & live) != 0.
__device__ __forceinline__ bool ma_bus_detected(const uint32_t* __restrict__ iw, const uint32_t* lp, const uint32_t* plp, uint32_t S, uint32_t c, Fp d) {
    const uint32_t M = iw[0];
    bool det = false;
    for (uint32_t m = 0; m < M; m++) {
        uint32_t pos = iw[2 + m];
        const uint32_t nf = iw[pos + 1];
        pos += 2;
        Fp c0, c1;
        ma_vcol2(iw, pos, lp, plp, S, c, d, c0, c1);
        if (c0 != c1) det = true;
        else if (!c0.is_zero())
            for (uint32_t j = 0; j < nf; j++) {
                Fp f0, f1;
                ma_vcol2(iw, pos, lp, plp, S, c, d, f0, f1);
                if (f0 != f1) det = true;
            }
    }
    return det;
}

// The same walk keeping WHICH interactions' records differ: bit m - m_lo for interaction m of [m_lo, m_lo + 32).
__device__ __forceinline__ uint32_t ma_bus_changed(const uint32_t* __restrict__ iw, const uint32_t* lp, const uint32_t* plp, uint32_t S, uint32_t c, Fp d, uint32_t m_lo) {
    const uint32_t M = iw[0], m_hi = m_lo + 32u < M ? m_lo + 32u : M;
    uint32_t det = 0;
    for (uint32_t m = m_lo; m < m_hi; m++) {
        uint32_t pos = iw[2 + m];
        const uint32_t nf = iw[pos + 1];
        pos += 2;
        Fp c0, c1;
        ma_vcol2(iw, pos, lp, plp, S, c, d, c0, c1);
        bool differs = c0 != c1;
        if (!differs && !c0.is_zero())
            for (uint32_t j = 0; j < nf; j++) {
                Fp f0, f1;
                ma_vcol2(iw, pos, lp, plp, S, c, d, f0, f1);
                if (f0 != f1) differs = true;
            }
        det |= differs ? 1u << (m - m_lo) : 0u;
    }
    return det;
}

}  // namespace vk
