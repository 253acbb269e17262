// The field audit's per-row elimination, shared by the kernels that ask it per record (kernels/field_audit.hip states the method; the link
// audit's mask kernel, kernels/link_audit.hip, runs the same base and the same per-record quotient): the dual-number folder and interpreter,
// the reduced basis of C + {psi_*} in LDS, the float mask of a live record.  Wave primitives: fa_ballot and fa_wave_sync; an emulation without
// waves defines VGPU_FA_WAVE_PRIMS and supplies both.
#pragma once
#include "launch.hpp"
#include "interactions.hpp"
#include "../chips/basic_machine.hpp"

namespace vk {

constexpr uint32_t FA_NONE = 0xffffffffu;

#ifndef VGPU_FA_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from wave-uniform control flow only.  (slot: two LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long fa_ballot(bool pred, uint32_t*) { return __ballot(pred); }
// LDS writes of this wave's lanes before it are seen by its lanes after it
__device__ __forceinline__ void fa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

struct FaJet {
    Fp v, d;
    __device__ __forceinline__ FaJet operator+(const FaJet& o) const { return FaJet{v + o.v, d + o.d}; }
    __device__ __forceinline__ FaJet operator-(const FaJet& o) const { return FaJet{v - o.v, d - o.d}; }
    __device__ __forceinline__ FaJet operator-() const { return FaJet{-v, -d}; }
    __device__ __forceinline__ FaJet operator*(const FaJet& o) const { return FaJet{v * o.v, v * o.d + d * o.v}; }
    __device__ __forceinline__ FaJet& operator+=(const FaJet& o) { *this = *this + o; return *this; }
    __device__ __forceinline__ FaJet& operator-=(const FaJet& o) { *this = *this - o; return *this; }
    __device__ __forceinline__ FaJet& operator*=(const FaJet& o) { *this = *this * o; return *this; }
};

// One dual evaluation: local / next rows in the LDS tile (lp: the local row's word of column 0, the next row is the word after; column
// stride S), this lane's seeds (cl: the column whose derivative is 1 where read as local, cn: as next; FA_NONE: none), and where the
// derivative of constraint k goes: out[k * w] when `own`.
struct FaRow {
    const uint32_t *lp, *plp;
    uint32_t S, cl, cn, w;
    Fp first, last, trans;
    uint32_t* out;
    bool own;
};

struct FaFolder {
    using Expr = FaJet;
    FaRow r;
    uint32_t k;
    __device__ __forceinline__ FaJet constant(uint32_t v) const { return FaJet{Fp::from_canonical(v), Fp::zero()}; }
    __device__ __forceinline__ FaJet main(int col, bool next) const {
        const Fp v = Fp::raw(r.lp[(uint32_t)col * r.S + (next ? 1u : 0u)]);
        return FaJet{v, Fp::raw((uint32_t)col == (next ? r.cn : r.cl) ? vg::R_MOD_P : 0u)};
    }
    __device__ __forceinline__ FaJet preprocessed(int col, bool next) const { return FaJet{Fp::raw(r.plp[(uint32_t)col * r.S + (next ? 1u : 0u)]), Fp::zero()}; }
    __device__ __forceinline__ FaJet is_first_row() const { return FaJet{r.first, Fp::zero()}; }
    __device__ __forceinline__ FaJet is_last_row() const { return FaJet{r.last, Fp::zero()}; }
    __device__ __forceinline__ FaJet is_transition() const { return FaJet{r.trans, Fp::zero()}; }
    __device__ __forceinline__ void assert_zero(const FaJet& e) {
        if (r.own) r.out[k * r.w] = e.d.v;
        k++;
    }
};

// CHIP: a vchips::ChipId, or CA_INTERPRET for the register program (regs: this lane's slot of the wave's dual register file: register i has
// its value at regs[128 i] and its derivative at regs[128 i + 64]).
template <int CHIP>
__device__ __forceinline__ void fa_eval(const FaArgs& a, const FaRow& r, uint32_t* regs) {
    if (CHIP >= 0) {
        FaFolder f;
        f.r = r; f.k = 0;
        vchips::eval_chip(CHIP, f);  // CHIP is a compile-time constant: the switch folds to the one chip
        return;
    }
    uint32_t k = 0;
#define FA_V(i) (regs[(uint32_t)(i) * 128u])
#define FA_D(i) (regs[(uint32_t)(i) * 128u + 64u])
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: FA_V(in.dst) = (uint32_t)in.a | ((uint32_t)in.b << 16); FA_D(in.dst) = 0; break;
            case vair::OP_LOAD_MAIN:
                FA_V(in.dst) = r.lp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)];
                FA_D(in.dst) = (uint32_t)in.a == (in.flag ? r.cn : r.cl) ? vg::R_MOD_P : 0u;
                break;
            case vair::OP_LOAD_PREP: FA_V(in.dst) = r.plp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)]; FA_D(in.dst) = 0; break;
            case vair::OP_SEL_FIRST: FA_V(in.dst) = r.first.v; FA_D(in.dst) = 0; break;
            case vair::OP_SEL_LAST: FA_V(in.dst) = r.last.v; FA_D(in.dst) = 0; break;
            case vair::OP_SEL_TRANS: FA_V(in.dst) = r.trans.v; FA_D(in.dst) = 0; break;
            case vair::OP_ADD: { const FaJet x{Fp::raw(FA_V(in.a)), Fp::raw(FA_D(in.a))}, y{Fp::raw(FA_V(in.b)), Fp::raw(FA_D(in.b))}, z = x + y; FA_V(in.dst) = z.v.v; FA_D(in.dst) = z.d.v; } break;
            case vair::OP_SUB: { const FaJet x{Fp::raw(FA_V(in.a)), Fp::raw(FA_D(in.a))}, y{Fp::raw(FA_V(in.b)), Fp::raw(FA_D(in.b))}, z = x - y; FA_V(in.dst) = z.v.v; FA_D(in.dst) = z.d.v; } break;
            case vair::OP_MUL: { const FaJet x{Fp::raw(FA_V(in.a)), Fp::raw(FA_D(in.a))}, y{Fp::raw(FA_V(in.b)), Fp::raw(FA_D(in.b))}, z = x * y; FA_V(in.dst) = z.v.v; FA_D(in.dst) = z.d.v; } break;
            case vair::OP_NEG: { const FaJet x{Fp::raw(FA_V(in.a)), Fp::raw(FA_D(in.a))}, z = -x; FA_V(in.dst) = z.v.v; FA_D(in.dst) = z.d.v; } break;
            case vair::OP_ASSERT:
                if (r.own) r.out[k * r.w] = FA_D(in.a);
                k++;
                break;
            default: break;  // OP_NOP padding
        }
    }
#undef FA_V
#undef FA_D
}

// eval_vcol (interactions.hpp) on a row of the LDS tile; advances pos.  Wave-uniform.
__device__ __forceinline__ Fp fa_vcol(const uint32_t* __restrict__ w, uint32_t& pos, const uint32_t* lp, const uint32_t* plp, uint32_t S) {
    const uint32_t nt = w[pos];
    Fp acc = Fp::raw(w[pos + 1]);
    pos += 2;
    for (uint32_t t = 0; t < nt; t++, pos += 2) {
        const uint32_t cw = w[pos], col = cw & 0x7fffffffu;
        const Fp wt = Fp::raw(w[pos + 1]);
        const Fp x = Fp::raw((cw >> 31) ? plp[col * S] : lp[col * S]);
        acc += wt.v == vg::R_MOD_P ? x : x * wt;
    }
    return acc;
}

// The wave's elimination state (all LDS): slot [4] for fa_ballot, row_of [w] (FA_NONE: not a pivot column; the basis row of pivot column p is
// row p of `basis`), irow [w] (a weight row), bufa / bufb [w + F] (row buffers, ping-pong), basis [w][BS], raw [K][w], quot [F][QS] the
// quotient's rows (phi' on columns < w, the tag on columns w .. w + F), qpiv [F] their pivot columns, the interpreter's registers.
struct FaWave {
    uint32_t *slot, *row_of, *irow, *bufa, *bufb, *basis, *raw, *quot, *qpiv, *regs;
    uint32_t w, BS, QS, WPL, lane, rho;
};

#define FA_EACH_BIT(mask, q, p, body) \
    for (unsigned long long m_ = (mask); m_; m_ &= m_ - 1) { const uint32_t p = (uint32_t)__builtin_ctzll(m_) + 64u * (uint32_t)(q); body }

// out [w] = cur [w] modulo the reduced basis (cur complete and visible to the wave; out visible after it).  Wave-uniform control flow.
__device__ __forceinline__ void fa_reduce(FaWave& W, const uint32_t* cur, uint32_t* out) {
    const uint32_t w = W.w, BS = W.BS, lane = W.lane;
    unsigned long long hit[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        hit[q] = fa_ballot(col < w && W.row_of[col] != FA_NONE && cur[col] != 0, W.slot);
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col >= w) continue;
        Fp acc = Fp::raw(cur[col]);
#pragma unroll
        for (int q = 0; q < 3; q++) FA_EACH_BIT(hit[q], q, p, acc -= Fp::raw(cur[p]) * Fp::raw(W.basis[p * BS + col]);)
        out[col] = acc.v;
    }
    fa_wave_sync();
}

// the first column below w where x is non-zero, or FA_NONE
__device__ __forceinline__ uint32_t fa_first(FaWave& W, const uint32_t* x) {
    uint32_t pc = FA_NONE;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = W.lane + 64u * (uint32_t)q;
        const unsigned long long m = fa_ballot(col < W.w && x[col] != 0, W.slot);
        if (pc == FA_NONE && m) pc = (uint32_t)__builtin_ctzll(m) + 64u * (uint32_t)q;
    }
    return pc;
}

// Inserts the row cur [w] (LDS, complete and visible to the wave) into the reduced basis.  Wave-uniform control flow.  Uses bufa.
__device__ __forceinline__ void fa_insert(FaWave& W, const uint32_t* cur) {
    const uint32_t w = W.w, BS = W.BS, lane = W.lane;
    if (W.rho == w) return;
    uint32_t* nxt = W.bufa;
    fa_reduce(W, cur, nxt);
    const uint32_t pc = fa_first(W, nxt);
    if (pc == FA_NONE) return;
    const Fp lead = Fp::raw(nxt[pc]);
    const Fp inv = (lead == Fp::one() || lead == -Fp::one()) ? lead : lead.inv();
    fa_wave_sync();
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) nxt[col] = (Fp::raw(nxt[col]) * inv).v;
    }
    fa_wave_sync();
    // the older rows that hold the new pivot column: lane <-> their pivot columns
    unsigned long long cm[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        cm[q] = fa_ballot(col < w && W.row_of[col] != FA_NONE && W.basis[col * BS + pc] != 0, W.slot);
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col >= w || col == pc) continue;
        const Fp x = Fp::raw(nxt[col]);
#pragma unroll
        for (int q = 0; q < 3; q++)
            FA_EACH_BIT(cm[q], q, p, { uint32_t* b = W.basis + p * BS; b[col] = (Fp::raw(b[col]) - Fp::raw(b[pc]) * x).v; })
    }
    fa_wave_sync();
    if (lane == (pc & 63u)) {
#pragma unroll
        for (int q = 0; q < 3; q++) FA_EACH_BIT(cm[q], q, p, W.basis[p * BS + pc] = 0;)
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) W.basis[pc * BS + col] = nxt[col];
    }
    fa_wave_sync();
    if (lane == (pc & 63u)) W.row_of[pc] = 1;
    W.rho++;
    fa_wave_sync();
}

// weight row x of interaction m (0: the count, 1 + j: field j) into irow
__device__ __forceinline__ void fa_weight_row(const FaArgs& a, FaWave& W, uint32_t at, uint32_t x) {
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = W.lane + 64u * wd;
        if (col < W.w) W.irow[col] = a.wr[at + 1 + x * W.w + col];
    }
    fa_wave_sync();
}
// the same in two halves, so that the next row's global loads fly while this one is eliminated: this lane's words of weight row x
struct FaWeights { uint32_t v[3]; };
__device__ __forceinline__ FaWeights fa_weight_load(const FaArgs& a, const FaWave& W, uint32_t at, uint32_t x) {
    FaWeights r;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = W.lane + 64u * (uint32_t)q;
        r.v[q] = col < W.w ? a.wr[at + 1 + x * W.w + col] : 0u;
    }
    return r;
}
__device__ __forceinline__ void fa_weight_store(FaWave& W, const FaWeights& r) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = W.lane + 64u * (uint32_t)q;
        if (col < W.w) W.irow[col] = r.v[q];
    }
}

// The reduced basis of C + {psi_*} of row (base + j) of the tile.  first / last / trans are those of evaluations q = r and q = r - 1.
template <int CHIP>
__device__ __forceinline__ void fa_base(const FaArgs& a, FaWave& W, const uint32_t* tm, const uint32_t* tp, uint32_t S, uint32_t j, uint64_t r) {
    const uint32_t w = W.w, lane = W.lane;
    const Fp one = Fp::one(), zero = Fp::zero();
    W.rho = 0;
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) W.row_of[col] = FA_NONE;
    }
    fa_wave_sync();
    if (CHIP != MA_BUS_ONLY) {
        const bool single_row = a.n == 1;
        const uint32_t n_which = single_row ? 1u : 2u;
        for (uint32_t which = 0; which < n_which && W.rho < w; which++) {
            // which = 0: the evaluation at row r (the cell is local; for n = 1 also next), 1: at row r - 1 (the cell is next)
            const uint64_t qr = which ? ((r + a.n - 1) & (a.n - 1)) : r;
            const uint32_t off = which ? 0u : 1u;
            for (uint32_t wd = 0; wd < W.WPL; wd++) {
                const uint32_t col = lane + 64u * wd;
                FaRow q;
                q.lp = tm + j + off; q.plp = tp + j + off; q.S = S; q.w = w;
                q.own = col < w;
                q.cl = (q.own && which == 0) ? col : FA_NONE;
                q.cn = (q.own && (which == 1 || single_row)) ? col : FA_NONE;
                q.first = qr == 0 ? one : zero; q.last = qr == a.n - 1 ? one : zero; q.trans = qr == a.n - 1 ? zero : one;
                q.out = W.raw + (q.own ? col : 0u);
                fa_eval<CHIP>(a, q, W.regs);
            }
            fa_wave_sync();
            for (uint32_t k = 0; k < a.K && W.rho < w; k++) fa_insert(W, W.raw + k * w);
            fa_wave_sync();
        }
    }
    for (uint32_t m = 0; m < a.M && W.rho < w; m++) {
        fa_weight_row(a, W, a.wr[2 + m], 0);
        fa_insert(W, W.irow);
    }
}

// bufb [W2] = bufa [W2] (complete and visible) modulo the quotient's nq REDUCED rows (a row is zero on the other rows' pivot columns, so every
// coefficient can be read before any update); returns the first non-zero column below w of the result, or FA_NONE.  Wave-uniform.
__device__ __forceinline__ uint32_t fa_quot_reduce(FaWave& W, uint32_t nq, uint32_t W2) {
    const uint32_t lane = W.lane, QS = W.QS;
    const unsigned long long hit = fa_ballot(lane < nq && W.bufa[W.qpiv[lane < nq ? lane : 0u]] != 0, W.slot);
    for (uint32_t col = lane; col < W2; col += 64u) {
        Fp acc = Fp::raw(W.bufa[col]);
        FA_EACH_BIT(hit, 0, q, acc -= Fp::raw(W.bufa[W.qpiv[q]]) * Fp::raw(W.quot[q * QS + col]);)
        W.bufb[col] = acc.v;
    }
    fa_wave_sync();
    return fa_first(W, W.bufb);
}

// Appends bufb [W2] with pivot column pc to the quotient: normalised, and column pc cleared from the older rows.  Wave-uniform.
__device__ __forceinline__ void fa_quot_push(FaWave& W, uint32_t& nq, uint32_t pc, uint32_t W2) {
    const uint32_t lane = W.lane, QS = W.QS;
    const Fp lead = Fp::raw(W.bufb[pc]);
    const Fp inv = (lead == Fp::one() || lead == -Fp::one()) ? lead : lead.inv();
    uint32_t* qr = W.quot + nq * QS;
    for (uint32_t col = lane; col < W2; col += 64u) qr[col] = (Fp::raw(W.bufb[col]) * inv).v;
    fa_wave_sync();
    const unsigned long long cm = fa_ballot(lane < nq && W.quot[(lane < nq ? lane : 0u) * QS + pc] != 0, W.slot);
    for (uint32_t col = lane; col < W2; col += 64u) {
        if (col == pc) continue;
        const Fp x = Fp::raw(qr[col]);
        FA_EACH_BIT(cm, 0, q, { uint32_t* b = W.quot + q * QS; b[col] = (Fp::raw(b[col]) - Fp::raw(b[pc]) * x).v; })
    }
    fa_wave_sync();
    if (lane == 0) {
        FA_EACH_BIT(cm, 0, q, W.quot[q * QS + pc] = 0;)
        W.qpiv[nq] = pc;
    }
    nq++;
    fa_wave_sync();
}

// The float mask of live record m (nf fields, weight rows at `at`): bit j set iff field j floats.  The base is left as it is.
__device__ __forceinline__ uint32_t fa_record(const FaArgs& a, FaWave& W, uint32_t at, uint32_t nf) {
    const uint32_t w = W.w, lane = W.lane, W2 = w + nf;
    if (W.rho == w) return 0;  // the base spans everything: every field is determined
    uint32_t nq = 0, det = 0;
    FaWeights pre = fa_weight_load(a, W, at, 1);
    for (uint32_t i = 0; i < nf; i++) {
        fa_weight_store(W, pre);
        if (lane < nf) W.bufa[w + lane] = lane == i ? vg::R_MOD_P : 0u;  // the tag: beside the columns fa_reduce writes
        fa_wave_sync();
        if (i + 1 < nf) pre = fa_weight_load(a, W, at, 2 + i);
        fa_reduce(W, W.irow, W.bufa);
        const uint32_t pc = fa_quot_reduce(W, nq, W2);
        if (pc == FA_NONE) det |= (uint32_t)fa_ballot(lane < nf && W.bufb[w + lane] != 0, W.slot);  // a left-null vector: its tag
        else fa_quot_push(W, nq, pc, W2);
    }
    return ~det & (nf >= 32u ? 0xffffffffu : (1u << nf) - 1u);
}

// u32 words of the wave's state (FaWave)
__host__ __device__ inline uint32_t fa_wave_words(const FaArgs& a, bool interpret) {
    const uint32_t w = a.width;
    return 4u + 2u * w + 2u * (w + a.F) + w * (w | 1u) + a.K * w + a.F * ((w + a.F) | 1u) + a.F + (interpret ? 128u * a.n_regs : 0u);
}

}  // namespace vk
