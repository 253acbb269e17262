// What the rank audit's kernels (rank_audit.hip) and the step audit's (step_audit.hip) share, moved here verbatim from rank_audit.hip: the wave
// primitives, the dual numbers and their folder, the dual evaluation, the interaction counts on the LDS tile, the wave's elimination state, the
// row insertion into the reduced basis, the row's basis, the pinned test and the emission of a canonical null vector.  rank_audit.hip's header
// comment describes them.  An emulation without waves defines VGPU_RA_WAVE_PRIMS before including this file and supplies ra_ballot and
// ra_wave_sync itself.
#pragma once
#include "launch.hpp"
#include "interactions.hpp"
#include "../chips/basic_machine.hpp"

namespace vk {

constexpr uint32_t RA_NONE = 0xffffffffu;
constexpr uint32_t RA_OUT_WORDS = 18;  // host/rank_audit.hpp: RA_ROW_WORDS

#ifndef VGPU_RA_WAVE_PRIMS
// bit l: `pred` holds on lane l of this wave.  Called from wave-uniform control flow only.  (slot: two LDS words the emulation goes through)
__device__ __forceinline__ unsigned long long ra_ballot(bool pred, uint32_t*) { return __ballot(pred); }
// LDS writes of this wave's lanes before it are seen by its lanes after it
__device__ __forceinline__ void ra_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

struct RaJet {
    Fp v, d;
    __device__ __forceinline__ RaJet operator+(const RaJet& o) const { return RaJet{v + o.v, d + o.d}; }
    __device__ __forceinline__ RaJet operator-(const RaJet& o) const { return RaJet{v - o.v, d - o.d}; }
    __device__ __forceinline__ RaJet operator-() const { return RaJet{-v, -d}; }
    __device__ __forceinline__ RaJet operator*(const RaJet& o) const { return RaJet{v * o.v, v * o.d + d * o.v}; }
    __device__ __forceinline__ RaJet& operator+=(const RaJet& o) { *this = *this + o; return *this; }
    __device__ __forceinline__ RaJet& operator-=(const RaJet& o) { *this = *this - o; return *this; }
    __device__ __forceinline__ RaJet& operator*=(const RaJet& o) { *this = *this * o; return *this; }
};

// One dual evaluation: local / next rows in the LDS tile (lp: the local row's word of column 0, the next row is the word after; column
// stride S), this lane's seeds (the column whose derivative is 1 where read as local: cl, as next: cn; RA_NONE: none), and where the
// derivative of constraint k goes: out[k * w] when `own`.
struct RaRow {
    const uint32_t *lp, *plp;
    uint32_t S, cl, cn, w;
    Fp first, last, trans;
    uint32_t* out;
    bool own;
};

struct JetFolder {
    using Expr = RaJet;
    RaRow r;
    uint32_t k;
    __device__ __forceinline__ RaJet constant(uint32_t v) const { return RaJet{Fp::from_canonical(v), Fp::zero()}; }
    __device__ __forceinline__ RaJet main(int col, bool next) const {
        const Fp v = Fp::raw(r.lp[(uint32_t)col * r.S + (next ? 1u : 0u)]);                    // one address per wave: a broadcast
        return RaJet{v, Fp::raw((uint32_t)col == (next ? r.cn : r.cl) ? vg::R_MOD_P : 0u)};  // the seed is per lane: a vector compare-select
    }
    __device__ __forceinline__ RaJet preprocessed(int col, bool next) const { return RaJet{Fp::raw(r.plp[(uint32_t)col * r.S + (next ? 1u : 0u)]), Fp::zero()}; }
    __device__ __forceinline__ RaJet is_first_row() const { return RaJet{r.first, Fp::zero()}; }
    __device__ __forceinline__ RaJet is_last_row() const { return RaJet{r.last, Fp::zero()}; }
    __device__ __forceinline__ RaJet is_transition() const { return RaJet{r.trans, Fp::zero()}; }
    __device__ __forceinline__ void assert_zero(const RaJet& e) {
        if (r.own) r.out[k * r.w] = e.d.v;
        k++;
    }
};

// CHIP: a vchips::ChipId, or CA_INTERPRET for the register program (regs: this lane's slot of the wave's dual register file: register i has
// its value at regs[128 i] and its derivative at regs[128 i + 64]).
template <int CHIP>
__device__ __forceinline__ void ra_eval(const RaArgs& a, const RaRow& r, uint32_t* regs) {
    if (CHIP >= 0) {
        JetFolder f;
        f.r = r; f.k = 0;
        vchips::eval_chip(CHIP, f);  // CHIP is a compile-time constant: the switch folds to the one chip
        return;
    }
    uint32_t k = 0;
#define RA_V(i) (regs[(uint32_t)(i) * 128u])
#define RA_D(i) (regs[(uint32_t)(i) * 128u + 64u])
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: RA_V(in.dst) = (uint32_t)in.a | ((uint32_t)in.b << 16); RA_D(in.dst) = 0; break;
            case vair::OP_LOAD_MAIN:
                RA_V(in.dst) = r.lp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)];
                RA_D(in.dst) = (uint32_t)in.a == (in.flag ? r.cn : r.cl) ? vg::R_MOD_P : 0u;
                break;
            case vair::OP_LOAD_PREP: RA_V(in.dst) = r.plp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)]; RA_D(in.dst) = 0; break;
            case vair::OP_SEL_FIRST: RA_V(in.dst) = r.first.v; RA_D(in.dst) = 0; break;
            case vair::OP_SEL_LAST: RA_V(in.dst) = r.last.v; RA_D(in.dst) = 0; break;
            case vair::OP_SEL_TRANS: RA_V(in.dst) = r.trans.v; RA_D(in.dst) = 0; break;
            case vair::OP_ADD: { const RaJet x{Fp::raw(RA_V(in.a)), Fp::raw(RA_D(in.a))}, y{Fp::raw(RA_V(in.b)), Fp::raw(RA_D(in.b))}, z = x + y; RA_V(in.dst) = z.v.v; RA_D(in.dst) = z.d.v; } break;
            case vair::OP_SUB: { const RaJet x{Fp::raw(RA_V(in.a)), Fp::raw(RA_D(in.a))}, y{Fp::raw(RA_V(in.b)), Fp::raw(RA_D(in.b))}, z = x - y; RA_V(in.dst) = z.v.v; RA_D(in.dst) = z.d.v; } break;
            case vair::OP_MUL: { const RaJet x{Fp::raw(RA_V(in.a)), Fp::raw(RA_D(in.a))}, y{Fp::raw(RA_V(in.b)), Fp::raw(RA_D(in.b))}, z = x * y; RA_V(in.dst) = z.v.v; RA_D(in.dst) = z.d.v; } break;
            case vair::OP_NEG: { const RaJet x{Fp::raw(RA_V(in.a)), Fp::raw(RA_D(in.a))}, z = -x; RA_V(in.dst) = z.v.v; RA_D(in.dst) = z.d.v; } break;
            case vair::OP_ASSERT:
                if (r.own) r.out[k * r.w] = RA_D(in.a);
                k++;
                break;
            default: break;  // OP_NOP padding
        }
    }
#undef RA_V
#undef RA_D
}

// eval_vcol (interactions.hpp) on a row of the LDS tile; advances pos.  Wave-uniform.
__device__ __forceinline__ Fp ra_vcol(const uint32_t* __restrict__ w, uint32_t& pos, const uint32_t* lp, const uint32_t* plp, uint32_t S) {
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

// A wave's elimination state (all LDS): slot [2] for ra_ballot, row_of [w] (RA_NONE: not a pivot column; the basis row of pivot column p is
// row p of `basis`: no indirection between a hit and its row), nzf [w] (some raw row is non-zero
// here), nxt [w] and irow [w] (row buffers), basis [w][BS], raw [K][w], the interpreter's registers.
struct RaWave {
    uint32_t *slot, *row_of, *nzf, *nxt, *irow, *basis, *raw, *regs;
    uint32_t w, BS, WPL, lane, rho;
};

#define RA_EACH_BIT(mask, q, p, body) \
    for (unsigned long long m_ = (mask); m_; m_ &= m_ - 1) { const uint32_t p = (uint32_t)__builtin_ctzll(m_) + 64u * (uint32_t)(q); body }

// Inserts the row cur [w] (LDS, complete and visible to the wave) into the reduced basis.  Wave-uniform control flow.
__device__ __forceinline__ void ra_insert(RaWave& W, const uint32_t* cur) {
    const uint32_t w = W.w, BS = W.BS, lane = W.lane;
    bool any = false;
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w && cur[col] != 0) { W.nzf[col] = 1; any = true; }
    }
    if (!ra_ballot(any, W.slot)) return;
    if (W.rho == w) return;
    unsigned long long hit[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        hit[q] = ra_ballot(col < w && W.row_of[col] != RA_NONE && cur[col] != 0, W.slot);
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col >= w) continue;
        Fp acc = Fp::raw(cur[col]);
#pragma unroll
        for (int q = 0; q < 3; q++) RA_EACH_BIT(hit[q], q, p, acc -= Fp::raw(cur[p]) * Fp::raw(W.basis[p * BS + col]);)
        W.nxt[col] = acc.v;
    }
    ra_wave_sync();
    uint32_t pc = RA_NONE;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        const unsigned long long m = ra_ballot(col < w && W.nxt[col] != 0, W.slot);
        if (pc == RA_NONE && m) pc = (uint32_t)__builtin_ctzll(m) + 64u * (uint32_t)q;
    }
    if (pc == RA_NONE) return;
    // wave-uniform: one inversion per new pivot; the leading entries of selector-gated and of bus rows are mostly 1 or -1, their own inverses
    const Fp lead = Fp::raw(W.nxt[pc]);
    const Fp inv = (lead == Fp::one() || lead == -Fp::one()) ? lead : lead.inv();
    ra_wave_sync();
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) W.nxt[col] = (Fp::raw(W.nxt[col]) * inv).v;
    }
    ra_wave_sync();
    // the older rows that hold the new pivot column: lane <-> their pivot columns
    unsigned long long cm[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        cm[q] = ra_ballot(col < w && W.row_of[col] != RA_NONE && W.basis[col * BS + pc] != 0, W.slot);
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col >= w || col == pc) continue;
        const Fp x = Fp::raw(W.nxt[col]);
#pragma unroll
        for (int q = 0; q < 3; q++)
            RA_EACH_BIT(cm[q], q, p, { uint32_t* b = W.basis + p * BS; b[col] = (Fp::raw(b[col]) - Fp::raw(b[pc]) * x).v; })
    }
    ra_wave_sync();
    if (lane == (pc & 63u)) {
#pragma unroll
        for (int q = 0; q < 3; q++) RA_EACH_BIT(cm[q], q, p, W.basis[p * BS + pc] = 0;)
    }
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) W.basis[pc * BS + col] = W.nxt[col];
    }
    ra_wave_sync();  // row_of[pc] is still read above by the other lanes of an emulated wave
    if (lane == (pc & 63u)) W.row_of[pc] = 1;
    W.rho++;
    ra_wave_sync();
}

// The reduced basis of row (base + j) of the tile.  first / last / trans are those of evaluations q = r (index 0) and q = r - 1 (index 1).
template <int CHIP>
__device__ __forceinline__ void ra_row(const RaArgs& a, RaWave& W, const uint32_t* tm, const uint32_t* tp, uint32_t S, uint32_t j, uint64_t r) {
    const uint32_t w = W.w, lane = W.lane;
    const Fp one = Fp::one(), zero = Fp::zero();
    W.rho = 0;
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) { W.row_of[col] = RA_NONE; W.nzf[col] = 0; }
    }
    ra_wave_sync();
    if (CHIP != MA_BUS_ONLY) {
        const bool single_row = a.n == 1;
        const uint32_t n_which = single_row ? 1u : 2u;
        for (uint32_t which = 0; which < n_which && W.rho < w; which++) {
            // which = 0: the evaluation at row r (the cell is local; for n = 1 also next), 1: at row r - 1 (the cell is next)
            const uint64_t qr = which ? ((r + a.n - 1) & (a.n - 1)) : r;
            const uint32_t off = which ? 0u : 1u;
            for (uint32_t wd = 0; wd < W.WPL; wd++) {
                const uint32_t col = lane + 64u * wd;
                RaRow q;
                q.lp = tm + j + off; q.plp = tp + j + off; q.S = S; q.w = w;
                q.own = col < w;
                q.cl = (q.own && which == 0) ? col : RA_NONE;
                q.cn = (q.own && (which == 1 || single_row)) ? col : RA_NONE;
                q.first = qr == 0 ? one : zero; q.last = qr == a.n - 1 ? one : zero; q.trans = qr == a.n - 1 ? zero : one;
                q.out = W.raw + (q.own ? col : 0u);
                ra_eval<CHIP>(a, q, W.regs);
            }
            ra_wave_sync();
            for (uint32_t k = 0; k < a.K && W.rho < w; k++) ra_insert(W, W.raw + k * w);
            ra_wave_sync();
        }
    }
    const uint32_t M = a.wr[0];
    for (uint32_t m = 0; m < M && W.rho < w; m++) {
        const uint32_t at = a.wr[2 + m], nf = a.wr[at];
        uint32_t pos = a.iw[2 + m] + 2;
        const bool live = !ra_vcol(a.iw, pos, tm + j + 1, tp + j + 1, S).is_zero();
        const uint32_t nr = live ? 1u + nf : 1u;
        for (uint32_t x = 0; x < nr && W.rho < w; x++) {
            for (uint32_t wd = 0; wd < W.WPL; wd++) {
                const uint32_t col = lane + 64u * wd;
                if (col < w) W.irow[col] = a.wr[at + 1 + x * w + col];
            }
            ra_wave_sync();
            ra_insert(W, W.irow);
            ra_wave_sync();
        }
    }
}

// pinned: a pivot column whose row of the reduced basis has no other non-zero entry
__device__ __forceinline__ bool ra_pinned(const RaWave& W, uint32_t col) {
    if (W.rho == W.w) return true;
    if (W.row_of[col] == RA_NONE) return false;
    const uint32_t* b = W.basis + col * W.BS;
    uint32_t other = 0;
    for (uint32_t k = 0; k < W.w; k++) other |= k == col ? 0u : b[k];
    return other == 0;
}

// The canonical null vector of loose column c (wave-uniform) into out [18]: row, n_support, the first 8 (column, coefficient) terms.
__device__ __forceinline__ void ra_emit(RaWave& W, uint32_t c, uint32_t row, uint32_t* __restrict__ out) {
    const uint32_t w = W.w, BS = W.BS, lane = W.lane;
    uint32_t f = c;
    if (W.row_of[c] != RA_NONE) {
        const uint32_t i = c;
        f = RA_NONE;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const uint32_t col = lane + 64u * (uint32_t)q;
            const unsigned long long m = ra_ballot(col < w && W.row_of[col] == RA_NONE && W.basis[i * BS + col] != 0, W.slot);
            if (f == RA_NONE && m) f = (uint32_t)__builtin_ctzll(m) + 64u * (uint32_t)q;
        }
        if (f == RA_NONE) return;  // a pinned column: not reached
    }
    uint32_t run = 0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        Fp v = Fp::zero();
        if (col < w) {
            if (col == f) v = Fp::one();
            else if (W.row_of[col] != RA_NONE) v = -Fp::raw(W.basis[col * BS + f]);
        }
        const unsigned long long m = ra_ballot(!v.is_zero(), W.slot);
        const uint32_t idx = run + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (!v.is_zero() && idx < 8u) { out[2 + 2 * idx] = col; out[3 + 2 * idx] = v.canonical(); }
        run += (uint32_t)__builtin_popcountll(m);
    }
    if (lane == 0) { out[0] = row; out[1] = run; }
}

__host__ __device__ inline uint32_t ra_wave_words(uint32_t w, uint32_t K, uint32_t n_regs, bool interpret) { return 4u + 4u * w + w * (w | 1u) + K * w + (interpret ? 128u * n_regs : 0u); }

}  // namespace vk
