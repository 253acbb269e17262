// Field audit on the device (host/field_audit.hpp states the contract): per trace row and live bus record, which of the record's fields the
// chip's constraints, the counts and the record's other fields leave undetermined to first order, and for the listed rows the witness direction.
//   shape    the rank audit's (kernels/rank_audit.hip): one WAVE per trace row, lane l <-> columns l, l + 64, l + 128; here ONE wave per
//            workgroup, the wave takes the workgroup's T rows one after the other, so nothing is exchanged between waves.  A chip of few rows
//            gets fewer rows per workgroup so that it still makes many workgroups; a chip of height 1 runs on one wave.
//   tile     the workgroup's rows, halo and wrap staged once as [column][S], S = (T + 2) | 1 odd.
//   eval     FaFolder: Expr = (value, derivative), the seed a per-lane compare-select; vchips::eval_chip<CHIP> once per lane word at q = r and
//            once at q = r - 1, every assert_zero leaves one Jacobian row in raw[k][column].  Captured AIRs run the register program with (v, d)
//            registers in LDS (CA_INTERPRET); a chip without constraints (MA_BUS_ONLY) evaluates nothing.  (This file's own copy of the rank
//            audit's folder: that file stays as it is.)
//   base     the reduced basis of C + {psi_*} in LDS as [w][BS], BS = w | 1, the row of pivot column p is row p; built ONCE per row by
//            insertion (ballots of the pivot lanes a row touches, LDS broadcasts of the coefficients).
//   record   per live record its F field rows are reduced modulo the base (not inserted: the base stays) and eliminated as [phi' | I_F] in
//            the small quotient, rows [F][QS], QS = (w + F) | 1, kept reduced so that a new row reads all its coefficients after one ballot: a
//            row whose phi' part vanishes leaves a left-null vector in its tag part; field j FLOATS iff coordinate j is zero in every
//            left-null vector found (they span the left null space: each has a 1 at its own field and zeros at the later ones).  A constant
//            field has phi = 0: its tag e_j is a left-null vector at once.
//   reuse    a chip without constraints depends on the row only through its live set: while the live set repeats the wave keeps the row
//            before's float masks (up to 32 interactions).
//   count    per slot (interaction, field) floating rows, per interaction live rows, in LDS; at the end table[slot][workgroup] and integer
//            atomics on the chip's totals.
//   scan     exclusive prefix of the table over workgroups, per listed slot.
//   list     workgroups that hold a floating row of rank < R of a listed slot compute their rows again; rank = prefix + floating rows before
//            in the workgroup, no atomic admits a row.  Only a listed row needs RREF(S_{m,j}), and never as a whole: the record's other fields
//            make a quotient modulo the base (no tags), phi_{m,j} is reduced against both, its first non-zero column is f, and b_f is read off
//            the base's rows corrected by the quotient's (fa_emit).  The base is never touched, so a row lists any number of fields.
// Wave primitives: fa_ballot and fa_wave_sync, of the same shape as the rank audit's two wrappers (lane broadcasts are LDS reads of one address
// after fa_wave_sync).  An emulation without waves defines VGPU_FA_WAVE_PRIMS and supplies both (tests/emu/field_audit_emu.cpp).
// LDS (u32 words): fa_lds_words below.  Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are
// powers of two, columns of programs and interactions are below the width, fields per interaction at most FA_MAX_FIELDS, rows written by
// `list` have ranks below R and slots below s_cut).
#include <mutex>
#include <stdexcept>
#include <string>
#include "launch.hpp"
#include "interactions.hpp"
#include "../chips/basic_machine.hpp"

namespace vk {

constexpr uint32_t FA_NONE = 0xffffffffu;
constexpr uint32_t FA_OUT_WORDS = 18;  // host/rank_audit.hpp: RA_ROW_WORDS

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

// The witness direction of floating field j of live record m into out [18]: row, n_support, the first 8 (column, coefficient) terms.  The
// base stays as it is: RREF(S_{m,j}) has the base's pivots and those of the quotient Q of the record's OTHER fields modulo the base; its
// base rows are the base's reduced by Q.  phi_{m,j} modulo both is zero on every pivot; its first non-zero column is f, its entry there
// phi . b_f, and b_f has 1 at f, -Q[q][f] at Q's pivots and -(B[p][f] - sum_q B[p][pivot q] Q[q][f]) at the base's.
__device__ __forceinline__ void fa_emit(const FaArgs& a, FaWave& W, uint32_t at, uint32_t nf, uint32_t j, uint32_t row, uint32_t* __restrict__ out) {
    const uint32_t w = W.w, BS = W.BS, QS = W.QS, lane = W.lane;
    uint32_t nq = 0;
    for (uint32_t i = 0; i < nf; i++) {
        if (i == j) continue;
        fa_weight_row(a, W, at, 1 + i);
        fa_reduce(W, W.irow, W.bufa);
        const uint32_t pc = fa_quot_reduce(W, nq, w);
        if (pc != FA_NONE) fa_quot_push(W, nq, pc, w);
    }
    fa_weight_row(a, W, at, 1 + j);
    fa_reduce(W, W.irow, W.bufa);
    const uint32_t f = fa_quot_reduce(W, nq, w);
    if (f == FA_NONE) return;  // a determined field: not reached
    const Fp inv = Fp::raw(W.bufb[f]).inv();
    uint32_t run = 0;
#pragma unroll
    for (int q3 = 0; q3 < 3; q3++) {
        const uint32_t col = lane + 64u * (uint32_t)q3;
        Fp v = Fp::zero();
        if (col < w) {
            if (col == f) v = inv;
            else if (W.row_of[col] != FA_NONE) {
                Fp e = Fp::raw(W.basis[col * BS + f]);
                for (uint32_t q = 0; q < nq; q++) e -= Fp::raw(W.basis[col * BS + W.qpiv[q]]) * Fp::raw(W.quot[q * QS + f]);
                v = -(e * inv);
            } else {
                for (uint32_t q = 0; q < nq; q++)
                    if (W.qpiv[q] == col) v = -(Fp::raw(W.quot[q * QS + f]) * inv);
            }
        }
        const unsigned long long m = fa_ballot(!v.is_zero(), W.slot);
        const uint32_t idx = run + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (!v.is_zero() && idx < 8u) { out[2 + 2 * idx] = col; out[3 + 2 * idx] = v.canonical(); }
        run += (uint32_t)__builtin_popcountll(m);
    }
    if (lane == 0) { out[0] = row; out[1] = run; }
}

// u32 words of a workgroup's LDS: head 8, per slot count / need / running, per interaction live rows / float mask / live flag / weight rows' offset / fields, the tile, the
// wave's state (FaWave).
__host__ __device__ inline uint32_t fa_head_words(const FaArgs& a) { return 8u + 3u * a.NS + 5u * a.M; }
__host__ __device__ inline uint32_t fa_wave_words(const FaArgs& a, bool interpret) {
    const uint32_t w = a.width;
    return 4u + 2u * w + 2u * (w + a.F) + w * (w | 1u) + a.K * w + a.F * ((w + a.F) | 1u) + a.F + (interpret ? 128u * a.n_regs : 0u);
}

// Workgroup x: rows [x T, x T + T).  mode MA_COUNT: totals (launch.hpp: FaArgs) and table[s * NB + x] = floating rows of slot s; mode MA_LIST:
// rows[(s * R + rank) * 18 ..] = the rank-th floating row of slot s < s_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(64) k_fa_audit(FaArgs a, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                 uint32_t s_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t fa_lds[];
    const uint32_t lane = threadIdx.x, w = a.width, T = a.T, S = (T + 2u) | 1u, M = a.M, NS = a.NS;
    uint32_t* cnt = fa_lds + 8;      // [NS] floating rows of the slot
    uint32_t* need = cnt + NS;       // [NS] list: the slot still lacks rows here
    uint32_t* running = need + NS;   // [NS] list: floating rows of the slot so far in this workgroup
    uint32_t* livec = running + NS;  // [M] live rows
    uint32_t* fm = livec + M;        // [M] the row's float mask of the interaction
    uint32_t* lv = fm + M;           // [M] the interaction is live on the row
    uint32_t* wat = lv + M;          // [M] where the interaction's weight rows are (a.wr), staged once: the row loop reads no descriptor from memory
    uint32_t* wnf = wat + M;         // [M] its fields
    uint32_t* tm = wnf + M;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S;
    FaWave W;
    W.w = w; W.BS = w | 1u; W.QS = (w + a.F) | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.irow = W.row_of + w; W.bufa = W.irow + w; W.bufb = W.bufa + w + a.F; W.basis = W.bufb + w + a.F; W.raw = W.basis + w * W.BS;
    W.quot = W.raw + a.K * w; W.qpiv = W.quot + a.F * W.QS;
    W.regs = W.qpiv + a.F + lane;
    for (uint32_t x = lane; x < fa_head_words(a); x += 64u) fa_lds[x] = 0;
    __syncthreads();
    for (uint32_t m = lane; m < M; m += 64u) { const uint32_t at = a.wr[2 + m]; wat[m] = at; wnf[m] = a.wr[at]; }
    __syncthreads();
    if (mode == MA_LIST) {
        for (uint32_t s = lane; s < NS && s < s_cut; s += 64u)
            if (table[(uint64_t)s * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)s * a.NB + blockIdx.x] < R) { need[s] = 1; fa_lds[0] = 1; }
        __syncthreads();
        if (!fa_lds[0]) return;  // the whole workgroup
    }
    // the tile: word j of a column is row (base + j - 1) mod n, j = 0 .. rows_here + 1
    const uint64_t base = (uint64_t)blockIdx.x * T;
    const uint32_t rows_here = a.n - base < T ? (uint32_t)(a.n - base) : T;
    const uint32_t RJ = rows_here + 2;
    for (uint32_t x = lane; x < w * RJ; x += 64u) {
        const uint32_t col = x / RJ, j = x - col * RJ;
        tm[col * S + j] = a.main[(uint64_t)col * a.mstride + ((base + j + a.n - 1) & (a.n - 1))];
    }
    for (uint32_t x = lane; x < a.prep_width * RJ; x += 64u) {
        const uint32_t col = x / RJ, j = x - col * RJ;
        tp[col * S + j] = a.prep[(uint64_t)col * a.pstride + ((base + j + a.n - 1) & (a.n - 1))];
    }
    __syncthreads();

    uint32_t live_prev = 0, s_live = 0, s_float = 0, s_rows = 0;  // wave-uniform
    bool have_prev = false;
    for (uint32_t j = 0; j < rows_here; j++) {
        const uint64_t r = base + j;
        // liveness of every interaction on the row
        uint32_t live = 0;
        for (uint32_t m = 0; m < M; m++) {
            uint32_t pos = a.iw[2 + m] + 2;
            const bool l = !fa_vcol(a.iw, pos, tm + j + 1, tp + j + 1, S).is_zero();
            if (lane == 0) lv[m] = l ? 1u : 0u;
            if (m < 32u) live |= l ? 1u << m : 0u;
        }
        const bool reuse = CHIP == MA_BUS_ONLY && M <= 32u && have_prev && live == live_prev;
        live_prev = live; have_prev = true;
        fa_wave_sync();
        if (!reuse) {
            fa_base<CHIP>(a, W, tm, tp, S, j, r);
            for (uint32_t m = 0; m < M; m++) {
                if (!lv[m]) continue;  // wave-uniform
                const uint32_t mask = fa_record(a, W, wat[m], wnf[m]);
                if (lane == 0) fm[m] = mask;
            }
            fa_wave_sync();
        }
        uint32_t slot0 = 0;
        bool any = false;
        for (uint32_t m = 0; m < M; m++) {
            const uint32_t at = wat[m], nf = wnf[m];
            if (lv[m]) {
                const uint32_t mask = fm[m];
                any = any || mask != 0;
                if (mode == MA_COUNT) {
                    s_live++;
                    s_float += (uint32_t)__builtin_popcount(mask);
                    if (lane == 0) livec[m]++;
                    if (lane < nf && ((mask >> lane) & 1u)) cnt[slot0 + lane]++;
                } else {
                    for (uint32_t b = mask; b; b &= b - 1) {
                        const uint32_t f = (uint32_t)__builtin_ctz(b), s = slot0 + f;
                        if (s >= s_cut || !need[s]) continue;  // wave-uniform
                        const uint32_t rank = prefix[(uint64_t)s * a.NB + blockIdx.x] + running[s];
                        fa_wave_sync();
                        if (lane == 0) running[s]++;
                        fa_wave_sync();
                        if (rank >= R) continue;
                        fa_emit(a, W, at, nf, f, (uint32_t)r, rows + ((uint64_t)s * R + rank) * FA_OUT_WORDS);
                    }
                }
            }
            slot0 += nf;
        }
        if (any) s_rows++;
        fa_wave_sync();  // lv and fm are written again for the next row
    }
    if (mode != MA_COUNT) return;
    __syncthreads();
    for (uint32_t s = lane; s < NS; s += 64u)
        if (cnt[s]) { atomicAdd(&totals[3 + M + s], (unsigned long long)cnt[s]); table[(uint64_t)s * a.NB + blockIdx.x] = cnt[s]; }
    for (uint32_t m = lane; m < M; m += 64u)
        if (livec[m]) atomicAdd(&totals[3 + m], (unsigned long long)livec[m]);
    if (lane == 0) {
        if (s_live) atomicAdd(&totals[0], (unsigned long long)s_live);
        if (s_float) atomicAdd(&totals[1], (unsigned long long)s_float);
        if (s_rows) atomicAdd(&totals[2], (unsigned long long)s_rows);
    }
}

// scan: block s of the grid handles slot s: prefix[s][x] = sum of table[s][x' < x]
__global__ void __launch_bounds__(256) k_fa_scan(const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB) {
    extern __shared__ uint32_t fa_lds[];  // [256] partial sums
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)c * NB;
    uint32_t s = 0;
    for (uint32_t x = lo; x < hi; x++) s += row[x];
    fa_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = fa_lds[i]; fa_lds[i] = run; run += x; }
    }
    __syncthreads();
    uint32_t run = fa_lds[t];
    uint32_t* out = prefix + (uint64_t)c * NB;
    for (uint32_t x = lo; x < hi; x++) { out[x] = run; run += row[x]; }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t fa_lds_bytes(const FaArgs& a, uint32_t T) {
    const size_t S = (T + 2u) | 1u;
    return 4 * ((size_t)fa_head_words(a) + ((size_t)a.width + a.prep_width) * S + fa_wave_words(a, a.native_chip == CA_INTERPRET));
}

void fa_shape(FaArgs& a) {
    const size_t LDS = 160 * 1024;
    if (a.F > FA_MAX_FIELDS)
        throw std::invalid_argument("field_audit: an interaction of " + std::to_string(a.F) + " fields; the device pass keeps a record's float mask in one word: at most " +
                                    std::to_string(FA_MAX_FIELDS) + " fields per interaction");
    if (a.width > 192 || fa_lds_bytes(a, 1) > LDS)
        throw std::invalid_argument("field_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints, " + std::to_string(a.M) + " interactions, " +
                                    std::to_string(a.NS) + " fields (" + std::to_string(a.F) + " at most in one record) and " + std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) +
                                    " interpreted registers does not fit a workgroup's LDS with one wave (" + std::to_string(fa_lds_bytes(a, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + quotient F ((w + F) | 1) + 128 per register + 4 w + 3 F + 12 + 3 fields + 5 interactions + 3 (w + prep w)), 163840 at most; "
                                    "at most 192 columns)");
    // 16 rows per workgroup (64 for a chip without constraints: its wave state is small and most rows reuse the row before's answer), fewer
    // while the chip has under 1024 workgroups or the tile does not fit
    uint32_t t = a.K ? 16 : 64;
    while (t > 1 && (a.n / t < 1024 || fa_lds_bytes(a, t) > LDS)) t >>= 1;
    a.T = t;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define FA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void fa_check(const FaArgs& a) {
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("field_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > 192 || a.F > FA_MAX_FIELDS) throw std::logic_error("field_audit: 1 to 192 columns, at most 32 fields per interaction");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.T == 0 || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("field_audit: inconsistent launch shape");
    if (fa_lds_bytes(a, a.T) > 160 * 1024) throw std::logic_error("field_audit: the launch shape does not fit the LDS");
    // the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("field_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("field_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) + ": " +
                                     hipGetErrorString(e));
    };
#define FA_X(C) opt_in((const void*)k_fa_audit<vchips::C>, "k_fa_audit<" #C ">");
    FA_CHIPS(FA_X)
#undef FA_X
    opt_in((const void*)k_fa_audit<CA_INTERPRET>, "k_fa_audit<CA_INTERPRET>");
    opt_in((const void*)k_fa_audit<MA_BUS_ONLY>, "k_fa_audit<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

static void fa_launch(hipStream_t st, const FaArgs& a, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t s_cut, uint32_t R, uint32_t* rows) {
    const dim3 grid(a.NB), block(64);
    const size_t lds = fa_lds_bytes(a, a.T);
    switch (a.native_chip) {
#define FA_X(C) case vchips::C: VK_LAUNCH((k_fa_audit<vchips::C>), grid, block, lds, st, a, mode, totals, table, prefix, s_cut, R, rows); break;
        FA_CHIPS(FA_X)
#undef FA_X
        case CA_INTERPRET: VK_LAUNCH((k_fa_audit<CA_INTERPRET>), grid, block, lds, st, a, mode, totals, table, prefix, s_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_fa_audit<MA_BUS_ONLY>), grid, block, lds, st, a, mode, totals, table, prefix, s_cut, R, rows); break;
        default: throw std::logic_error("field_audit: a native chip id without constraints");
    }
}

void launch_fa_count(hipStream_t st, const FaArgs& a, unsigned long long* totals, uint32_t* table) {
    fa_check(a);
    if (!a.M) return;  // no interaction, no record: the zeroed totals are the answer
    static const char* names[14] = {"k_fa_count.cpu", "k_fa_count.program", "k_fa_count.mem", "k_fa_count.add", "k_fa_count.sub", "k_fa_count.mul", "k_fa_count.div", "k_fa_count.shift",
                                    "k_fa_count.lt", "k_fa_count.com", "k_fa_count.bitwise", "k_fa_count.output", "k_fa_count.range", "k_fa_count.static_data"};
    const int id = a.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_fa_count.bus" : "k_fa_count");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width), a.evaluations);
    fa_launch(st, a, MA_COUNT, totals, table, nullptr, 0, 0, nullptr);
}

void launch_fa_scan(hipStream_t st, const FaArgs& a, const uint32_t* table, uint32_t* prefix, uint32_t s_cut) {
    fa_check(a);
    if (!s_cut) return;
    ProfScope ps("k_fa_scan", st, 8.0 * (double)a.NB * s_cut);
    VK_LAUNCH(k_fa_scan, dim3(s_cut), dim3(256), 256 * 4, st, table, prefix, a.NB);
}

void launch_fa_list(hipStream_t st, const FaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t s_cut, uint32_t R, uint32_t* rows) {
    fa_check(a);
    ProfScope ps("k_fa_list", st, 0);
    fa_launch(st, a, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, s_cut, R, rows);
}

}  // namespace vk
