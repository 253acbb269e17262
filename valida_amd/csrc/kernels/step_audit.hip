// Step audit on the device (host/step_audit.hpp states the contract): per trace row the rank audit's reduced basis of the row's Jacobian, then
// the finite moves M[r] + t v_f along the basis vector of every non-pivot column f for every step t, judged by Air::eval at q = r and q = r - 1
// against the row's own baseline.
//   shape    rank_audit.hip's: one WAVE per trace row, lane <-> column for the dual evaluation and the elimination (rank_elim.hpp: the very
//            functions of the rank audit), NW waves per workgroup, RPW rows per wave, the tile [column][S] with halo and wrap.
//   baseline while the Jacobian rows are produced the VALUE part of every assert_zero says whether constraint k is non-zero on M at that q: one
//            bit per (q, k) in LDS (the value is the same on every lane; lane 0 records it).  No fixed limit on K.
//   items    after the elimination the row has nu = w - rho non-pivot columns; the work items are (non-pivot column f, step s), nu S of them,
//            item = index of f among the non-pivot columns times S plus s.  Lane l takes items l, l + 64, ...: ceil(nu S / 64) passes.
//   move     StepFolder, Expr = Fp: main(col, next) adds t v_f[col] where (col, role) is the moved row's role at this q (wave-uniform);
//            v_f[col] = 1 at f, -basis[col][f] for a pivot column (wave-uniform test, a per-lane LDS read of the coefficient), else 0.
//            assert_zero ORs (value != 0 and baseline bit clear) into one flag.  Two evaluations per pass (q = r, q = r - 1), one for n = 1.
//            Captured AIRs run the register program on the value half of the dual register file.  The bus rule is not evaluated: v_f
//            annihilates every count row and every live field row, the word for it stays 0.
//   masks    the pass bits of an item go to LDS by ballot; every loose column c finds the non-pivot column f(c) whose vector it takes (itself,
//            or the first other non-zero entry of its reduced basis row) and assembles its S bits.
//   bus-only a chip without constraints evaluates nothing: every loose column is exact; the basis is reused across rows of equal live sets.
//   count    per column loose / zero / exact / coupled-and-exact / listable rows by LDS atomics, integer atomics on the chip's totals, the
//            listable count into table[column][workgroup]; scan: the rank audit's k_ra_scan; list: workgroups that hold a needed row run
//            their rows again, ranks from prefix + running + the waves before: no atomic admits a row.
// LDS (u32 words): 8 + (7 + NW) w + (w + prep w) S + per wave (the rank audit's words + 24 pass-bit words + ceil(2 K / 32) baseline words).
// Every index is bounded by what the host computed, as in rank_audit.hip; items < nu S <= 192 * 4 = 768 = 24 * 32 pass bits.
#include <mutex>
#include <stdexcept>
#include <string>
#include "rank_elim.hpp"

namespace vk {

constexpr uint32_t SA_OUT_WORDS = 20;   // host/step_audit.hpp: SA_ROW_WORDS
constexpr uint32_t SA_PASS_WORDS = 24;  // 768 items

// JetFolder that also records the baseline: bl (null on every lane but one) gets bit (bit0 + k) when constraint k is non-zero on M
struct SaJetFolder : JetFolder {
    uint32_t* bl;
    uint32_t bit0;
    __device__ __forceinline__ void assert_zero(const RaJet& e) {
        if (bl && !e.v.is_zero()) bl[(bit0 + k) >> 5] |= 1u << ((bit0 + k) & 31u);
        JetFolder::assert_zero(e);
    }
};

// ra_eval with the baseline bits
template <int CHIP>
__device__ __forceinline__ void sa_jet_eval(const RaArgs& a, const RaRow& r, uint32_t* regs, uint32_t* bl, uint32_t bit0) {
    if (CHIP >= 0) {
        SaJetFolder f;
        f.r = r; f.k = 0; f.bl = bl; f.bit0 = bit0;
        vchips::eval_chip(CHIP, f);
        return;
    }
    uint32_t k = 0;
#define SA_V(i) (regs[(uint32_t)(i) * 128u])
#define SA_D(i) (regs[(uint32_t)(i) * 128u + 64u])
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: SA_V(in.dst) = (uint32_t)in.a | ((uint32_t)in.b << 16); SA_D(in.dst) = 0; break;
            case vair::OP_LOAD_MAIN:
                SA_V(in.dst) = r.lp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)];
                SA_D(in.dst) = (uint32_t)in.a == (in.flag ? r.cn : r.cl) ? vg::R_MOD_P : 0u;
                break;
            case vair::OP_LOAD_PREP: SA_V(in.dst) = r.plp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)]; SA_D(in.dst) = 0; break;
            case vair::OP_SEL_FIRST: SA_V(in.dst) = r.first.v; SA_D(in.dst) = 0; break;
            case vair::OP_SEL_LAST: SA_V(in.dst) = r.last.v; SA_D(in.dst) = 0; break;
            case vair::OP_SEL_TRANS: SA_V(in.dst) = r.trans.v; SA_D(in.dst) = 0; break;
            case vair::OP_ADD: { const RaJet x{Fp::raw(SA_V(in.a)), Fp::raw(SA_D(in.a))}, y{Fp::raw(SA_V(in.b)), Fp::raw(SA_D(in.b))}, z = x + y; SA_V(in.dst) = z.v.v; SA_D(in.dst) = z.d.v; } break;
            case vair::OP_SUB: { const RaJet x{Fp::raw(SA_V(in.a)), Fp::raw(SA_D(in.a))}, y{Fp::raw(SA_V(in.b)), Fp::raw(SA_D(in.b))}, z = x - y; SA_V(in.dst) = z.v.v; SA_D(in.dst) = z.d.v; } break;
            case vair::OP_MUL: { const RaJet x{Fp::raw(SA_V(in.a)), Fp::raw(SA_D(in.a))}, y{Fp::raw(SA_V(in.b)), Fp::raw(SA_D(in.b))}, z = x * y; SA_V(in.dst) = z.v.v; SA_D(in.dst) = z.d.v; } break;
            case vair::OP_NEG: { const RaJet x{Fp::raw(SA_V(in.a)), Fp::raw(SA_D(in.a))}, z = -x; SA_V(in.dst) = z.v.v; SA_D(in.dst) = z.d.v; } break;
            case vair::OP_ASSERT:
                if (bl && SA_V(in.a) != 0) bl[(bit0 + k) >> 5] |= 1u << ((bit0 + k) & 31u);
                if (r.own) r.out[k * r.w] = SA_D(in.a);
                k++;
                break;
            default: break;  // OP_NOP padding
        }
    }
#undef SA_D
}

// ra_row with the baseline: bl [ceil(2 K / 32)] gets bit (which K + k), which = 0: q = r, 1: q = r - 1
template <int CHIP>
__device__ __forceinline__ void sa_row(const RaArgs& a, RaWave& W, const uint32_t* tm, const uint32_t* tp, uint32_t S, uint32_t j, uint64_t r, uint32_t* bl) {
    const uint32_t w = W.w, lane = W.lane;
    const Fp one = Fp::one(), zero = Fp::zero();
    W.rho = 0;
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col < w) { W.row_of[col] = RA_NONE; W.nzf[col] = 0; }
    }
    for (uint32_t x = lane; x < (2u * a.K + 31u) / 32u; x += 64u) bl[x] = 0;
    ra_wave_sync();
    if (CHIP != MA_BUS_ONLY) {
        const bool single_row = a.n == 1;
        const uint32_t n_which = single_row ? 1u : 2u;
        for (uint32_t which = 0; which < n_which && W.rho < w; which++) {
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
                sa_jet_eval<CHIP>(a, q, W.regs, (lane == 0 && wd == 0) ? bl : nullptr, which * a.K);
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

// One plain evaluation of a moved row: local / next rows as RaRow (lp: the local row's word of column 0, the next row the word after), the
// wave's basis, this lane's non-pivot column f and step t (zero: no item), which roles the moved row has at this q, the baseline bits.
struct SaStep {
    const uint32_t *lp, *plp, *row_of, *basis, *bl;
    uint32_t S, BS, f, bit0;
    Fp t, first, last, trans;
    bool mv_local, mv_next;
    __device__ __forceinline__ Fp load(uint32_t col, bool next) const {
        Fp v = Fp::raw(lp[col * S + (next ? 1u : 0u)]);  // one address per wave: a broadcast
        if (next ? mv_next : mv_local) {                 // wave-uniform
            if (row_of[col] != RA_NONE) v -= t * Fp::raw(basis[col * BS + f]);  // wave-uniform test; the coefficient is per lane
            else v += Fp::raw(col == f ? t.v : 0u);
        }
        return v;
    }
    __device__ __forceinline__ bool held(uint32_t k) const { return !((bl[(bit0 + k) >> 5] >> ((bit0 + k) & 31u)) & 1u); }
};

struct StepFolder {
    using Expr = Fp;
    SaStep r;
    uint32_t k;
    bool det;
    __device__ __forceinline__ Fp constant(uint32_t v) const { return Fp::from_canonical(v); }
    __device__ __forceinline__ Fp main(int col, bool next) const { return r.load((uint32_t)col, next); }
    __device__ __forceinline__ Fp preprocessed(int col, bool next) const { return Fp::raw(r.plp[(uint32_t)col * r.S + (next ? 1u : 0u)]); }
    __device__ __forceinline__ Fp is_first_row() const { return r.first; }
    __device__ __forceinline__ Fp is_last_row() const { return r.last; }
    __device__ __forceinline__ Fp is_transition() const { return r.trans; }
    __device__ __forceinline__ void assert_zero(const Fp& e) { det = det || (!e.is_zero() && r.held(k)); k++; }
};

// Some constraint that held on M is non-zero on the moved row at this q.  regs: this lane's slot of the wave's register file (value halves).
template <int CHIP>
__device__ __forceinline__ bool sa_step_eval(const RaArgs& a, const SaStep& r, uint32_t* regs) {
    if (CHIP >= 0) {
        StepFolder f;
        f.r = r; f.k = 0; f.det = false;
        vchips::eval_chip(CHIP, f);
        return f.det;
    }
    uint32_t k = 0;
    bool det = false;
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: SA_V(in.dst) = (uint32_t)in.a | ((uint32_t)in.b << 16); break;
            case vair::OP_LOAD_MAIN: SA_V(in.dst) = r.load((uint32_t)in.a, in.flag != 0).v; break;
            case vair::OP_LOAD_PREP: SA_V(in.dst) = r.plp[(uint32_t)in.a * r.S + (in.flag ? 1u : 0u)]; break;
            case vair::OP_SEL_FIRST: SA_V(in.dst) = r.first.v; break;
            case vair::OP_SEL_LAST: SA_V(in.dst) = r.last.v; break;
            case vair::OP_SEL_TRANS: SA_V(in.dst) = r.trans.v; break;
            case vair::OP_ADD: { const uint32_t x = SA_V(in.a), y = SA_V(in.b); SA_V(in.dst) = (Fp::raw(x) + Fp::raw(y)).v; } break;
            case vair::OP_SUB: { const uint32_t x = SA_V(in.a), y = SA_V(in.b); SA_V(in.dst) = (Fp::raw(x) - Fp::raw(y)).v; } break;
            case vair::OP_MUL: { const uint32_t x = SA_V(in.a), y = SA_V(in.b); SA_V(in.dst) = (Fp::raw(x) * Fp::raw(y)).v; } break;
            case vair::OP_NEG: { const uint32_t x = SA_V(in.a); SA_V(in.dst) = (-Fp::raw(x)).v; } break;
            case vair::OP_ASSERT: det = det || (SA_V(in.a) != 0 && r.held(k)); k++; break;
            default: break;  // OP_NOP padding
        }
    }
    return det;
}
#undef SA_V

// The pass bits of the row's items into pb [24] (bit `item`: the move goes undetected).  Leaves W.nxt [i] = the i-th non-pivot column and
// W.irow [column] = its index among them.  Wave-uniform control flow.
template <int CHIP>
__device__ __forceinline__ void sa_steps(const SaArgs& sa, RaWave& W, const uint32_t* tm, const uint32_t* tp, uint32_t S, uint32_t j, uint64_t r, const uint32_t* bl, uint32_t* pb) {
    const RaArgs& a = sa.r;
    const uint32_t w = W.w, lane = W.lane, Sn = sa.n_steps;
    const Fp one = Fp::one(), zero = Fp::zero();
    uint32_t nu = 0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        const bool np = col < w && W.row_of[col] == RA_NONE;
        const unsigned long long m = ra_ballot(np, W.slot);
        const uint32_t idx = nu + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (np) { W.nxt[idx] = col; W.irow[col] = idx; }
        nu += (uint32_t)__builtin_popcountll(m);
    }
    ra_wave_sync();
    const uint32_t items = nu * Sn;
    const bool single_row = a.n == 1;
    for (uint32_t p = 0; p * 64u < items; p++) {
        const uint32_t item = p * 64u + lane;
        const bool has = item < items;
        const uint32_t i = has ? item / Sn : 0u, s = item - i * Sn;
        SaStep q;
        q.f = W.nxt[i];
        const uint32_t tv = s == 0 ? sa.steps[0] : s == 1 ? sa.steps[1] : s == 2 ? sa.steps[2] : sa.steps[3];  // selects: no indexed private array
        q.t = Fp::raw(has ? tv : 0u);
        q.S = S; q.BS = W.BS; q.row_of = W.row_of; q.basis = W.basis; q.bl = bl;
        bool det = false;
        for (uint32_t which = 0; which < (single_row ? 1u : 2u); which++) {
            const uint64_t qr = which ? ((r + a.n - 1) & (a.n - 1)) : r;
            const uint32_t off = which ? 0u : 1u;
            q.lp = tm + j + off; q.plp = tp + j + off;
            q.mv_local = which == 0; q.mv_next = which == 1 || single_row;
            q.first = qr == 0 ? one : zero; q.last = qr == a.n - 1 ? one : zero; q.trans = qr == a.n - 1 ? zero : one;
            q.bit0 = which * a.K;
            det = sa_step_eval<CHIP>(a, q, W.regs) || det;
        }
        const unsigned long long m = ra_ballot(has && !det, W.slot);
        if (lane == 0) { pb[2 * p] = (uint32_t)m; pb[2 * p + 1] = (uint32_t)(m >> 32); }
    }
    ra_wave_sync();
}

__host__ __device__ inline uint32_t sa_wave_words(uint32_t w, uint32_t K, uint32_t n_regs, bool interpret) {
    return ra_wave_words(w, K, n_regs, interpret) + SA_PASS_WORDS + (2u * K + 31u) / 32u;
}

// Workgroup x: rows [x T, x T + T).  mode MA_COUNT: totals (launch.hpp: SaArgs) and table[c * NB + x] = listable rows of column c; mode
// MA_LIST: rows[(c * R + rank) * 20 ..] = the rank-th listable row of column c < c_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_sa_audit(SaArgs sa, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                  uint32_t c_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t sa_lds[];
    const RaArgs& a = sa.r;
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6, w = a.width, T = a.T, S = (T + 2u) | 1u;
    const uint32_t Sn = sa.n_steps, ALL = (1u << Sn) - 1u;
    uint32_t* sums = sa_lds + 1;  // confirmed rows, refuted rows, passes of step 0..3
    uint32_t* cnt = sa_lds + 8;   // [5][w] loose, zero, exact, coupled-and-exact, listable rows of the column
    uint32_t* need = cnt + 5 * w;
    uint32_t* running = need + w;
    uint32_t* cb = running + w;   // [NW][w] the listable bits of the round's rows
    uint32_t* tm = cb + NW * w;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S + wave * sa_wave_words(w, a.K, a.n_regs, CHIP == CA_INTERPRET);
    RaWave W;
    W.w = w; W.BS = w | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.nzf = W.row_of + w; W.nxt = W.nzf + w; W.irow = W.nxt + w; W.basis = W.irow + w; W.raw = W.basis + w * W.BS;
    W.regs = W.raw + a.K * w + lane;
    uint32_t* pb = W.raw + a.K * w + (CHIP == CA_INTERPRET ? 128u * a.n_regs : 0u);
    uint32_t* bl = pb + SA_PASS_WORDS;
    for (uint32_t x = t; x < 8u + (7u + NW) * w; x += NT) sa_lds[x] = 0;
    __syncthreads();
    if (mode == MA_LIST) {
        for (uint32_t c = t; c < w && c < c_cut; c += NT)
            if (table[(uint64_t)c * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)c * a.NB + blockIdx.x] < R) { need[c] = 1; sa_lds[0] = 1; }
        __syncthreads();
        if (!sa_lds[0]) return;  // the whole workgroup
    }
    // the tile: word j of a column is row (base + j - 1) mod n, j = 0 .. rows_here + 1
    const uint64_t base = (uint64_t)blockIdx.x * T;
    const uint32_t rows_here = a.n - base < T ? (uint32_t)(a.n - base) : T;
    const uint32_t RJ = rows_here + 2;
    for (uint32_t x = t; x < w * RJ; x += NT) {
        const uint32_t col = x / RJ, j = x - col * RJ;
        tm[col * S + j] = a.main[(uint64_t)col * a.mstride + ((base + j + a.n - 1) & (a.n - 1))];
    }
    for (uint32_t x = t; x < a.prep_width * RJ; x += NT) {
        const uint32_t col = x / RJ, j = x - col * RJ;
        tp[col * S + j] = a.prep[(uint64_t)col * a.pstride + ((base + j + a.n - 1) & (a.n - 1))];
    }
    __syncthreads();

    // lz: bit q this lane's column of word q is loose, bit 3 + q it is zero; pm: bits [4 q, 4 q + 4) its pass mask.  A bus-only chip keeps
    // them, with the basis, across rows of equal live sets (rank_audit.hip).
    uint32_t live_prev = 0, lz = 0, pm = 0;
    bool have_prev = false;
    for (uint32_t i = 0; i < a.RPW; i++) {
        const uint32_t j = i * NW + wave;
        const uint64_t r = base + j;
        const bool active = j < rows_here;  // wave-uniform
        if (active) {
            bool reuse = false;
            if (CHIP == MA_BUS_ONLY && a.wr[0] <= 32u) {
                uint32_t live = 0;
                for (uint32_t m = 0; m < a.wr[0]; m++) {
                    uint32_t pos = a.iw[2 + m] + 2;
                    live |= ra_vcol(a.iw, pos, tm + j + 1, tp + j + 1, S).is_zero() ? 0u : 1u << m;
                }
                reuse = have_prev && live == live_prev;
                live_prev = live; have_prev = true;
            }
            if (!reuse) {
                sa_row<CHIP>(a, W, tm, tp, S, j, r, bl);
                if (CHIP != MA_BUS_ONLY && W.rho != w) sa_steps<CHIP>(sa, W, tm, tp, S, j, r, bl, pb);
                lz = 0; pm = 0;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const uint32_t col = lane + 64u * (uint32_t)q;
                    if (col >= w || W.rho == w) continue;
                    // the non-pivot column whose vector this column takes: itself, or the first other entry of its reduced basis row (the
                    // other pivot columns are zero there); none: pinned
                    uint32_t f = col;
                    if (W.row_of[col] != RA_NONE) {
                        const uint32_t* b = W.basis + col * W.BS;
                        f = RA_NONE;
                        for (uint32_t k = 0; k < w; k++) f = (f == RA_NONE && k != col && b[k] != 0) ? k : f;
                    }
                    if (f == RA_NONE) continue;
                    uint32_t mask = ALL;
                    if (CHIP != MA_BUS_ONLY) {
                        const uint32_t it0 = W.irow[f] * Sn;
                        mask = 0;
                        for (uint32_t s = 0; s < Sn; s++) mask |= ((pb[(it0 + s) >> 5] >> ((it0 + s) & 31u)) & 1u) << s;
                    }
                    lz |= (1u << q) | (W.nzf[col] == 0 ? 8u << q : 0u);
                    pm |= mask << (4 * q);
                }
            }
            bool confirmed = false, refuted = false;
            uint32_t pass_here[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t col = lane + 64u * (uint32_t)q;
                const bool loose = col < w && ((lz >> q) & 1u), zero = (lz >> (3 + q)) & 1u;
                const uint32_t mask = (pm >> (4 * q)) & 15u;
                const bool exact = loose && mask == ALL, listable = loose && (!zero || !exact);
                if (mode == MA_COUNT) {
                    if (loose) atomicAdd(&cnt[col], 1u);
                    if (loose && zero) atomicAdd(&cnt[w + col], 1u);
                    if (exact) atomicAdd(&cnt[2 * w + col], 1u);
                    if (exact && !zero) atomicAdd(&cnt[3 * w + col], 1u);
                    if (listable) atomicAdd(&cnt[4 * w + col], 1u);
                    if ((uint32_t)q < W.WPL) {  // wave-uniform
                        confirmed = confirmed || ra_ballot(exact && !zero, W.slot) != 0;
                        refuted = refuted || ra_ballot(loose && !exact, W.slot) != 0;
#pragma unroll
                        for (int s = 0; s < 4; s++)
                            if ((uint32_t)s < Sn) pass_here[s] += (uint32_t)__builtin_popcountll(ra_ballot(loose && ((mask >> s) & 1u), W.slot));
                    }
                } else if (col < w) {
                    cb[wave * w + col] = listable ? 1u : 0u;
                }
            }
            if (mode == MA_COUNT && lane == 0) {
                if (confirmed) atomicAdd(&sums[0], 1u);
                if (refuted) atomicAdd(&sums[1], 1u);
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if (pass_here[s]) atomicAdd(&sums[2 + s], pass_here[s]);
            }
        } else if (mode == MA_LIST) {
            for (uint32_t col = lane; col < w; col += 64u) cb[wave * w + col] = 0;
        }
        if (mode != MA_LIST) continue;
        __syncthreads();
        if (active) {
            // the pass mask and zero flag of every column where lane 0 finds them when it writes a listed row
            ra_wave_sync();
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t col = lane + 64u * (uint32_t)q;
                if (col < w) W.irow[col] = ((pm >> (4 * q)) & 15u) | (((lz >> (3 + q)) & 1u) << 8);
            }
            ra_wave_sync();
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t col = lane + 64u * (uint32_t)q;
                bool e = col < w && col < c_cut && need[col] != 0 && cb[wave * w + col] != 0;
                if (e) {
                    uint32_t rank = prefix[(uint64_t)col * a.NB + blockIdx.x] + running[col];
                    for (uint32_t k = 0; k < wave; k++) rank += cb[k * w + col];
                    e = rank < R;
                    W.nxt[col] = rank;
                }
                const unsigned long long m = ra_ballot(e, W.slot);
                ra_wave_sync();
                RA_EACH_BIT(m, q, c, {
                    uint32_t* out = rows + ((uint64_t)c * R + W.nxt[c]) * SA_OUT_WORDS;
                    ra_emit(W, c, (uint32_t)r, out + 2);  // row, n_support, terms at words 2 .. 19; lane 0 then puts the row's head over words 0 .. 2
                    if (lane == 0) { out[0] = (uint32_t)r; out[1] = W.irow[c] & 15u; out[2] = W.irow[c] >> 8; }
                })
            }
        }
        __syncthreads();
        if (wave == 0)
            for (uint32_t c = lane; c < w; c += 64u) {
                uint32_t s = 0;
                for (uint32_t k = 0; k < NW; k++) s += cb[k * w + c];
                running[c] += s;
            }
        __syncthreads();
    }
    if (mode != MA_COUNT) return;
    __syncthreads();
    for (uint32_t c = t; c < w; c += NT) {
#pragma unroll
        for (uint32_t x = 0; x < 4; x++)
            if (cnt[x * w + c]) atomicAdd(&totals[6 + 4 * c + x], (unsigned long long)cnt[x * w + c]);
        if (cnt[4 * w + c]) table[(uint64_t)c * a.NB + blockIdx.x] = cnt[4 * w + c];
    }
    if (t < 6 && sums[t]) atomicAdd(&totals[t], (unsigned long long)sums[t]);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t sa_lds_bytes(const SaArgs& sa, uint32_t NW, uint32_t T) {
    const RaArgs& a = sa.r;
    const size_t S = (T + 2u) | 1u;
    return 4 * (8 + (size_t)(7 + NW) * a.width + ((size_t)a.width + a.prep_width) * S + (size_t)NW * sa_wave_words(a.width, a.K, a.n_regs, a.native_chip == CA_INTERPRET));
}

void sa_shape(SaArgs& sa) {
    RaArgs& a = sa.r;
    const size_t LDS = 160 * 1024;
    if (a.width > 192 || sa_lds_bytes(sa, 1, 1) > LDS)
        throw std::invalid_argument("step_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints and " +
                                    std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) + " interpreted registers does not fit a workgroup's LDS with one wave (" +
                                    std::to_string(sa_lds_bytes(sa, 1, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + 128 per register + 12 w + 36 + ceil(2 K / 32) + 3 (w + prep w)), 163840 at most; at most 192 columns)");
    // the most waves per CU; among equals the larger workgroup (fewer tiles staged): rank_audit.hip's rule
    uint32_t best = 1, best_waves = 0;
    for (uint32_t nw = 4; nw >= 1; nw >>= 1) {
        uint32_t rpw = 16;
        while (rpw > 1 && (a.n / ((uint64_t)nw * rpw) < 1024 || sa_lds_bytes(sa, nw, nw * rpw) > LDS)) rpw >>= 1;
        const size_t b = sa_lds_bytes(sa, nw, nw * rpw);
        if (b > LDS) continue;
        const uint32_t waves = (uint32_t)(LDS / b) * nw;
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    a.NW = best;
    uint32_t rpw = 16;
    while (rpw > 1 && (a.n / ((uint64_t)a.NW * rpw) < 1024 || sa_lds_bytes(sa, a.NW, a.NW * rpw) > LDS)) rpw >>= 1;
    a.RPW = rpw;
    a.T = a.NW * a.RPW;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define SA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void sa_check(const SaArgs& sa) {
    const RaArgs& a = sa.r;
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("step_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > 192) throw std::logic_error("step_audit: 1 to 192 columns");
    if (sa.n_steps == 0 || sa.n_steps > 4) throw std::logic_error("step_audit: 1 to 4 steps");
    if (a.n == 0 || (a.n & (a.n - 1)) || (a.NW != 1 && a.NW != 2 && a.NW != 4) || a.RPW == 0 || a.T != a.NW * a.RPW || a.NB != (uint32_t)((a.n + a.T - 1) / a.T))
        throw std::logic_error("step_audit: inconsistent launch shape");
    if (sa_lds_bytes(sa, a.NW, a.T) > 160 * 1024) throw std::logic_error("step_audit: the launch shape does not fit the LDS");
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has the opt-in to more than 64 KB of dynamic LDS
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("step_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("step_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) + ": " +
                                     hipGetErrorString(e));
    };
#define SA_X(C) opt_in((const void*)k_sa_audit<vchips::C>, "k_sa_audit<" #C ">");
    SA_CHIPS(SA_X)
#undef SA_X
    opt_in((const void*)k_sa_audit<CA_INTERPRET>, "k_sa_audit<CA_INTERPRET>");
    opt_in((const void*)k_sa_audit<MA_BUS_ONLY>, "k_sa_audit<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

static void sa_launch(hipStream_t st, const SaArgs& sa, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows) {
    const RaArgs& a = sa.r;
    const dim3 grid(a.NB), block(64 * a.NW);
    const size_t lds = sa_lds_bytes(sa, a.NW, a.T);
    switch (a.native_chip) {
#define SA_X(C) case vchips::C: VK_LAUNCH((k_sa_audit<vchips::C>), grid, block, lds, st, sa, mode, totals, table, prefix, c_cut, R, rows); break;
        SA_CHIPS(SA_X)
#undef SA_X
        case CA_INTERPRET: VK_LAUNCH((k_sa_audit<CA_INTERPRET>), grid, block, lds, st, sa, mode, totals, table, prefix, c_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_sa_audit<MA_BUS_ONLY>), grid, block, lds, st, sa, mode, totals, table, prefix, c_cut, R, rows); break;
        default: throw std::logic_error("step_audit: a native chip id without constraints");
    }
}

void launch_sa_count(hipStream_t st, const SaArgs& sa, unsigned long long* totals, uint32_t* table) {
    sa_check(sa);
    static const char* names[14] = {"k_sa_count.cpu", "k_sa_count.program", "k_sa_count.mem", "k_sa_count.add", "k_sa_count.sub", "k_sa_count.mul", "k_sa_count.div", "k_sa_count.shift",
                                    "k_sa_count.lt", "k_sa_count.com", "k_sa_count.bitwise", "k_sa_count.output", "k_sa_count.range", "k_sa_count.static_data"};
    const int id = sa.r.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_sa_count.bus" : "k_sa_count");
    ProfScope ps(name, st, 4.0 * (double)sa.r.n * (sa.r.width + sa.r.prep_width), sa.r.evaluations);
    sa_launch(st, sa, MA_COUNT, totals, table, nullptr, 0, 0, nullptr);
}

void launch_sa_list(hipStream_t st, const SaArgs& sa, const uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows) {
    sa_check(sa);
    ProfScope ps("k_sa_list", st, 0);
    sa_launch(st, sa, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, c_cut, R, rows);
}

}  // namespace vk
