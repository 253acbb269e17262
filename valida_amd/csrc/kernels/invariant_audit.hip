// Invariant audit on the device (host/invariant_audit.hpp states the contract): per chip the affine-linear relations every row of the trace
// keeps, and per relation the rows on which the rank audit's Jacobian enforces it.
//   basis    phase 1, k_ia_basis: workgroup x (ONE wave) takes the RB consecutive rows [x RB, x RB + RB) of the working layout (column-major
//            Montgomery) as augmented rows (1, M[r][0], .., M[r][w - 1]), AW = w + 1 columns, lane l <-> columns l, l + 64, l + 128, and
//            keeps a REDUCED basis of at most AW rows in LDS as [AW][BS], BS = AW | 1 (the row of pivot column p is row p): rank_elim.hpp's
//            ra_insert, the very function — a new row is reduced in one sweep (every coefficient read before any update), a pivot is added
//            only when something is left, and once rho = AW the workgroup stops.  Rows are staged 32 at a time as [32][BS]: the global
//            reads are 128-byte runs of one column, the LDS writes of 32 lanes go to 32 different banks (odd row stride), and the row ra_insert
//            reads is contiguous.  The workgroup writes its pivot flags and basis rows to part.
//   merge    k_ia_merge: a second elimination of the workgroups' basis rows into one basis, as a tree of fan 16 (every workgroup of a level,
//            one wave, eliminates up to 16 partial bases into one; the last level is one workgroup) — the RREF of the whole matrix whatever
//            the grid and the tree were (it is unique) — then rho, d, the pivot flags and, per non-pivot column f ascending, the canonical
//            vector l_f = 1, l_p = -basis[p][f] for the pivot columns p, 0 elsewhere, written to inv.
//   enforce  phase 2, k_ia_enforce<CHIP>: rank_audit.hip's shape — one wave per trace row, NW waves per workgroup, RPW rows per wave, the tile
//            [column][S] with halo and wrap, ra_row<CHIP> (the rank audit's dual evaluation and LDS elimination, unchanged; a chip without
//            constraints keeps the basis while its live set is unchanged).  The d invariants c_i = (l_1 .. l_w) are staged in LDS once per
//            workgroup; per row and invariant one reduce-only sweep against the row's reduced basis: ballot of the pivot lanes where c_i is
//            non-zero, per hit one LDS broadcast of the coefficient and one multiply-subtract per lane; enforced iff nothing is left
//            (one ballot).  rho = w: everything is enforced, no sweep.  The verdicts of a row are three wave-uniform 64-bit masks.
//   count    lane i & 63 counts the free rows of invariant i in a register; at the end of the workgroup's rows LDS atomics, then one integer
//            atomic per workgroup and invariant on the chip's totals; the count also goes into table[i][workgroup].
//   scan     the rank audit's k_ra_scan over table rows (launch_ra_scan).
//   list     workgroups that hold a free row of rank < R of a listed invariant run their rows again; the waves of a round exchange their
//            free bits through LDS so that rank = prefix + rows before in the workgroup; the owning lane writes the row.  No atomic admits a row.
// LDS (u32 words): phase 1 and merge: 8 + 3 AW + AW BS + 32 BS.  Phase 2: 8 + (3 + NW) d + d w (counters, need, running, free bits, the
// invariants) + (w + prep w) S (tile) + per wave the rank audit's words — and never less than the rank audit's own bytes for the same shape
// (ia_lds_bytes): the shape must also pass launch_ra_scan's check.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, w <= 191 so AW <= 192 =
// 3 x 64 lane words, d <= w, rows written by `list` have ranks below R and invariants below i_cut <= d).
#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include "rank_elim.hpp"

namespace vk {

__host__ __device__ inline uint32_t ia_basis_words(uint32_t AW) { return 8u + 3u * AW + AW * (AW | 1u) + IA_TILE_ROWS * (AW | 1u); }

// the wave's elimination state over AW augmented columns in lds: slot, row_of, nzf, nxt, basis (irow, raw, regs are not used by ra_insert)
__device__ __forceinline__ RaWave ia_wave(uint32_t* lds, uint32_t AW, uint32_t lane) {
    RaWave W;
    W.w = AW; W.BS = AW | 1u; W.WPL = (AW + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = lds; W.row_of = lds + 8; W.nzf = W.row_of + AW; W.nxt = W.nzf + AW; W.basis = W.nxt + AW;
    W.irow = nullptr; W.raw = nullptr; W.regs = nullptr;
    for (uint32_t c = lane; c < AW; c += 64u) { W.row_of[c] = RA_NONE; W.nzf[c] = 0; }
    ra_wave_sync();
    return W;
}

// Workgroup x (64 threads): the reduced basis of the augmented rows [x RB, min(n, x RB + RB)) -> part + x AW (AW + 1): AW pivot flags, then
// row p of [AW][AW] for every pivot column p.
__global__ void __launch_bounds__(64) k_ia_basis(const uint32_t* __restrict__ main, uint64_t mstride, uint64_t n, uint32_t w, uint32_t RB, uint32_t* __restrict__ part) {
    extern __shared__ uint32_t ia_lds[];
    const uint32_t lane = threadIdx.x, AW = w + 1u, BS = AW | 1u;
    RaWave W = ia_wave(ia_lds, AW, lane);
    uint32_t* tile = W.basis + AW * BS;  // [32][BS]
    const uint64_t base = (uint64_t)blockIdx.x * RB, end = base + RB < n ? base + RB : n;
    for (uint64_t t0 = base; t0 < end && W.rho < AW; t0 += IA_TILE_ROWS) {
        const uint32_t rows = end - t0 < IA_TILE_ROWS ? (uint32_t)(end - t0) : IA_TILE_ROWS;
        for (uint32_t x = lane; x < AW * IA_TILE_ROWS; x += 64u) {
            const uint32_t col = x / IA_TILE_ROWS, j = x % IA_TILE_ROWS;
            if (j < rows) tile[j * BS + col] = col ? main[(uint64_t)(col - 1u) * mstride + t0 + j] : vg::R_MOD_P;
        }
        ra_wave_sync();
        for (uint32_t j = 0; j < rows && W.rho < AW; j++) ra_insert(W, tile + j * BS);
        ra_wave_sync();
    }
    uint32_t* out = part + (uint64_t)blockIdx.x * AW * (AW + 1u);
    for (uint32_t c = lane; c < AW; c += 64u) out[c] = W.row_of[c] != RA_NONE ? 1u : 0u;
    for (uint32_t p = 0; p < AW; p++) {
        if (W.row_of[p] == RA_NONE) continue;  // wave-uniform
        for (uint32_t c = lane; c < AW; c += 64u) out[AW + (uint64_t)p * AW + c] = W.basis[p * BS + c];
    }
}

// Workgroup x (64 threads) eliminates the partial bases [x fan, min(n_parts, x fan + fan)) of `part` into one.  out_part != null: written as a
// partial basis at out_part + x AW (AW + 1) (a level of the tree); otherwise (one workgroup) inv as launch.hpp (IaArgs) describes it.
__global__ void __launch_bounds__(64) k_ia_merge(const uint32_t* __restrict__ part, uint32_t n_parts, uint32_t fan, uint32_t w, uint32_t* __restrict__ out_part, uint32_t* __restrict__ inv) {
    extern __shared__ uint32_t ia_lds[];
    const uint32_t lane = threadIdx.x, AW = w + 1u, BS = AW | 1u;
    RaWave W = ia_wave(ia_lds, AW, lane);
    uint32_t* cur = W.basis + AW * BS;  // [AW]
    const uint32_t g0 = blockIdx.x * fan, g1 = n_parts - g0 < fan ? n_parts : g0 + fan;
    for (uint32_t g = g0; g < g1 && W.rho < AW; g++) {
        const uint32_t* in = part + (uint64_t)g * AW * (AW + 1u);
        for (uint32_t p = 0; p < AW && W.rho < AW; p++) {
            if (!in[p]) continue;  // wave-uniform
            for (uint32_t c = lane; c < AW; c += 64u) cur[c] = in[AW + (uint64_t)p * AW + c];
            ra_wave_sync();
            ra_insert(W, cur);
            ra_wave_sync();
        }
    }
    if (out_part) {
        uint32_t* out = out_part + (uint64_t)blockIdx.x * AW * (AW + 1u);
        for (uint32_t c = lane; c < AW; c += 64u) out[c] = W.row_of[c] != RA_NONE ? 1u : 0u;
        for (uint32_t p = 0; p < AW; p++) {
            if (W.row_of[p] == RA_NONE) continue;  // wave-uniform
            for (uint32_t c = lane; c < AW; c += 64u) out[AW + (uint64_t)p * AW + c] = W.basis[p * BS + c];
        }
        return;
    }
    if (lane == 0) { inv[0] = W.rho; inv[1] = AW - W.rho; }
    for (uint32_t c = lane; c < AW; c += 64u) inv[2 + c] = W.row_of[c] != RA_NONE ? 1u : 0u;
    uint32_t i = 0;
    for (uint32_t f = 0; f < AW; f++) {
        if (W.row_of[f] != RA_NONE) continue;  // wave-uniform
        uint32_t* out = inv + 2 + AW + (uint64_t)i * AW;
        for (uint32_t c = lane; c < AW; c += 64u) {
            Fp v = Fp::zero();
            if (c == f) v = Fp::one();
            else if (W.row_of[c] != RA_NONE) v = -Fp::raw(W.basis[c * BS + f]);
            out[c] = v.v;
        }
        i++;
    }
}

// Is invariant c [w] (LDS) outside the row space of the wave's reduced basis?  Wave-uniform.
__device__ __forceinline__ bool ia_free(RaWave& W, const uint32_t* c) {
    const uint32_t w = W.w, BS = W.BS, lane = W.lane;
    unsigned long long hit[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t col = lane + 64u * (uint32_t)q;
        hit[q] = ra_ballot(col < w && W.row_of[col] != RA_NONE && c[col] != 0, W.slot);
    }
    bool left = false;
    for (uint32_t wd = 0; wd < W.WPL; wd++) {
        const uint32_t col = lane + 64u * wd;
        if (col >= w) continue;
        Fp acc = Fp::raw(c[col]);
#pragma unroll
        for (int q = 0; q < 3; q++) RA_EACH_BIT(hit[q], q, p, acc -= Fp::raw(c[p]) * Fp::raw(W.basis[p * BS + col]);)
        left |= !acc.is_zero();
    }
    return ra_ballot(left, W.slot) != 0;
}

// Workgroup x: rows [x T, x T + T).  mode MA_COUNT: totals[i] += free rows of invariant i, table[i * NB + x] = the same; mode MA_LIST:
// rows[i * R + rank] = the rank-th free row of invariant i < i_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_ia_enforce(IaArgs ia, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                    uint32_t i_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t ia_lds[];
    const RaArgs& a = ia.r;
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6, w = a.width, d = ia.d, T = a.T, S = (T + 2u) | 1u, AW = w + 1u;
    uint32_t* cnt = ia_lds + 8;  // [d] free rows of the invariant
    uint32_t* need = cnt + d;
    uint32_t* running = need + d;
    uint32_t* cb = running + d;  // [NW][d] the free bits of the round's rows
    uint32_t* vecs = cb + NW * d;  // [d][w]
    uint32_t* tm = vecs + d * w;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S + wave * ra_wave_words(w, a.K, a.n_regs, CHIP == CA_INTERPRET);
    RaWave W;
    W.w = w; W.BS = w | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.nzf = W.row_of + w; W.nxt = W.nzf + w; W.irow = W.nxt + w; W.basis = W.irow + w; W.raw = W.basis + w * W.BS;
    W.regs = W.raw + a.K * w + lane;
    for (uint32_t x = t; x < 8u + (3u + NW) * d; x += NT) ia_lds[x] = 0;
    __syncthreads();
    if (mode == MA_LIST) {
        for (uint32_t i = t; i < d && i < i_cut; i += NT)
            if (table[(uint64_t)i * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)i * a.NB + blockIdx.x] < R) { need[i] = 1; ia_lds[0] = 1; }
        __syncthreads();
        if (!ia_lds[0]) return;  // the whole workgroup
    }
    for (uint32_t x = t; x < d * w; x += NT) {
        const uint32_t i = x / w, col = x - i * w;
        vecs[x] = ia.vec[(uint64_t)i * AW + 1u + col];
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

    uint32_t live_prev = 0;
    bool have_prev = false;
    unsigned long long fb[3] = {0, 0, 0};  // bit l of fb[q]: invariant l + 64 q is free at the wave's row (wave-uniform)
    uint32_t mine[3] = {0, 0, 0};          // this lane's invariants' free rows so far
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
                ra_row<CHIP>(a, W, tm, tp, S, j, r);
                fb[0] = fb[1] = fb[2] = 0;
                if (W.rho != w)
                    for (uint32_t k = 0; k < d; k++)
                        if (ia_free(W, vecs + k * w)) fb[k >> 6] |= 1ull << (k & 63u);
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t k = lane + 64u * (uint32_t)q;
                if (k >= d) continue;
                const uint32_t bit = (uint32_t)(fb[q] >> lane) & 1u;
                if (mode == MA_COUNT) mine[q] += bit;
                else cb[wave * d + k] = bit;
            }
        } else if (mode == MA_LIST) {
            for (uint32_t k = lane; k < d; k += 64u) cb[wave * d + k] = 0;
        }
        if (mode != MA_LIST) continue;
        __syncthreads();
        if (active) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t k = lane + 64u * (uint32_t)q;
                if (k < d && k < i_cut && need[k] != 0 && cb[wave * d + k] != 0) {
                    uint32_t rank = prefix[(uint64_t)k * a.NB + blockIdx.x] + running[k];
                    for (uint32_t x = 0; x < wave; x++) rank += cb[x * d + k];
                    if (rank < R) rows[(uint64_t)k * R + rank] = (uint32_t)r;
                }
            }
        }
        __syncthreads();
        if (wave == 0)
            for (uint32_t k = lane; k < d; k += 64u) {
                uint32_t s = 0;
                for (uint32_t x = 0; x < NW; x++) s += cb[x * d + k];
                running[k] += s;
            }
        __syncthreads();
    }
    if (mode != MA_COUNT) return;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t k = lane + 64u * (uint32_t)q;
        if (k < d && mine[q]) atomicAdd(&cnt[k], mine[q]);
    }
    __syncthreads();
    for (uint32_t k = t; k < d; k += NT) {
        if (!cnt[k]) continue;
        atomicAdd(&totals[k], (unsigned long long)cnt[k]);
        table[(uint64_t)k * a.NB + blockIdx.x] = cnt[k];
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t ia_basis_lds_bytes(uint32_t width) { return 4 * (size_t)ia_basis_words(width + 1u); }

void ia_basis_shape(IaArgs& ia) {
    const RaArgs& a = ia.r;
    const size_t LDS = 160 * 1024;
    if (a.width > IA_MAX_WIDTH || ia_basis_lds_bytes(a.width) > LDS)
        throw std::invalid_argument("invariant_audit: the basis of a chip of " + std::to_string(a.width) + " columns does not fit a workgroup's LDS (" + std::to_string(ia_basis_lds_bytes(a.width)) +
                                    " bytes: 4 x ((w + 1) ((w + 1) | 1) + 3 (w + 1) + 32 ((w + 1) | 1) + 8), 163840 at most; at most 191 columns: one lane per augmented column, three words per lane)");
    // workgroups of whole tiles of rows: at most IA_MAX_WORKGROUPS, and no more than 64 MB of partial bases
    const uint64_t slot = (a.width + 1ull) * (a.width + 2ull);
    const uint64_t most = std::min<uint64_t>(IA_MAX_WORKGROUPS, std::max<uint64_t>(1, (1ull << 24) / slot));
    const uint64_t tiles = (a.n + IA_TILE_ROWS - 1) / IA_TILE_ROWS;
    const uint64_t per = (tiles + most - 1) / most;
    ia.RB = (uint32_t)(per * IA_TILE_ROWS);
    ia.NB1 = (uint32_t)((a.n + ia.RB - 1) / ia.RB);
}

size_t ia_lds_bytes(const IaArgs& ia, uint32_t NW, uint32_t T) {
    const RaArgs& a = ia.r;
    const size_t S = (T + 2u) | 1u;
    const size_t own = 4 * (8 + (size_t)(3 + NW) * ia.d + (size_t)ia.d * a.width + ((size_t)a.width + a.prep_width) * S +
                            (size_t)NW * ra_wave_words(a.width, a.K, a.n_regs, a.native_chip == CA_INTERPRET));
    // never less than the rank audit's bytes for the same shape: the listing pass goes through launch_ra_scan, which checks those, and with few
    // invariants this audit's (3 + NW + w) d words are fewer than the rank audit's (5 + NW) w.  The kernels are launched with the larger figure.
    return std::max(own, ra_lds_bytes(a, NW, T));
}

void ia_shape(IaArgs& ia) {
    RaArgs& a = ia.r;
    const size_t LDS = 160 * 1024;
    if (a.width > IA_MAX_WIDTH || ia.d > a.width || ia_lds_bytes(ia, 1, 1) > LDS)
        throw std::invalid_argument("invariant_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints, " +
                                    std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) + " interpreted registers and " + std::to_string(ia.d) +
                                    " invariants does not fit a workgroup's LDS with one wave (" + std::to_string(ia_lds_bytes(ia, 1, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + 128 per register + 4 w + 12 + 3 (w + prep w) + the larger of d (w + 4) and 6 w, the rank audit's counters, whose scan lists the rows), 163840 at most, d = w counted before the invariants are known; at most 191 columns)");
    // the most waves per CU; among equals the larger workgroup (fewer tiles staged): rank_audit.hip's rule
    uint32_t best = 1, best_waves = 0;
    for (uint32_t nw = 4; nw >= 1; nw >>= 1) {
        uint32_t rpw = 16;
        while (rpw > 1 && (a.n / ((uint64_t)nw * rpw) < 1024 || ia_lds_bytes(ia, nw, nw * rpw) > LDS)) rpw >>= 1;
        const size_t b = ia_lds_bytes(ia, nw, nw * rpw);
        if (b > LDS) continue;
        const uint32_t waves = (uint32_t)(LDS / b) * nw;
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    a.NW = best;
    uint32_t rpw = 16;
    while (rpw > 1 && (a.n / ((uint64_t)a.NW * rpw) < 1024 || ia_lds_bytes(ia, a.NW, a.NW * rpw) > LDS)) rpw >>= 1;
    a.RPW = rpw;
    a.T = a.NW * a.RPW;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define IA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

// the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
static void ia_opt_in() {
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("invariant_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("invariant_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) +
                                     ": " + hipGetErrorString(e));
    };
    opt_in((const void*)k_ia_basis, "k_ia_basis");
    opt_in((const void*)k_ia_merge, "k_ia_merge");
#define IA_X(C) opt_in((const void*)k_ia_enforce<vchips::C>, "k_ia_enforce<" #C ">");
    IA_CHIPS(IA_X)
#undef IA_X
    opt_in((const void*)k_ia_enforce<CA_INTERPRET>, "k_ia_enforce<CA_INTERPRET>");
    opt_in((const void*)k_ia_enforce<MA_BUS_ONLY>, "k_ia_enforce<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

static void ia_basis_check(const IaArgs& ia) {
    const RaArgs& a = ia.r;
    if (a.width == 0 || a.width > IA_MAX_WIDTH) throw std::logic_error("invariant_audit: 1 to 191 columns");
    // the kernels take any slice length and any number of workgroups; whole tiles and IA_MAX_WORKGROUPS are ia_basis_shape's choice
    if (a.n == 0 || ia.RB == 0 || ia.NB1 == 0 || ia.NB1 != (uint32_t)((a.n + ia.RB - 1) / ia.RB))
        throw std::logic_error("invariant_audit: inconsistent basis launch shape");
    if (ia_basis_lds_bytes(a.width) > 160 * 1024) throw std::logic_error("invariant_audit: the basis does not fit the LDS");
    ia_opt_in();
}

void launch_ia_basis(hipStream_t st, const IaArgs& ia, uint32_t* part) {
    ia_basis_check(ia);
    ProfScope ps("k_ia_basis", st, 4.0 * (double)ia.r.n * ia.r.width);
    VK_LAUNCH(k_ia_basis, dim3(ia.NB1), dim3(64), ia_basis_lds_bytes(ia.r.width), st, ia.r.main, ia.r.mstride, ia.r.n, ia.r.width, ia.RB, part);
}

void launch_ia_merge(hipStream_t st, const IaArgs& ia, uint32_t* part, uint32_t* inv) {
    ia_basis_check(ia);
    ProfScope ps("k_ia_merge", st, 4.0 * (double)ia_part_words(ia));
    // a tree of fan IA_MERGE_FAN: the levels ping-pong between the workgroups' slots and the spare slots behind them (launch.hpp: ia_part_words)
    const uint64_t slot = (ia.r.width + 1ull) * (ia.r.width + 2ull);
    uint32_t *src = part, *dst = part + (uint64_t)ia.NB1 * slot;
    uint32_t n = ia.NB1;
    while (n > IA_MERGE_FAN) {
        const uint32_t m = (n + IA_MERGE_FAN - 1) / IA_MERGE_FAN;
        VK_LAUNCH(k_ia_merge, dim3(m), dim3(64), ia_basis_lds_bytes(ia.r.width), st, src, n, IA_MERGE_FAN, ia.r.width, dst, nullptr);
        std::swap(src, dst);
        n = m;
    }
    VK_LAUNCH(k_ia_merge, dim3(1), dim3(64), ia_basis_lds_bytes(ia.r.width), st, src, n, IA_MERGE_FAN, ia.r.width, nullptr, inv);
}

static void ia_check(const IaArgs& ia) {
    const RaArgs& a = ia.r;
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("invariant_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > IA_MAX_WIDTH || ia.d == 0 || ia.d > a.width || !ia.vec) throw std::logic_error("invariant_audit: 1 to 191 columns and 1 to w invariants");
    if (a.n == 0 || (a.n & (a.n - 1)) || (a.NW != 1 && a.NW != 2 && a.NW != 4) || a.RPW == 0 || a.T != a.NW * a.RPW || a.NB != (uint32_t)((a.n + a.T - 1) / a.T))
        throw std::logic_error("invariant_audit: inconsistent launch shape");
    if (ia_lds_bytes(ia, a.NW, a.T) > 160 * 1024) throw std::logic_error("invariant_audit: the launch shape does not fit the LDS");
    ia_opt_in();
}

static void ia_launch(hipStream_t st, const IaArgs& ia, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows) {
    const RaArgs& a = ia.r;
    const dim3 grid(a.NB), block(64 * a.NW);
    const size_t lds = ia_lds_bytes(ia, a.NW, a.T);
    switch (a.native_chip) {
#define IA_X(C) case vchips::C: VK_LAUNCH((k_ia_enforce<vchips::C>), grid, block, lds, st, ia, mode, totals, table, prefix, i_cut, R, rows); break;
        IA_CHIPS(IA_X)
#undef IA_X
        case CA_INTERPRET: VK_LAUNCH((k_ia_enforce<CA_INTERPRET>), grid, block, lds, st, ia, mode, totals, table, prefix, i_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_ia_enforce<MA_BUS_ONLY>), grid, block, lds, st, ia, mode, totals, table, prefix, i_cut, R, rows); break;
        default: throw std::logic_error("invariant_audit: a native chip id without constraints");
    }
}

void launch_ia_count(hipStream_t st, const IaArgs& ia, unsigned long long* totals, uint32_t* table) {
    ia_check(ia);
    static const char* names[14] = {"k_ia_count.cpu", "k_ia_count.program", "k_ia_count.mem", "k_ia_count.add", "k_ia_count.sub", "k_ia_count.mul", "k_ia_count.div", "k_ia_count.shift",
                                    "k_ia_count.lt", "k_ia_count.com", "k_ia_count.bitwise", "k_ia_count.output", "k_ia_count.range", "k_ia_count.static_data"};
    const int id = ia.r.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_ia_count.bus" : "k_ia_count");
    ProfScope ps(name, st, 4.0 * (double)ia.r.n * (ia.r.width + ia.r.prep_width), ia.r.evaluations);
    ia_launch(st, ia, MA_COUNT, totals, table, nullptr, 0, 0, nullptr);
}

void launch_ia_list(hipStream_t st, const IaArgs& ia, const uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows) {
    ia_check(ia);
    ProfScope ps("k_ia_list", st, 0);
    ia_launch(st, ia, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, i_cut, R, rows);
}

}  // namespace vk
