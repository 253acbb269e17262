// Transition audit on the device (host/transition_audit.hpp states the contract): per chip and gate the affine-linear relations every gated
// two-row window of the trace keeps, and per listed relation the windows at which the rank audit's Jacobian does not hold it.
//   flags    k_ta_flags: per main column the class of every value (0, 1, something else) over the rows 0 .. n - 2 (the column as `local`) and over
//            1 .. n - 1 (as `next`): a workgroup walks TA_BOOL_ROWS rows of every column; the three flags of each role are reduced per wave by
//            ballots, the windows on which the column is 1 by the popcount of a ballot, then one OR and one integer add per workgroup and column.
//   basis    phase 1, k_ta_basis: the invariant audit's shape (one wave per slice, lane l <-> window columns l, l + 64, l + 128, a REDUCED basis of
//            at most AW rows in LDS as [AW][AW], rank_elim.hpp's ra_insert, the very function) with three differences: the tile stages
//            TA_TILE_WINDOWS + 1 trace rows once as [row][w | 1] and serves each as `local` of window r and `next` of window r - 1 (the slice's last
//            window reads the first row of the following slice); gates run over gridDim.y; a wave skips the windows where its gate is false
//            (one LDS word, wave-uniform) and stops at full rank.  The window's row is gathered into `cur` (contiguous, as ra_insert reads it).
//   merge    k_ta_merge: invariant_audit.hip's k_ia_merge as a kernel of this audit's own (that file is not edited and its kernel takes one
//            basis): the same elimination of partial bases by a tree of fan 16, gates over gridDim.y, and the same final image per gate.
//   enforce  phase 2, k_ta_enforce<CHIP>: rank_audit.hip's shape (one wave per trace row, the tile [column][S] with halo and wrap, ra_row<CHIP>
//            unchanged).  The listed entries' vectors are staged in LDS, EC at a time (once per workgroup when they all fit, otherwise per
//            round of rows and chunk).  Per row r and entry up to two reduce-only sweeps against the row's reduced basis: the `local` part when
//            window r exists and its gate holds, the `next` part for window r - 1; the gate bits come from the tile.  One bit per (entry, half,
//            row) goes to HBM as [n][2][EW] words, each written whole by the wave that owns the row: no atomics.
//   count    k_ta_count: thread <-> entry, a workgroup walks WPB windows: free at r = bit [r][0] | bit [r + 1][1].  MA_COUNT: table[e][x] and one
//            integer atomic on totals[e]; scan (k_ta_scan: the rank audit's scan over table rows); MA_LIST: the thread whose prefix is below R
//            walks its windows again and writes rows[e][rank].  No atomic admits a row: the words are identical run after run.
// LDS (u32 words): phase 1 and merge: 8 + 3 AW + AW AW + AW + 33 (w | 1) (AW is odd).  Phase 2: 8 + EC (2 w + 4) + (w + prep w) S (tile) + per wave
// the rank audit's words.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, AW <= TA_MAX_WINDOW <
// 192 = 3 x 64 lane words, gate columns are in 1 .. 2 w, listed windows have ranks below R).
#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include "rank_elim.hpp"

namespace vk {

constexpr uint32_t TA_F_OUTSIDE = 1, TA_F_ANY0 = 2, TA_F_ANY1 = 4;  // host/transition_audit.hpp: TA_OUTSIDE, TA_ANY0, TA_ANY1

__host__ __device__ inline uint32_t ta_basis_words(uint32_t w) {
    const uint32_t AW = 2u * w + 1u;
    return 8u + 3u * AW + AW * AW + AW + (TA_TILE_WINDOWS + 1u) * (w | 1u);
}

// Workgroup x: rows [x TA_BOOL_ROWS, ..) of every column.  LDS: [w][4] flags (local | next << 3), ones as local, ones as next, unused; then two
// ballot words per wave.
__global__ void __launch_bounds__(256) k_ta_flags(const uint32_t* __restrict__ main, uint64_t mstride, uint64_t n, uint32_t w, uint32_t* __restrict__ flags, unsigned long long* __restrict__ ones) {
    extern __shared__ uint32_t ta_lds[];
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t* acc = ta_lds;
    uint32_t* slot = ta_lds + 4u * w + 2u * wave;
    for (uint32_t x = t; x < 4u * w; x += NT) acc[x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * TA_BOOL_ROWS;
    const uint32_t rows = n - base < TA_BOOL_ROWS ? (uint32_t)(n - base) : TA_BOOL_ROWS;
    for (uint32_t c = 0; c < w; c++) {
        uint32_t fl = 0, n_loc = 0, n_nxt = 0;  // n_loc, n_nxt: wave-uniform
        for (uint32_t j0 = 0; j0 < rows; j0 += NT) {  // workgroup-uniform trip count
            const uint32_t j = j0 + t;
            const uint64_t r = base + j;
            const bool in = j < rows, loc = in && r + 1 < n, nxt = in && r >= 1;
            const uint32_t v = in ? main[(uint64_t)c * mstride + r] : 0u;
            const uint32_t cls = v == 0 ? TA_F_ANY0 : (v == vg::R_MOD_P ? TA_F_ANY1 : TA_F_OUTSIDE);
            if (loc) fl |= cls;
            if (nxt) fl |= cls << 3;
            n_loc += (uint32_t)__builtin_popcountll(ra_ballot(loc && cls == TA_F_ANY1, slot));
            n_nxt += (uint32_t)__builtin_popcountll(ra_ballot(nxt && cls == TA_F_ANY1, slot));
        }
        uint32_t wf = 0;
#pragma unroll
        for (uint32_t b = 0; b < 6; b++) wf |= ra_ballot((fl >> b) & 1u, slot) ? 1u << b : 0u;
        if (lane == 0) {
            if (wf) atomicOr(&acc[4u * c], wf);
            if (n_loc) atomicAdd(&acc[4u * c + 1], n_loc);
            if (n_nxt) atomicAdd(&acc[4u * c + 2], n_nxt);
        }
    }
    __syncthreads();
    for (uint32_t c = t; c < w; c += NT) {
        const uint32_t f = acc[4u * c];
        if (f & 7u) atomicOr(&flags[1u + c], f & 7u);
        if (f >> 3) atomicOr(&flags[1u + w + c], f >> 3);
        if (acc[4u * c + 1]) atomicAdd(&ones[1u + c], (unsigned long long)acc[4u * c + 1]);
        if (acc[4u * c + 2]) atomicAdd(&ones[1u + w + c], (unsigned long long)acc[4u * c + 2]);
    }
}

// the wave's elimination state over AW window columns in lds: slot, row_of, nzf, nxt, basis (irow, raw, regs are not used by ra_insert)
__device__ __forceinline__ RaWave ta_wave(uint32_t* lds, uint32_t AW, uint32_t lane) {
    RaWave W;
    W.w = AW; W.BS = AW | 1u; W.WPL = (AW + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = lds; W.row_of = lds + 8; W.nzf = W.row_of + AW; W.nxt = W.nzf + AW; W.basis = W.nxt + AW;
    W.irow = nullptr; W.raw = nullptr; W.regs = nullptr;
    for (uint32_t c = lane; c < AW; c += 64u) { W.row_of[c] = RA_NONE; W.nzf[c] = 0; }
    ra_wave_sync();
    return W;
}

// a partial basis: AW pivot flags, then row p of [AW][AW] for every pivot column p
__device__ __forceinline__ void ta_write_part(const RaWave& W, uint32_t* out) {
    const uint32_t AW = W.w, BS = W.BS, lane = W.lane;
    for (uint32_t c = lane; c < AW; c += 64u) out[c] = W.row_of[c] != RA_NONE ? 1u : 0u;
    for (uint32_t p = 0; p < AW; p++) {
        if (W.row_of[p] == RA_NONE) continue;  // wave-uniform
        for (uint32_t c = lane; c < AW; c += 64u) out[AW + (uint64_t)p * AW + c] = W.basis[p * BS + c];
    }
}

// Workgroup (x, g), 64 threads: the reduced basis of the windows [x RB, min(n - 1, x RB + RB)) on which gate g holds -> slot x of gate g's part.
__global__ void __launch_bounds__(64) k_ta_basis(const uint32_t* __restrict__ main, uint64_t mstride, uint64_t n, uint32_t w, uint32_t RB, const uint32_t* __restrict__ gates,
                                                 uint64_t gate_slots, uint32_t* __restrict__ part) {
    extern __shared__ uint32_t ta_lds[];
    const uint32_t lane = threadIdx.x, AW = 2u * w + 1u, ws = w | 1u;
    RaWave W = ta_wave(ta_lds, AW, lane);
    uint32_t* cur = W.basis + AW * W.BS;  // [AW]
    uint32_t* tile = cur + AW;            // [TA_TILE_WINDOWS + 1][ws]
    const uint32_t gj = gates[2u * blockIdx.y], gv = gates[2u * blockIdx.y + 1u];
    const uint64_t NWIN = n - 1, base = (uint64_t)blockIdx.x * RB, end = base + RB < NWIN ? base + RB : NWIN;
    for (uint64_t t0 = base; t0 < end && W.rho < AW; t0 += TA_TILE_WINDOWS) {
        const uint32_t wins = end - t0 < TA_TILE_WINDOWS ? (uint32_t)(end - t0) : TA_TILE_WINDOWS;
        for (uint32_t x = lane; x < w * (TA_TILE_WINDOWS + 1u); x += 64u) {
            const uint32_t col = x / (TA_TILE_WINDOWS + 1u), j = x % (TA_TILE_WINDOWS + 1u);
            if (j <= wins) tile[j * ws + col] = main[(uint64_t)col * mstride + t0 + j];  // t0 + wins <= n - 1
        }
        ra_wave_sync();
        for (uint32_t j = 0; j < wins && W.rho < AW; j++) {
            if (gj && (gj <= w ? tile[j * ws + gj - 1u] : tile[(j + 1u) * ws + gj - 1u - w]) != gv) continue;  // wave-uniform
            for (uint32_t c = lane; c < AW; c += 64u) cur[c] = c == 0 ? vg::R_MOD_P : (c <= w ? tile[j * ws + c - 1u] : tile[(j + 1u) * ws + c - 1u - w]);
            ra_wave_sync();
            ra_insert(W, cur);
            ra_wave_sync();
        }
        ra_wave_sync();
    }
    ta_write_part(W, part + ((uint64_t)blockIdx.y * gate_slots + blockIdx.x) * AW * (AW + 1u));
}

// Workgroup (x, g), 64 threads, eliminates the partial bases [x fan, min(n_parts, x fan + fan)) of gate g at src into one.  dst != null: written as
// slot x of gate g at dst (a level of the tree); otherwise (one workgroup per gate) inv + g inv_words as launch.hpp (TaArgs) describes it.
__global__ void __launch_bounds__(64) k_ta_merge(const uint32_t* __restrict__ src, uint32_t n_parts, uint32_t fan, uint32_t AW, uint64_t gate_slots, uint32_t* __restrict__ dst,
                                                 uint32_t* __restrict__ inv_all, uint64_t inv_words) {
    extern __shared__ uint32_t ta_lds[];
    const uint32_t lane = threadIdx.x, BS = AW | 1u;
    RaWave W = ta_wave(ta_lds, AW, lane);
    uint32_t* cur = W.basis + AW * BS;  // [AW]
    const uint64_t slot = (uint64_t)AW * (AW + 1u);
    const uint32_t g0 = blockIdx.x * fan, g1 = n_parts - g0 < fan ? n_parts : g0 + fan;
    for (uint32_t g = g0; g < g1 && W.rho < AW; g++) {
        const uint32_t* in = src + ((uint64_t)blockIdx.y * gate_slots + g) * slot;
        for (uint32_t p = 0; p < AW && W.rho < AW; p++) {
            if (!in[p]) continue;  // wave-uniform
            for (uint32_t c = lane; c < AW; c += 64u) cur[c] = in[AW + (uint64_t)p * AW + c];
            ra_wave_sync();
            ra_insert(W, cur);
            ra_wave_sync();
        }
    }
    if (dst) {
        ta_write_part(W, dst + ((uint64_t)blockIdx.y * gate_slots + blockIdx.x) * slot);
        return;
    }
    uint32_t* inv = inv_all + (uint64_t)blockIdx.y * inv_words;
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

// Is c [w] (LDS) outside the row space of the wave's reduced basis?  Wave-uniform.  (invariant_audit.hip's ia_free.)
__device__ __forceinline__ bool ta_free(RaWave& W, const uint32_t* c) {
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

// Workgroup x: rows [x T, x T + T) -> their words of bits.
template <int CHIP>
__global__ void __launch_bounds__(256) k_ta_enforce(TaArgs ta, uint32_t* __restrict__ bits) {
    extern __shared__ uint32_t ta_lds[];
    const RaArgs& a = ta.r;
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6, w = a.width, T = a.T, S = (T + 2u) | 1u;
    const uint32_t E = ta.E, EC = ta.EC, EW = (E + 31u) >> 5, NCH = (E + EC - 1u) / EC;
    uint32_t* vecs = ta_lds + 8;         // [EC][2 w]
    uint32_t* eg = vecs + EC * 2u * w;   // [EC][4]
    uint32_t* tm = eg + EC * 4u;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S + wave * ra_wave_words(w, a.K, a.n_regs, CHIP == CA_INTERPRET);
    RaWave W;
    W.w = w; W.BS = w | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.nzf = W.row_of + w; W.nxt = W.nzf + w; W.irow = W.nxt + w; W.basis = W.irow + w; W.raw = W.basis + w * W.BS;
    W.regs = W.raw + a.K * w + lane;
    auto stage = [&](uint32_t ch) {
        const uint32_t e0 = ch * EC, cnt = E - e0 < EC ? E - e0 : EC;
        for (uint32_t x = t; x < cnt * 2u * w; x += NT) vecs[x] = ta.evec[(uint64_t)e0 * 2u * w + x];
        for (uint32_t x = t; x < cnt * 4u; x += NT) eg[x] = ta.egate[(uint64_t)e0 * 4u + x];
    };
    if (NCH == 1) stage(0);
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
            if (!reuse) ra_row<CHIP>(a, W, tm, tp, S, j, r);
        }
        uint32_t wa = 0, wb = 0;  // wave-uniform: the words of bits being filled (a word may span two chunks)
        for (uint32_t ch = 0; ch < NCH; ch++) {
            if (NCH > 1) {
                __syncthreads();
                stage(ch);
                __syncthreads();
            }
            if (!active) continue;
            const uint32_t e0 = ch * EC, cnt = E - e0 < EC ? E - e0 : EC;
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t e = e0 + k, gj = eg[4u * k], gv = eg[4u * k + 1u], nz = eg[4u * k + 2u];
                // the gate's cell on window q: row q (tile word q - base + 1) for a `local` column, row q + 1 for a `next` one
                const uint32_t* gc = !gj ? tm : (gj <= w ? tm + (gj - 1u) * S : tm + (gj - 1u - w) * S + 1u);
                if (W.rho != w) {
                    if ((nz & 1u) && r + 1 < a.n && (!gj || gc[j + 1u] == gv) && ta_free(W, vecs + k * 2u * w)) wa |= 1u << (e & 31u);
                    if ((nz & 2u) && r >= 1 && (!gj || gc[j] == gv) && ta_free(W, vecs + k * 2u * w + w)) wb |= 1u << (e & 31u);
                }
                if ((e & 31u) == 31u || e + 1 == E) {
                    if (lane == 0) {
                        bits[(r * 2u) * EW + (e >> 5)] = wa;
                        bits[(r * 2u + 1u) * EW + (e >> 5)] = wb;
                    }
                    wa = wb = 0;
                }
            }
        }
    }
}

// Workgroup (x, y): entry e = 256 y + t over the windows [x WPB, min(n - 1, x WPB + WPB)).
__global__ void __launch_bounds__(256) k_ta_count(const uint32_t* __restrict__ bits, uint64_t n, uint32_t E, uint32_t WPB, uint32_t NB2, uint32_t mode, unsigned long long* __restrict__ totals,
                                                  uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix, uint32_t R, uint32_t* __restrict__ rows) {
    const uint32_t e = blockIdx.y * blockDim.x + threadIdx.x, EW = (E + 31u) >> 5;
    if (e >= E) return;
    const uint64_t at = (uint64_t)e * NB2 + blockIdx.x;
    uint32_t rank = 0;
    if (mode == MA_LIST) {
        if (!table[at] || prefix[at] >= R) return;
        rank = prefix[at];
    }
    const uint64_t NWIN = n - 1, base = (uint64_t)blockIdx.x * WPB, end = base + WPB < NWIN ? base + WPB : NWIN;
    const uint32_t wd = e >> 5, sh = e & 31u;
    uint32_t cnt = 0;
    for (uint64_t r = base; r < end; r++) {
        const uint32_t f = ((bits[(r * 2u) * EW + wd] | bits[((r + 1) * 2u + 1u) * EW + wd]) >> sh) & 1u;
        if (mode == MA_COUNT) { cnt += f; continue; }
        if (!f) continue;
        rows[(uint64_t)e * R + rank] = (uint32_t)r;
        if (++rank >= R) return;
    }
    if (mode != MA_COUNT) return;
    table[at] = cnt;
    if (cnt) atomicAdd(&totals[e], (unsigned long long)cnt);
}

// Row c of table [..][NB] -> its exclusive prefix (rank_audit.hip's k_ra_scan).
__global__ void __launch_bounds__(256) k_ta_scan(const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB) {
    extern __shared__ uint32_t ta_lds[];  // [256] partial sums
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)c * NB;
    uint32_t s = 0;
    for (uint32_t x = lo; x < hi; x++) s += row[x];
    ta_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = ta_lds[i]; ta_lds[i] = run; run += x; }
    }
    __syncthreads();
    uint32_t run = ta_lds[t];
    uint32_t* out = prefix + (uint64_t)c * NB;
    for (uint32_t x = lo; x < hi; x++) { out[x] = run; run += row[x]; }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t ta_basis_lds_bytes(uint32_t width) { return 4 * (size_t)ta_basis_words(width); }

void ta_basis_shape(TaArgs& ta, uint32_t gates) {
    const RaArgs& a = ta.r;
    const size_t LDS = 160 * 1024;
    const uint64_t AW = 2ull * a.width + 1;
    if (AW > TA_MAX_WINDOW || ta_basis_lds_bytes(a.width) > LDS)
        throw std::invalid_argument("transition_audit: the window of a chip of " + std::to_string(a.width) + " columns has 2 w + 1 = " + std::to_string(AW) + " columns, at most " +
                                    std::to_string(TA_MAX_WINDOW) + " (its basis and tile take " + std::to_string(ta_basis_lds_bytes(a.width)) +
                                    " bytes of a workgroup's LDS: 4 x ((2 w + 1)^2 + 4 (2 w + 1) + 33 (w | 1) + 8), 163840 at most)");
    // slices of whole tiles of windows: at most IA_MAX_WORKGROUPS per gate, and no more than 128 MB of partial bases over `gates` gates
    const uint64_t NWIN = a.n > 1 ? a.n - 1 : 1;
    const uint64_t most = std::min<uint64_t>(IA_MAX_WORKGROUPS, std::max<uint64_t>(1, (1ull << 25) / (ta_slot_words(ta) * std::max(1u, gates))));
    const uint64_t tiles = (NWIN + TA_TILE_WINDOWS - 1) / TA_TILE_WINDOWS;
    const uint64_t per = (tiles + most - 1) / most;
    ta.RB = (uint32_t)(per * TA_TILE_WINDOWS);
    ta.NB1 = (uint32_t)((NWIN + ta.RB - 1) / ta.RB);
}

size_t ta_lds_bytes(const TaArgs& ta, uint32_t NW, uint32_t T, uint32_t EC) {
    const RaArgs& a = ta.r;
    const size_t S = (T + 2u) | 1u;
    return 4 * (8 + (size_t)EC * (2 * (size_t)a.width + 4) + ((size_t)a.width + a.prep_width) * S + (size_t)NW * ra_wave_words(a.width, a.K, a.n_regs, a.native_chip == CA_INTERPRET));
}

void ta_shape(TaArgs& ta) {
    RaArgs& a = ta.r;
    const size_t LDS = 160 * 1024;
    if (2 * a.width + 1 > TA_MAX_WINDOW || ta_lds_bytes(ta, 1, 1, 1) > LDS)
        throw std::invalid_argument("transition_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints and " +
                                    std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) + " interpreted registers does not fit a workgroup's LDS with one wave and one entry staged (" +
                                    std::to_string(ta_lds_bytes(ta, 1, 1, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + 128 per register + 4 w + 12 + 3 (w + prep w) + 2 w + 4), 163840 at most)");
    // the entries staged at a time when sizing the launch: all of them up to 16; the chunk then grows into what the chosen shape leaves unused
    const uint32_t ec0 = std::max(1u, std::min(ta.E, 16u));
    auto fits = [&](uint32_t nw, uint32_t rpw, uint32_t ec) { return ta_lds_bytes(ta, nw, nw * rpw, ec) <= LDS; };
    uint32_t ec_min = ec0;
    while (ec_min > 1 && !fits(1, 1, ec_min)) ec_min >>= 1;
    // the most waves per CU; among equals the larger workgroup (fewer tiles staged): rank_audit.hip's rule
    uint32_t best = 1, best_waves = 0;
    for (uint32_t nw = 4; nw >= 1; nw >>= 1) {
        uint32_t rpw = 16;
        while (rpw > 1 && (a.n / ((uint64_t)nw * rpw) < 1024 || !fits(nw, rpw, ec_min))) rpw >>= 1;
        if (!fits(nw, rpw, ec_min)) continue;
        const uint32_t waves = (uint32_t)(LDS / ta_lds_bytes(ta, nw, nw * rpw, ec_min)) * nw;
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    a.NW = best;
    uint32_t rpw = 16;
    while (rpw > 1 && (a.n / ((uint64_t)a.NW * rpw) < 1024 || !fits(a.NW, rpw, ec_min))) rpw >>= 1;
    a.RPW = rpw;
    a.T = a.NW * a.RPW;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
    // the chunk: what the workgroup's share of the LDS leaves, without lowering the workgroups per CU
    const size_t b = ta_lds_bytes(ta, a.NW, a.T, ec_min), share = LDS / (LDS / b);
    const uint64_t more = (share - b) / (4 * (2 * (size_t)a.width + 4));
    ta.EC = (uint32_t)std::min<uint64_t>(std::max(1u, ta.E), ec_min + more);
    const uint64_t NWIN = a.n > 1 ? a.n - 1 : 1;
    ta.WPB = (uint32_t)std::max<uint64_t>(256, (NWIN + IA_MAX_WORKGROUPS - 1) / IA_MAX_WORKGROUPS);
    ta.NB2 = (uint32_t)((NWIN + ta.WPB - 1) / ta.WPB);
}

#define TA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

// the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
static void ta_opt_in() {
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("transition_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("transition_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) +
                                     ": " + hipGetErrorString(e));
    };
    opt_in((const void*)k_ta_basis, "k_ta_basis");
    opt_in((const void*)k_ta_merge, "k_ta_merge");
#define TA_X(C) opt_in((const void*)k_ta_enforce<vchips::C>, "k_ta_enforce<" #C ">");
    TA_CHIPS(TA_X)
#undef TA_X
    opt_in((const void*)k_ta_enforce<CA_INTERPRET>, "k_ta_enforce<CA_INTERPRET>");
    opt_in((const void*)k_ta_enforce<MA_BUS_ONLY>, "k_ta_enforce<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

static void ta_basis_check(const TaArgs& ta) {
    const RaArgs& a = ta.r;
    if (a.width == 0 || 2 * a.width + 1 > TA_MAX_WINDOW) throw std::logic_error("transition_audit: 1 to 91 columns");
    // the kernels take any slice length and any number of slices; whole tiles and the caps are ta_basis_shape's choice
    if (a.n < 2 || ta.RB == 0 || ta.NB1 == 0 || ta.NB1 != (uint32_t)((a.n - 1 + ta.RB - 1) / ta.RB)) throw std::logic_error("transition_audit: inconsistent basis launch shape");
    if (ta_basis_lds_bytes(a.width) > 160 * 1024) throw std::logic_error("transition_audit: the basis does not fit the LDS");
    ta_opt_in();
}

void launch_ta_flags(hipStream_t st, const TaArgs& ta, uint32_t* flags, unsigned long long* ones) {
    const RaArgs& a = ta.r;
    if (a.width == 0 || a.n < 2) throw std::logic_error("transition_audit: a chip without windows");
    ProfScope ps("k_ta_flags", st, 4.0 * (double)a.n * a.width);
    const uint32_t NT = 256;
    VK_LAUNCH(k_ta_flags, dim3((uint32_t)((a.n + TA_BOOL_ROWS - 1) / TA_BOOL_ROWS)), dim3(NT), 4 * (4 * (size_t)a.width + 2 * (NT / 64)), st, a.main, a.mstride, a.n, a.width, flags, ones);
}

void launch_ta_basis(hipStream_t st, const TaArgs& ta, uint32_t* part) {
    ta_basis_check(ta);
    if (ta.G == 0 || ta.G > 65535 || !ta.gates) throw std::logic_error("transition_audit: 1 to 65535 gates");
    ProfScope ps("k_ta_basis", st, 4.0 * (double)ta.r.n * ta.r.width * ta.G);
    VK_LAUNCH(k_ta_basis, dim3(ta.NB1, ta.G), dim3(64), ta_basis_lds_bytes(ta.r.width), st, ta.r.main, ta.r.mstride, ta.r.n, ta.r.width, ta.RB, ta.gates, ta_gate_slots(ta), part);
}

void launch_ta_merge(hipStream_t st, const TaArgs& ta, uint32_t* part, uint32_t* inv) {
    ta_basis_check(ta);
    if (ta.G == 0 || ta.G > 65535) throw std::logic_error("transition_audit: 1 to 65535 gates");
    ProfScope ps("k_ta_merge", st, 4.0 * (double)ta_part_words(ta));
    // a tree of fan IA_MERGE_FAN: within a gate's slots the levels ping-pong between the slices' slots and the spare slots behind them
    const uint32_t AW = 2 * ta.r.width + 1;
    uint32_t *src = part, *dst = part + (uint64_t)ta.NB1 * ta_slot_words(ta);
    uint32_t n = ta.NB1;
    while (n > IA_MERGE_FAN) {
        const uint32_t m = (n + IA_MERGE_FAN - 1) / IA_MERGE_FAN;
        VK_LAUNCH(k_ta_merge, dim3(m, ta.G), dim3(64), ta_basis_lds_bytes(ta.r.width), st, src, n, IA_MERGE_FAN, AW, ta_gate_slots(ta), dst, nullptr, 0ull);
        std::swap(src, dst);
        n = m;
    }
    VK_LAUNCH(k_ta_merge, dim3(1, ta.G), dim3(64), ta_basis_lds_bytes(ta.r.width), st, src, n, IA_MERGE_FAN, AW, ta_gate_slots(ta), nullptr, inv, ta_inv_words(ta));
}

static void ta_check(const TaArgs& ta) {
    const RaArgs& a = ta.r;
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("transition_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || 2 * a.width + 1 > TA_MAX_WINDOW || ta.E == 0 || ta.EC == 0 || ta.EC > ta.E || !ta.evec || !ta.egate) throw std::logic_error("transition_audit: 1 to 91 columns and at least one entry");
    if (a.n < 2 || (a.n & (a.n - 1)) || (a.NW != 1 && a.NW != 2 && a.NW != 4) || a.RPW == 0 || a.T != a.NW * a.RPW || a.NB != (uint32_t)((a.n + a.T - 1) / a.T))
        throw std::logic_error("transition_audit: inconsistent launch shape");
    if (ta.WPB == 0 || ta.NB2 != (uint32_t)((a.n - 1 + ta.WPB - 1) / ta.WPB)) throw std::logic_error("transition_audit: inconsistent count shape");
    if (ta_lds_bytes(ta, a.NW, a.T, ta.EC) > 160 * 1024) throw std::logic_error("transition_audit: the launch shape does not fit the LDS");
    ta_opt_in();
}

void launch_ta_enforce(hipStream_t st, const TaArgs& ta, uint32_t* bits) {
    ta_check(ta);
    const RaArgs& a = ta.r;
    static const char* names[14] = {"k_ta_enforce.cpu", "k_ta_enforce.program", "k_ta_enforce.mem", "k_ta_enforce.add", "k_ta_enforce.sub", "k_ta_enforce.mul", "k_ta_enforce.div",
                                    "k_ta_enforce.shift", "k_ta_enforce.lt", "k_ta_enforce.com", "k_ta_enforce.bitwise", "k_ta_enforce.output", "k_ta_enforce.range", "k_ta_enforce.static_data"};
    const int id = a.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_ta_enforce.bus" : "k_ta_enforce");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width), a.evaluations);
    const dim3 grid(a.NB), block(64 * a.NW);
    const size_t lds = ta_lds_bytes(ta, a.NW, a.T, ta.EC);
    switch (a.native_chip) {
#define TA_X(C) case vchips::C: VK_LAUNCH((k_ta_enforce<vchips::C>), grid, block, lds, st, ta, bits); break;
        TA_CHIPS(TA_X)
#undef TA_X
        case CA_INTERPRET: VK_LAUNCH((k_ta_enforce<CA_INTERPRET>), grid, block, lds, st, ta, bits); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_ta_enforce<MA_BUS_ONLY>), grid, block, lds, st, ta, bits); break;
        default: throw std::logic_error("transition_audit: a native chip id without constraints");
    }
}

void launch_ta_count(hipStream_t st, const TaArgs& ta, const uint32_t* bits, unsigned long long* totals, uint32_t* table) {
    ta_check(ta);
    ProfScope ps("k_ta_count", st, 8.0 * (double)ta.r.n * ((ta.E + 31u) / 32u));
    VK_LAUNCH(k_ta_count, dim3(ta.NB2, (ta.E + 255u) / 256u), dim3(256), 0, st, bits, ta.r.n, ta.E, ta.WPB, ta.NB2, MA_COUNT, totals, table, nullptr, 0u, nullptr);
}

void launch_ta_scan(hipStream_t st, const TaArgs& ta, const uint32_t* table, uint32_t* prefix) {
    ta_check(ta);
    ProfScope ps("k_ta_scan", st, 8.0 * (double)ta.NB2 * ta.E);
    VK_LAUNCH(k_ta_scan, dim3(ta.E), dim3(256), 256 * 4, st, table, prefix, ta.NB2);
}

void launch_ta_list(hipStream_t st, const TaArgs& ta, const uint32_t* bits, const uint32_t* table, const uint32_t* prefix, uint32_t R, uint32_t* rows) {
    ta_check(ta);
    ProfScope ps("k_ta_list", st, 0);
    VK_LAUNCH(k_ta_count, dim3(ta.NB2, (ta.E + 255u) / 256u), dim3(256), 0, st, bits, ta.r.n, ta.E, ta.WPB, ta.NB2, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, R, rows);
}

}  // namespace vk
