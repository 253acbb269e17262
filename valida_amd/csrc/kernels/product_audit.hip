// Product audit on the device (host/product_audit.hpp states the contract): per chip the products of two independent columns that are an affine
// function of the row on every row of the trace, and per relation the rows on which the rank audit's Jacobian enforces it.  The pivot columns Pi
// come from the invariant audit's phase 1 and merge (launch_ia_basis, launch_ia_merge); pcols [rho] lists them (pcols[0] = 0 is the constant).
//   rows     k_pq_rows: workgroup x (ONE wave) takes the RS consecutive rows [x RS, x RS + RS) of the working layout (column-major Montgomery)
//            restricted to Pi, rho columns, lane l <-> columns l, l + 64, l + 128, and eliminates them in order into a reduced basis in LDS
//            (rank_elim.hpp's ra_insert, the very function); a row that raised the rank is remembered: at most rho per slice.  Rows are staged
//            32 at a time as [32][BS], BS = rho | 1 (odd row stride: the LDS writes of 32 lanes go to 32 banks).  The slot of the workgroup:
//            [0] how many, then the rows ascending.
//   merge    k_pq_rowmerge: the first-independent rows of L ++ R are those of first-independent(L) ++ first-independent(R) taken in that order,
//            so a node (one wave) reads the rows its up to 16 slots name, in slot order, from the trace again, inserts them and keeps the ones
//            that raise the rank: a tree of fan 16 that keeps slice order gives the same rho rows whatever the grid.
//   solve    k_pq_solve: one workgroup of 256 threads gathers G [rho][rho], the basis rows over Pi, and inverts it by Gauss-Jordan on (G | 1)
//            [rho][2 rho] — in LDS when 4 (16 + rho + 2 rho^2) bytes fit 160 KB (rho <= 142), else in pool scratch — first non-zero row as the
//            pivot; G is regular by construction, status[0] = 1 otherwise.  k_pq_beta: lanes over pairs, beta_pair = inverse x (products at the
//            basis rows), [m][rho]; sets the pair's flag.
//   sweep    k_pq_sweep (the hot path): workgroup (x, y) = 64 rows x 32 pairs, 256 threads.  The rows are staged in LDS as [rho][64] (global
//            reads are 256-byte runs of one column; lane <-> row, so the reads of one column are 64 consecutive words: no bank conflict), the
//            beta of the group as [32][rho] (a wave reads one word at a time: a broadcast).  One thread owns one (row, pair) at a time: wave v
//            takes pairs v, v + 4, ..; rho multiply-adds, four products to one Montgomery reduction (monty_reduce_wide).  A mismatch stores 0
//            into the pair's flag: the final set does not depend on order.  LDS: 4 (64 rho + 32 rho + 64) bytes, 73 KB at rho = 192.  A first
//            launch runs the first 256 rows with all m pairs, k_pq_compact (one workgroup, an ordered scan) lists the survivors, a second
//            launch runs all rows with those.
//   enforce  k_pq_enforce<CHIP>: rank_audit.hip's shape — one wave per trace row, NW waves per workgroup, RPW rows per wave, the tile
//            [column][S] with halo and wrap, ra_row<CHIP> once per row (the rank audit's dual evaluation and LDS elimination, unchanged).  The
//            relations are sparse lists (i, j, then (column, -beta) for beta's support and for i and j); a group of them is staged in LDS by
//            the whole workgroup while every wave's basis is live (one group: staged once).  Per row and relation the wave scatters g_r into
//            one of its two row buffers (the list's value plus the row's cell at i and j), one ballot per lane word gives the flat bit and
//            the pivot columns to reduce by, one reduce-only sweep against the reduced basis the verdict (rho = w: enforced, no sweep), and
//            the lanes that wrote g_r clear it again: one wave sync per relation, the buffers alternate.
//   count    lane 0 of a wave adds the verdicts to the wave's own counters in LDS; at the end of the workgroup's rows the waves' counters are
//            summed, one integer atomic per workgroup and relation on the chip's totals; the count also goes into table[e][workgroup].
//   scan     the rank audit's k_ra_scan over table rows (launch_ra_scan).
//   list     workgroups that hold a free row of rank < R of a listed relation run their rows again; the waves of a round exchange their free
//            bits through LDS so that rank = prefix + rows before in the workgroup; the owning lane writes the row.  No atomic admits a row.
// LDS (u32 words): rows and merge: 8 + 3 rho + rho BS + 32 BS.  Enforce: 8 + (2 NW + 2) E (the waves' counters or free bits, need, running) +
// GE + 1 + GW (the staged group) + (w + prep w) S (tile) + per wave the rank audit's words — and never less than the rank audit's own bytes for
// the same shape (pq_lds_bytes): the shape must also pass launch_ra_scan's check.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, rho <= 192 = 3 x 64 lane
// words, rows named by a slot are rows of the trace, columns of an entry are below w, rows written by `list` have ranks below R and relations
// below i_cut <= E).
#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include "rank_elim.hpp"

namespace vk {

__host__ __device__ inline uint32_t pq_rows_lds_words(uint32_t rho) { return 8u + 3u * rho + rho * (rho | 1u) + IA_TILE_ROWS * (rho | 1u); }

// the wave's elimination state over rho compacted columns in lds: slot, row_of, nzf, nxt, basis (irow, raw, regs are not used by ra_insert)
__device__ __forceinline__ RaWave pq_wave(uint32_t* lds, uint32_t rho, uint32_t lane) {
    RaWave W;
    W.w = rho; W.BS = rho | 1u; W.WPL = (rho + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = lds; W.row_of = lds + 8; W.nzf = W.row_of + rho; W.nxt = W.nzf + rho; W.basis = W.nxt + rho;
    W.irow = nullptr; W.raw = nullptr; W.regs = nullptr;
    for (uint32_t c = lane; c < rho; c += 64u) { W.row_of[c] = RA_NONE; W.nzf[c] = 0; }
    ra_wave_sync();
    return W;
}

// Workgroup x (64 threads): the rows of [x RS, min(n, x RS + RS)) that raise the rank of the rows before them in the slice -> part + x (rho + 1)
__global__ void __launch_bounds__(64) k_pq_rows(const uint32_t* __restrict__ main, uint64_t mstride, uint64_t n, uint32_t rho, const uint32_t* __restrict__ pcols, uint32_t RS,
                                                uint32_t* __restrict__ part) {
    extern __shared__ uint32_t pq_lds[];
    const uint32_t lane = threadIdx.x, BS = rho | 1u;
    RaWave W = pq_wave(pq_lds, rho, lane);
    uint32_t* tile = W.basis + rho * BS;  // [32][BS]
    uint32_t* out = part + (uint64_t)blockIdx.x * (rho + 1u);
    const uint64_t base = (uint64_t)blockIdx.x * RS, end = base + RS < n ? base + RS : n;
    for (uint64_t t0 = base; t0 < end && W.rho < rho; t0 += IA_TILE_ROWS) {
        const uint32_t rows = end - t0 < IA_TILE_ROWS ? (uint32_t)(end - t0) : IA_TILE_ROWS;
        for (uint32_t x = lane; x < rho * IA_TILE_ROWS; x += 64u) {
            const uint32_t col = x / IA_TILE_ROWS, j = x % IA_TILE_ROWS;
            if (j < rows) tile[j * BS + col] = col ? main[(uint64_t)(pcols[col] - 1u) * mstride + t0 + j] : vg::R_MOD_P;
        }
        ra_wave_sync();
        for (uint32_t j = 0; j < rows && W.rho < rho; j++) {
            const uint32_t before = W.rho;
            ra_insert(W, tile + j * BS);
            if (W.rho != before && lane == 0) out[W.rho] = (uint32_t)(t0 + j);  // wave-uniform
        }
        ra_wave_sync();
    }
    if (lane == 0) out[0] = W.rho;
}

// Workgroup x (64 threads) inserts the rows the slots [x fan, min(n_parts, x fan + fan)) of `part` name, in order, and writes the ones that raise
// the rank to slot x of out.
__global__ void __launch_bounds__(64) k_pq_rowmerge(const uint32_t* __restrict__ main, uint64_t mstride, uint32_t rho, const uint32_t* __restrict__ pcols,
                                                    const uint32_t* __restrict__ part, uint32_t n_parts, uint32_t fan, uint32_t* __restrict__ out_part) {
    extern __shared__ uint32_t pq_lds[];
    const uint32_t lane = threadIdx.x, BS = rho | 1u;
    RaWave W = pq_wave(pq_lds, rho, lane);
    uint32_t* cur = W.basis + rho * BS;  // [rho]
    uint32_t* out = out_part + (uint64_t)blockIdx.x * (rho + 1u);
    const uint32_t g0 = blockIdx.x * fan, g1 = n_parts - g0 < fan ? n_parts : g0 + fan;
    for (uint32_t g = g0; g < g1 && W.rho < rho; g++) {
        const uint32_t* in = part + (uint64_t)g * (rho + 1u);
        const uint32_t cnt = in[0] < rho ? in[0] : rho;  // wave-uniform
        for (uint32_t k = 0; k < cnt && W.rho < rho; k++) {
            const uint32_t r = in[1 + k];
            for (uint32_t c = lane; c < rho; c += 64u) cur[c] = c ? main[(uint64_t)(pcols[c] - 1u) * mstride + r] : vg::R_MOD_P;
            ra_wave_sync();
            const uint32_t before = W.rho;
            ra_insert(W, cur);
            if (W.rho != before && lane == 0) out[W.rho] = r;
            ra_wave_sync();
        }
    }
    if (lane == 0) out[0] = W.rho;
}

// One workgroup: G [rho][rho] = the rows `rows[1 ..]` over Pi, inv = its inverse.  aug: [rho][2 rho] of global scratch, or null: in LDS.
__global__ void __launch_bounds__(256) k_pq_solve(const uint32_t* __restrict__ main, uint64_t mstride, uint32_t rho, const uint32_t* __restrict__ pcols, const uint32_t* __restrict__ rows,
                                                  uint32_t* aug, uint32_t* __restrict__ G, uint32_t* __restrict__ inv, uint32_t* __restrict__ status) {
    extern __shared__ uint32_t pq_lds[];
    const uint32_t t = threadIdx.x, NT = blockDim.x, W2 = 2u * rho;
    uint32_t* ctl = pq_lds;        // [0] pivot row or RA_NONE, [1] the inverse of the pivot
    uint32_t* fcol = pq_lds + 16;  // [rho] column k before the elimination step
    uint32_t* a = aug ? aug : fcol + rho;
    for (uint32_t x = t; x < rho * rho; x += NT) {
        const uint32_t k = x / rho, c = x - k * rho;
        const uint32_t v = c ? main[(uint64_t)(pcols[c] - 1u) * mstride + rows[1 + k]] : vg::R_MOD_P;
        G[x] = v;
        a[k * W2 + c] = v;
        a[k * W2 + rho + c] = c == k ? vg::R_MOD_P : 0u;
    }
    __syncthreads();
    for (uint32_t k = 0; k < rho; k++) {
        if (t == 0) {
            uint32_t p = k;
            while (p < rho && a[p * W2 + k] == 0) p++;
            ctl[0] = p < rho ? p : RA_NONE;
            if (p < rho) ctl[1] = Fp::raw(a[p * W2 + k]).inv().v;
        }
        __syncthreads();
        const uint32_t p = ctl[0];
        if (p == RA_NONE) {  // the whole workgroup
            if (t == 0) status[0] = 1;
            return;
        }
        const Fp s = Fp::raw(ctl[1]);
        // rows p and k change places; the new row k is scaled
        for (uint32_t c = t; c < W2; c += NT) {
            const uint32_t vp = a[p * W2 + c], vk_ = a[k * W2 + c];
            a[k * W2 + c] = (Fp::raw(vp) * s).v;
            if (p != k) a[p * W2 + c] = vk_;
        }
        __syncthreads();
        for (uint32_t r = t; r < rho; r += NT) fcol[r] = a[r * W2 + k];
        __syncthreads();
        for (uint32_t x = t; x < rho * W2; x += NT) {
            const uint32_t r = x / W2, c = x - r * W2;
            if (r == k || fcol[r] == 0) continue;
            a[x] = (Fp::raw(a[x]) - Fp::raw(fcol[r]) * Fp::raw(a[k * W2 + c])).v;
        }
        __syncthreads();
    }
    for (uint32_t x = t; x < rho * rho; x += NT) {
        const uint32_t k = x / rho, c = x - k * rho;
        inv[x] = a[k * W2 + rho + c];
    }
    if (t == 0) status[0] = 0;
}

// pair p of q independent columns as positions (ti, tj) in pcols, 1 <= ti <= tj <= q
__device__ __forceinline__ void pq_pair(uint32_t q, uint32_t p, uint32_t& ti, uint32_t& tj) {
    uint32_t t = 1;
    while (p >= q - t + 1u) { p -= q - t + 1u; t++; }
    ti = t; tj = t + p;
}

// Thread <-> pair: beta[p][t] = sum_k inv[t][k] G[k][ti] G[k][tj]; flags[p] = 1
__global__ void __launch_bounds__(256) k_pq_beta(const uint32_t* __restrict__ G, const uint32_t* __restrict__ inv, uint32_t rho, uint32_t m, uint32_t* __restrict__ beta,
                                                 uint32_t* __restrict__ flags) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    uint32_t ti, tj;
    pq_pair(rho - 1u, p, ti, tj);
    for (uint32_t t = 0; t < rho; t++) {
        Fp s = Fp::zero();
        for (uint32_t k = 0; k < rho; k++) s += Fp::raw(inv[t * rho + k]) * (Fp::raw(G[k * rho + ti]) * Fp::raw(G[k * rho + tj]));
        beta[(uint64_t)p * rho + t] = s.v;
    }
    flags[p] = 1;
}

// Workgroup (x, y): rows [64 x, 64 x + 64) below n_rows, pairs list[32 y .. 32 y + 32) (list null: the pairs themselves).  A (row, pair) whose
// product is not beta . a_r clears the pair's flag.
__global__ void __launch_bounds__(256) k_pq_sweep(const uint32_t* __restrict__ main, uint64_t mstride, uint64_t n_rows, uint32_t rho, const uint32_t* __restrict__ pcols,
                                                  const uint32_t* __restrict__ beta, const uint32_t* __restrict__ list, uint32_t n_list, uint32_t* __restrict__ flags) {
    extern __shared__ uint32_t pq_lds[];
    const uint32_t t = threadIdx.x, NT = blockDim.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6;
    uint32_t* pid = pq_lds;                                  // [32] the pair, [32] ti | tj << 16
    uint32_t* tile = pq_lds + 2u * PQ_TILE_PAIRS;            // [rho][64]
    uint32_t* bl = tile + rho * PQ_TILE_ROWS;                // [32][rho]
    const uint64_t r0 = (uint64_t)blockIdx.x * PQ_TILE_ROWS;
    const uint32_t p0 = blockIdx.y * PQ_TILE_PAIRS, np = n_list - p0 < PQ_TILE_PAIRS ? n_list - p0 : PQ_TILE_PAIRS;
    const uint32_t rows = n_rows - r0 < PQ_TILE_ROWS ? (uint32_t)(n_rows - r0) : PQ_TILE_ROWS;
    if (t < np) {
        const uint32_t p = list ? list[p0 + t] : p0 + t;
        uint32_t ti, tj;
        pq_pair(rho - 1u, p, ti, tj);
        pid[t] = p; pid[PQ_TILE_PAIRS + t] = ti | (tj << 16);
    }
    for (uint32_t x = t; x < rho * PQ_TILE_ROWS; x += NT) {
        const uint32_t col = x / PQ_TILE_ROWS, j = x % PQ_TILE_ROWS;
        tile[x] = j < rows ? (col ? main[(uint64_t)(pcols[col] - 1u) * mstride + r0 + j] : vg::R_MOD_P) : 0u;
    }
    __syncthreads();
    for (uint32_t x = t; x < np * rho; x += NT) {
        const uint32_t k = x / rho, c = x - k * rho;
        bl[x] = beta[(uint64_t)pid[k] * rho + c];
    }
    __syncthreads();
    if (lane >= rows) return;
    for (uint32_t k = wave; k < np; k += NW) {
        const uint32_t* b = bl + k * rho;
        const uint32_t tt = pid[PQ_TILE_PAIRS + k], ti = tt & 0xffffu, tj = tt >> 16;
        Fp s = Fp::zero();
        uint32_t c = 0;
        for (; c + 4u <= rho; c += 4u) {
            const uint64_t acc = (uint64_t)tile[c * PQ_TILE_ROWS + lane] * b[c] + (uint64_t)tile[(c + 1u) * PQ_TILE_ROWS + lane] * b[c + 1u] +
                                 (uint64_t)tile[(c + 2u) * PQ_TILE_ROWS + lane] * b[c + 2u] + (uint64_t)tile[(c + 3u) * PQ_TILE_ROWS + lane] * b[c + 3u];
            s += Fp::raw(vg::monty_reduce_wide(acc));
        }
        for (; c < rho; c++) s += Fp::raw(tile[c * PQ_TILE_ROWS + lane]) * Fp::raw(b[c]);
        const Fp prod = Fp::raw(tile[ti * PQ_TILE_ROWS + lane]) * Fp::raw(tile[tj * PQ_TILE_ROWS + lane]);
        if (s != prod) flags[pid[k]] = 0;
    }
}

// One workgroup: out = the pairs of list[0 .. n_in) (null: 0 .. n_in - 1) whose flag is set, in order; count[0] = how many
__global__ void __launch_bounds__(256) k_pq_compact(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ list, uint32_t n_in, uint32_t* __restrict__ out,
                                                    uint32_t* __restrict__ count) {
    extern __shared__ uint32_t pq_lds[];  // [256] partial sums
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n_in + 255u) / 256u;
    const uint32_t lo = t * chunk < n_in ? t * chunk : n_in, hi = lo + chunk < n_in ? lo + chunk : n_in;
    uint32_t s = 0;
    for (uint32_t x = lo; x < hi; x++) s += flags[list ? list[x] : x] ? 1u : 0u;
    pq_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = pq_lds[i]; pq_lds[i] = run; run += x; }
        count[0] = run;
    }
    __syncthreads();
    uint32_t run = pq_lds[t];
    for (uint32_t x = lo; x < hi; x++) {
        const uint32_t p = list ? list[x] : x;
        if (flags[p]) out[run++] = p;
    }
}

// out[k][0 .. rho) = beta[list[k]][0 .. rho)
__global__ void __launch_bounds__(256) k_pq_gather(const uint32_t* __restrict__ beta, const uint32_t* __restrict__ list, uint32_t n_list, uint32_t rho, uint32_t* __restrict__ out) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (uint64_t)n_list * rho) return;
    const uint32_t k = (uint32_t)(x / rho), c = (uint32_t)(x - (uint64_t)k * rho);
    out[x] = beta[(uint64_t)list[k] * rho + c];
}

// Workgroup x: rows [x T, x T + T).  mode MA_COUNT: totals[2 e] += free rows of relation e, totals[2 e + 1] += flat rows, table[e * NB + x] = the
// free rows; mode MA_LIST: rows[e * R + rank] = the rank-th free row of relation e < i_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_pq_enforce(PqArgs pa, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                    uint32_t i_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t pq_lds[];
    const RaArgs& a = pa.r;
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6, w = a.width, E = pa.E, T = a.T, S = (T + 2u) | 1u;
    uint32_t* fa = pq_lds + 8;     // [NW][E] count: the wave's free rows of the relation; list: the free bits of the round's rows
    uint32_t* fl = fa + NW * E;    // [NW][E] count: the wave's flat rows
    uint32_t* need = fl + NW * E;  // [E]
    uint32_t* running = need + E;  // [E]
    uint32_t* goff = running + E;  // [GE + 1] the staged group's offsets
    uint32_t* gw = goff + pa.GE + 1u;  // [GW] its words
    uint32_t* tm = gw + pa.GW;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S + wave * ra_wave_words(w, a.K, a.n_regs, CHIP == CA_INTERPRET);
    RaWave W;
    W.w = w; W.BS = w | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.nzf = W.row_of + w; W.nxt = W.nzf + w; W.irow = W.nxt + w; W.basis = W.irow + w; W.raw = W.basis + w * W.BS;
    W.regs = W.raw + a.K * w + lane;
    for (uint32_t x = t; x < 8u + (2u * NW + 2u) * E; x += NT) pq_lds[x] = 0;
    __syncthreads();
    if (mode == MA_LIST) {
        for (uint32_t e = t; e < E && e < i_cut; e += NT)
            if (table[(uint64_t)e * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)e * a.NB + blockIdx.x] < R) { need[e] = 1; pq_lds[0] = 1; }
        __syncthreads();
        if (!pq_lds[0]) return;  // the whole workgroup
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
    uint32_t staged = RA_NONE;  // the group in LDS
    unsigned long long piv[3] = {0, 0, 0};  // the pivot columns of the wave's basis (wave-uniform)
    for (uint32_t i = 0; i < a.RPW; i++) {
        const uint32_t j = i * NW + wave;
        const uint64_t r = base + j;
        const bool active = j < rows_here;  // wave-uniform
        if (active) {
            bool reuse = false;
            if (CHIP == MA_BUS_ONLY && a.wr[0] <= 32u) {
                // a chip without constraints keeps the basis while its live set is unchanged (the rank audit's rule)
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
                // the two row buffers become the gradients': all zero between two relations
                for (uint32_t col = lane; col < w; col += 64u) { W.irow[col] = 0; W.nxt[col] = 0; }
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const uint32_t col = lane + 64u * (uint32_t)q;
                    piv[q] = ra_ballot(col < w && W.row_of[col] != RA_NONE, W.slot);
                }
                ra_wave_sync();
            }
        }
        for (uint32_t g = 0; g < pa.G; g++) {
            const uint32_t e0 = pa.gstart[g], e1 = pa.gstart[g + 1], o0 = pa.eoff[e0];
            if (staged != g) {  // the whole workgroup
                __syncthreads();
                for (uint32_t x = t; x <= e1 - e0; x += NT) goff[x] = pa.eoff[e0 + x] - o0;
                for (uint32_t x = t; x < pa.eoff[e1] - o0; x += NT) gw[x] = pa.ewords[o0 + x];
                __syncthreads();
                staged = g;
            }
            if (!active) continue;
            for (uint32_t e = e0; e < e1; e++) {
                // g_r of the relation into the buffer of its parity: the list names every column of beta's support and i and j, each once, so
                // one scatter builds it; the lanes that wrote it clear it after the verdict, and the next relation takes the other buffer
                uint32_t* gr = (e & 1u) ? W.nxt : W.irow;
                const uint32_t* en = gw + goff[e - e0];
                const uint32_t ci = en[0], cj = en[1], nt = (goff[e - e0 + 1] - goff[e - e0] - 2u) >> 1;
                const Fp xi = Fp::raw(tm[ci * S + j + 1]), xj = Fp::raw(tm[cj * S + j + 1]);
                for (uint32_t k = lane; k < nt; k += 64u) {
                    const uint32_t col = en[2 + 2 * k];
                    Fp v = Fp::raw(en[3 + 2 * k]);
                    if (col == ci) v += xj;
                    if (col == cj) v += xi;
                    gr[col] = v.v;
                }
                ra_wave_sync();
                unsigned long long nzb[3] = {0, 0, 0};
                for (uint32_t q = 0; q < W.WPL; q++) {
                    const uint32_t col = lane + 64u * q;
                    nzb[q] = ra_ballot(col < w && gr[col] != 0, W.slot);
                }
                const bool flat = (nzb[0] | nzb[1] | nzb[2]) == 0;
                bool fr = false;
                if (!flat && W.rho != w) {
                    // one reduce-only sweep against the reduced basis (the invariant audit's): the coefficients are all read before any update
                    bool left = false;
                    for (uint32_t wd = 0; wd < W.WPL; wd++) {
                        const uint32_t col = lane + 64u * wd;
                        if (col >= w) continue;
                        Fp acc = Fp::raw(gr[col]);
#pragma unroll
                        for (int q = 0; q < 3; q++) RA_EACH_BIT(nzb[q] & piv[q], q, p, acc -= Fp::raw(gr[p]) * Fp::raw(W.basis[p * W.BS + col]);)
                        left |= !acc.is_zero();
                    }
                    fr = ra_ballot(left, W.slot) != 0;
                }
                if (lane == 0) {
                    if (mode == MA_COUNT) { fa[wave * E + e] += fr ? 1u : 0u; fl[wave * E + e] += flat ? 1u : 0u; }
                    else fa[wave * E + e] = fr ? 1u : 0u;
                }
                // every read of gr feeds a ballot above: they are done
                for (uint32_t k = lane; k < nt; k += 64u) gr[en[2 + 2 * k]] = 0;
            }
            ra_wave_sync();
        }
        if (mode != MA_LIST) continue;
        if (!active)
            for (uint32_t e = lane; e < E; e += 64u) fa[wave * E + e] = 0;
        __syncthreads();
        if (active) {
            for (uint32_t e = lane; e < E && e < i_cut; e += 64u) {
                if (need[e] == 0 || fa[wave * E + e] == 0) continue;
                uint32_t rank = prefix[(uint64_t)e * a.NB + blockIdx.x] + running[e];
                for (uint32_t x = 0; x < wave; x++) rank += fa[x * E + e];
                if (rank < R) rows[(uint64_t)e * R + rank] = (uint32_t)r;
            }
        }
        __syncthreads();
        if (wave == 0)
            for (uint32_t e = lane; e < E; e += 64u) {
                uint32_t s = 0;
                for (uint32_t x = 0; x < NW; x++) s += fa[x * E + e];
                running[e] += s;
            }
        __syncthreads();
    }
    if (mode != MA_COUNT) return;
    __syncthreads();
    for (uint32_t e = t; e < E; e += NT) {
        uint32_t f = 0, z = 0;
        for (uint32_t x = 0; x < NW; x++) { f += fa[x * E + e]; z += fl[x * E + e]; }
        if (f) { atomicAdd(&totals[2 * e], (unsigned long long)f); table[(uint64_t)e * a.NB + blockIdx.x] = f; }
        if (z) atomicAdd(&totals[2 * e + 1], (unsigned long long)z);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static size_t pq_rows_lds_bytes(uint32_t rho) { return 4 * (size_t)pq_rows_lds_words(rho); }
static size_t pq_solve_lds_bytes(uint32_t rho) { return 4 * (16 + (size_t)rho + (pq_solve_in_lds(rho) ? 2 * (size_t)rho * rho : 0)); }
static size_t pq_sweep_lds_bytes(uint32_t rho) { return 4 * (2 * (size_t)PQ_TILE_PAIRS + (size_t)rho * PQ_TILE_ROWS + (size_t)PQ_TILE_PAIRS * rho); }

void pq_rows_shape(PqArgs& pa) {
    const RaArgs& a = pa.r;
    // slices of whole tiles of rows: at most IA_MAX_WORKGROUPS (the invariant audit's rule)
    const uint64_t tiles = (a.n + IA_TILE_ROWS - 1) / IA_TILE_ROWS;
    const uint64_t per = (tiles + IA_MAX_WORKGROUPS - 1) / IA_MAX_WORKGROUPS;
    pa.RS = (uint32_t)(per * IA_TILE_ROWS);
    pa.NB2 = (uint32_t)((a.n + pa.RS - 1) / pa.RS);
}

size_t pq_lds_bytes(const PqArgs& pa, uint32_t NW, uint32_t T) {
    const RaArgs& a = pa.r;
    const size_t S = (T + 2u) | 1u;
    const size_t own = 4 * (8 + (size_t)(2 * NW + 2) * pa.E + pa.GE + 1 + pa.GW + ((size_t)a.width + a.prep_width) * S +
                            (size_t)NW * ra_wave_words(a.width, a.K, a.n_regs, a.native_chip == CA_INTERPRET));
    // never less than the rank audit's bytes for the same shape: the listing pass goes through launch_ra_scan, which checks those
    return std::max(own, ra_lds_bytes(a, NW, T));
}

void pq_shape(PqArgs& pa) {
    RaArgs& a = pa.r;
    const size_t LDS = 160 * 1024;
    if (a.width > IA_MAX_WIDTH || pq_lds_bytes(pa, 1, 1) > LDS)
        throw std::invalid_argument("product_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints, " +
                                    std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) + " interpreted registers and " + std::to_string(pa.E) +
                                    " relations does not fit a workgroup's LDS with one wave (" + std::to_string(pq_lds_bytes(pa, 1, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + 128 per register + 4 w + 12 + 3 (w + prep w) + 4 E of counters + the staged group of " +
                                    std::to_string(pa.GE) + " relations and " + std::to_string(pa.GW) + " words + 1), 163840 at most; at most 191 columns)");
    // the most waves per CU; among equals the larger workgroup (fewer tiles staged): rank_audit.hip's rule
    uint32_t best = 1, best_waves = 0;
    for (uint32_t nw = 4; nw >= 1; nw >>= 1) {
        uint32_t rpw = 16;
        while (rpw > 1 && (a.n / ((uint64_t)nw * rpw) < 1024 || pq_lds_bytes(pa, nw, nw * rpw) > LDS)) rpw >>= 1;
        const size_t b = pq_lds_bytes(pa, nw, nw * rpw);
        if (b > LDS) continue;
        const uint32_t waves = (uint32_t)(LDS / b) * nw;
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    a.NW = best;
    uint32_t rpw = 16;
    while (rpw > 1 && (a.n / ((uint64_t)a.NW * rpw) < 1024 || pq_lds_bytes(pa, a.NW, a.NW * rpw) > LDS)) rpw >>= 1;
    a.RPW = rpw;
    a.T = a.NW * a.RPW;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define PQ_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

// the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
static void pq_opt_in() {
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("product_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("product_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) +
                                     ": " + hipGetErrorString(e));
    };
    opt_in((const void*)k_pq_rows, "k_pq_rows");
    opt_in((const void*)k_pq_rowmerge, "k_pq_rowmerge");
    opt_in((const void*)k_pq_solve, "k_pq_solve");
    opt_in((const void*)k_pq_sweep, "k_pq_sweep");
#define PQ_X(C) opt_in((const void*)k_pq_enforce<vchips::C>, "k_pq_enforce<" #C ">");
    PQ_CHIPS(PQ_X)
#undef PQ_X
    opt_in((const void*)k_pq_enforce<CA_INTERPRET>, "k_pq_enforce<CA_INTERPRET>");
    opt_in((const void*)k_pq_enforce<MA_BUS_ONLY>, "k_pq_enforce<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

// what every launch before the enforcement phase takes: the space and, where given, the slices
static void pq_space_check(const PqArgs& pa, bool slices) {
    const RaArgs& a = pa.r;
    if (a.width == 0 || a.width > IA_MAX_WIDTH || pa.rho < 2 || pa.rho > a.width + 1u || !pa.pcols) throw std::logic_error("product_audit: 1 to 191 columns, 2 to w + 1 pivot columns");
    if (a.n == 0 || (slices && (pa.RS == 0 || pa.NB2 == 0 || pa.NB2 != (uint32_t)((a.n + pa.RS - 1) / pa.RS)))) throw std::logic_error("product_audit: inconsistent basis-row launch shape");
    if (pq_rows_lds_bytes(pa.rho) > 160 * 1024 || pq_sweep_lds_bytes(pa.rho) > 160 * 1024) throw std::logic_error("product_audit: the space does not fit the LDS");
    pq_opt_in();
}

void launch_pq_rows(hipStream_t st, const PqArgs& pa, uint32_t* part) {
    pq_space_check(pa, true);
    ProfScope ps("k_pq_rows", st, 4.0 * (double)pa.r.n * pa.rho);
    VK_LAUNCH(k_pq_rows, dim3(pa.NB2), dim3(64), pq_rows_lds_bytes(pa.rho), st, pa.r.main, pa.r.mstride, pa.r.n, pa.rho, pa.pcols, pa.RS, part);
}

void launch_pq_rowmerge(hipStream_t st, const PqArgs& pa, uint32_t* part, uint32_t* rows) {
    pq_space_check(pa, true);
    ProfScope ps("k_pq_rowmerge", st, 4.0 * (double)pq_rows_words(pa));
    // a tree of fan IA_MERGE_FAN: the levels ping-pong between the slices' slots and the spare slots behind them (launch.hpp: pq_rows_words)
    const uint64_t slot = pa.rho + 1ull;
    uint32_t *src = part, *dst = part + (uint64_t)pa.NB2 * slot;
    uint32_t n = pa.NB2;
    while (n > IA_MERGE_FAN) {
        const uint32_t m = (n + IA_MERGE_FAN - 1) / IA_MERGE_FAN;
        VK_LAUNCH(k_pq_rowmerge, dim3(m), dim3(64), pq_rows_lds_bytes(pa.rho), st, pa.r.main, pa.r.mstride, pa.rho, pa.pcols, src, n, IA_MERGE_FAN, dst);
        std::swap(src, dst);
        n = m;
    }
    VK_LAUNCH(k_pq_rowmerge, dim3(1), dim3(64), pq_rows_lds_bytes(pa.rho), st, pa.r.main, pa.r.mstride, pa.rho, pa.pcols, src, n, IA_MERGE_FAN, rows);
}

void launch_pq_solve(hipStream_t st, const PqArgs& pa, const uint32_t* rows, uint32_t* aug, uint32_t* G, uint32_t* inv, uint32_t* status) {
    pq_space_check(pa, false);
    if (!aug && !pq_solve_in_lds(pa.rho)) throw std::logic_error("product_audit: the inverse of this many columns needs scratch");
    ProfScope ps("k_pq_solve", st, 8.0 * (double)pa.rho * pa.rho);
    VK_LAUNCH(k_pq_solve, dim3(1), dim3(256), pq_solve_lds_bytes(pa.rho), st, pa.r.main, pa.r.mstride, pa.rho, pa.pcols, rows, pq_solve_in_lds(pa.rho) ? nullptr : aug, G, inv, status);
}

void launch_pq_beta(hipStream_t st, const PqArgs& pa, const uint32_t* G, const uint32_t* inv, uint32_t* beta, uint32_t* flags) {
    pq_space_check(pa, false);
    const uint32_t m = (uint32_t)pq_pairs(pa.rho);
    ProfScope ps("k_pq_beta", st, 4.0 * (double)m * pa.rho);
    VK_LAUNCH(k_pq_beta, dim3((m + 255u) / 256u), dim3(256), 0, st, G, inv, pa.rho, m, beta, flags);
}

void launch_pq_sweep(hipStream_t st, const PqArgs& pa, const char* name, uint64_t n_rows, const uint32_t* beta, const uint32_t* list, uint32_t n_list, uint32_t* flags) {
    pq_space_check(pa, false);
    if (n_rows == 0 || n_rows > pa.r.n || n_list > pq_pairs(pa.rho)) throw std::logic_error("product_audit: the sweep's rows and pairs are those of the chip");
    if (!n_list) return;
    ProfScope ps(name, st, 4.0 * (double)n_rows * pa.rho);
    const dim3 grid((uint32_t)((n_rows + PQ_TILE_ROWS - 1) / PQ_TILE_ROWS), (n_list + PQ_TILE_PAIRS - 1) / PQ_TILE_PAIRS);
    VK_LAUNCH(k_pq_sweep, grid, dim3(256), pq_sweep_lds_bytes(pa.rho), st, pa.r.main, pa.r.mstride, n_rows, pa.rho, pa.pcols, beta, list, n_list, flags);
}

void launch_pq_compact(hipStream_t st, const uint32_t* flags, const uint32_t* list, uint32_t n_in, uint32_t* out, uint32_t* count) {
    ProfScope ps("k_pq_compact", st, 8.0 * (double)n_in);
    VK_LAUNCH(k_pq_compact, dim3(1), dim3(256), 256 * 4, st, flags, list, n_in, out, count);
}

void launch_pq_gather(hipStream_t st, const PqArgs& pa, const uint32_t* beta, const uint32_t* list, uint32_t n_list, uint32_t* out) {
    if (!n_list) return;
    ProfScope ps("k_pq_gather", st, 8.0 * (double)n_list * pa.rho);
    const uint64_t words = (uint64_t)n_list * pa.rho;
    VK_LAUNCH(k_pq_gather, dim3((uint32_t)((words + 255u) / 256u)), dim3(256), 0, st, beta, list, n_list, pa.rho, out);
}

static void pq_check(const PqArgs& pa) {
    const RaArgs& a = pa.r;
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("product_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > IA_MAX_WIDTH || pa.E == 0 || pa.G == 0 || !pa.eoff || !pa.ewords || !pa.gstart) throw std::logic_error("product_audit: 1 to 191 columns and at least one relation");
    if (a.n == 0 || (a.n & (a.n - 1)) || (a.NW != 1 && a.NW != 2 && a.NW != 4) || a.RPW == 0 || a.T != a.NW * a.RPW || a.NB != (uint32_t)((a.n + a.T - 1) / a.T))
        throw std::logic_error("product_audit: inconsistent launch shape");
    if (pq_lds_bytes(pa, a.NW, a.T) > 160 * 1024) throw std::logic_error("product_audit: the launch shape does not fit the LDS");
    pq_opt_in();
}

static void pq_launch(hipStream_t st, const PqArgs& pa, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows) {
    const RaArgs& a = pa.r;
    const dim3 grid(a.NB), block(64 * a.NW);
    const size_t lds = pq_lds_bytes(pa, a.NW, a.T);
    switch (a.native_chip) {
#define PQ_X(C) case vchips::C: VK_LAUNCH((k_pq_enforce<vchips::C>), grid, block, lds, st, pa, mode, totals, table, prefix, i_cut, R, rows); break;
        PQ_CHIPS(PQ_X)
#undef PQ_X
        case CA_INTERPRET: VK_LAUNCH((k_pq_enforce<CA_INTERPRET>), grid, block, lds, st, pa, mode, totals, table, prefix, i_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_pq_enforce<MA_BUS_ONLY>), grid, block, lds, st, pa, mode, totals, table, prefix, i_cut, R, rows); break;
        default: throw std::logic_error("product_audit: a native chip id without constraints");
    }
}

void launch_pq_count(hipStream_t st, const PqArgs& pa, unsigned long long* totals, uint32_t* table) {
    pq_check(pa);
    static const char* names[14] = {"k_pq_count.cpu", "k_pq_count.program", "k_pq_count.mem", "k_pq_count.add", "k_pq_count.sub", "k_pq_count.mul", "k_pq_count.div", "k_pq_count.shift",
                                    "k_pq_count.lt", "k_pq_count.com", "k_pq_count.bitwise", "k_pq_count.output", "k_pq_count.range", "k_pq_count.static_data"};
    const int id = pa.r.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_pq_count.bus" : "k_pq_count");
    ProfScope ps(name, st, 4.0 * (double)pa.r.n * (pa.r.width + pa.r.prep_width), pa.r.evaluations);
    pq_launch(st, pa, MA_COUNT, totals, table, nullptr, 0, 0, nullptr);
}

void launch_pq_list(hipStream_t st, const PqArgs& pa, const uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows) {
    pq_check(pa);
    ProfScope ps("k_pq_list", st, 0);
    pq_launch(st, pa, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, i_cut, R, rows);
}

}  // namespace vk
