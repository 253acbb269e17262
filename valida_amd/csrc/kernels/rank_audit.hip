// Rank audit on the device (host/rank_audit.hpp states the contract): per trace row the reduced row echelon form of the Jacobian of
// everything that reads the row's w main cells — constraints at the row and at the row before, and the interactions' records — and from it
// the rank, the zero columns, the loose / pinned / coupled columns and the canonical null vectors.
//   shape    one WAVE per trace row, lane l <-> columns l, l + 64, l + 128 (WPL = ceil(w / 64) words per lane, at most 3); NW waves per
//            workgroup, each wave RPW rows one after the other: a workgroup owns T = NW RPW consecutive rows.  A chip of few rows gets fewer
//            rows per wave so that it still makes many workgroups; a chip of height 1 runs on one wave: its Jacobian rows are not split
//            over workgroups (that would need a second elimination of the partial bases to keep the RREF unique) — the latency is accepted.
//   tile     the workgroup's rows, halo and wrap staged once as [column][S], S = (T + 2) | 1 ODD: a wave reads one row, so the lanes of a
//            wave read the same word (a broadcast) during Air::eval and different columns of the same row elsewhere — with an odd column
//            stride those 64 reads fall into 64 different words of 32 banks, 2 per bank and group of 32 lanes: conflict-free.
//   eval     JetFolder: Expr = (value, derivative); + and - componentwise, (a b).d = a.v b.d + a.d b.v; main(col, next) seeds d = 1 where
//            (col, next) is this lane's cell — a per-lane compare-select.  vchips::eval_chip<CHIP> runs once per lane word at q = r (cell as
//            local; n = 1: also as next) and once at q = r - 1 (cell as next); every assert_zero leaves one Jacobian row spread across the
//            wave, kept in LDS raw[k][column].  Captured AIRs run the register program with (v, d) registers in LDS (CA_INTERPRET); a chip
//            without constraints (MA_BUS_ONLY) evaluates nothing.  The interaction rows come from the host's weight rows (ra_weight_rows),
//            the count of each interaction is evaluated once per row for liveness.
//   basis    the wave keeps its reduced basis in LDS as [w][BS], BS = w | 1: the row of pivot column p is row p (row_of[p] flags it).  A new row is skipped when its ballot is
//            empty; otherwise reduced against the pivots it touches (ballot of pivot lanes with a non-zero entry; per hit one LDS broadcast
//            of the coefficient and one multiply-subtract per lane — the other pivot entries of a REDUCED basis row are zero, so every
//            coefficient can be read before any update), normalised by one field inversion, and its pivot column cleared from the older rows
//            that hold it (ballot again).  Once rho = w the wave skips everything that is left of the row, wave-uniformly (no column is zero
//            then).  Zero columns: the complement of the OR of the raw rows' non-zero flags.
//   count    per-column loose / zero / coupled rows by LDS atomics per workgroup, then integer atomics on the chip's totals; the coupled
//            count also goes into table[column][workgroup].
//   scan     exclusive prefix of the table over workgroups, per listed column.
//   list     workgroups that hold a coupled row of rank < R of a listed column eliminate their rows again; the waves of a round exchange
//            their coupled bits through LDS so that rank = prefix + rows before in the workgroup, and the wave that owns the row writes the
//            canonical null vector while its basis is still there.  No atomic admits a row.
// Wave primitives: ra_ballot and ra_wave_sync (lane broadcasts are LDS reads of one address after ra_wave_sync).  An emulation without waves
// defines VGPU_RA_WAVE_PRIMS and supplies both through LDS and __syncthreads() for 64-thread workgroups (tests/emu/rank_audit_emu.cpp).
// LDS (u32 words): 8 + (5 + NW) w (sums, counters, need, running, coupled bits) + (w + prep w) S (tile) + per wave 4 + 4 w (row_of, non-zero
// flags, two row buffers) + w BS (basis) + K w (raw rows) + 128 registers (interpreted: (v, d) x 64 lanes).
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, columns of programs
// and interactions are below the width, rows written by `list` have ranks below R and columns below the width).
#include <mutex>
#include <stdexcept>
#include <string>
#include "rank_elim.hpp"

namespace vk {

// Workgroup x: rows [x T, x T + T).  mode MA_COUNT: totals (launch.hpp: RaArgs) and table[c * NB + x] = coupled rows of column c; mode MA_LIST:
// rows[(c * R + rank) * 18 ..] = the rank-th coupled row of column c < c_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_ra_audit(RaArgs a, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                  uint32_t c_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t ra_lds[];
    const uint32_t NT = blockDim.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6, NW = NT >> 6, w = a.width, T = a.T, S = (T + 2u) | 1u;
    uint32_t* sums = ra_lds + 1;  // nullity, zero columns, coupled rows, max nullity
    uint32_t* cnt = ra_lds + 8;   // [3][w] loose, zero, coupled rows of the column
    uint32_t* need = cnt + 3 * w;
    uint32_t* running = need + w;
    uint32_t* cb = running + w;   // [NW][w] the coupled bits of the round's rows
    uint32_t* tm = cb + NW * w;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S + wave * ra_wave_words(w, a.K, a.n_regs, CHIP == CA_INTERPRET);
    RaWave W;
    W.w = w; W.BS = w | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.nzf = W.row_of + w; W.nxt = W.nzf + w; W.irow = W.nxt + w; W.basis = W.irow + w; W.raw = W.basis + w * W.BS;
    W.regs = W.raw + a.K * w + lane;
    for (uint32_t x = t; x < 8u + (5u + NW) * w; x += NT) ra_lds[x] = 0;
    __syncthreads();
    if (mode == MA_LIST) {
        for (uint32_t c = t; c < w && c < c_cut; c += NT)
            if (table[(uint64_t)c * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)c * a.NB + blockIdx.x] < R) { need[c] = 1; ra_lds[0] = 1; }
        __syncthreads();
        if (!ra_lds[0]) return;  // the whole workgroup
    }
    // the tile: word j of a column is row (base + j - 1) mod n, j = 0 .. rows_here + 1
    const uint64_t base = (uint64_t)blockIdx.x * T;
    const uint32_t rows_here = a.n - base < T ? (uint32_t)(a.n - base) : T;
    // one loop over (column, j): every thread of the workgroup loads, whatever the tile's height
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

    // A chip without constraints has a Jacobian that depends on the row only through WHICH interactions are live: a row with the live set of
    // the wave's row before keeps that row's basis and flags (the same matrix, so the same RREF; up to 32 interactions).
    uint32_t live_prev = 0, lz = 0, z = 0;  // lz: bit q this lane's column of word q is loose, bit 3 + q it is zero
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
                ra_row<CHIP>(a, W, tm, tp, S, j, r);
                lz = 0; z = 0;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const uint32_t col = lane + 64u * (uint32_t)q;
                    bool zero = false;
                    if (col < w) {
                        zero = W.rho != w && W.nzf[col] == 0;
                        lz |= (ra_pinned(W, col) ? 0u : 1u << q) | (zero ? 8u << q : 0u);
                    }
                    z += (uint32_t)__builtin_popcountll(ra_ballot(zero, W.slot));
                }
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint32_t col = lane + 64u * (uint32_t)q;
                if (col >= w) continue;
                const bool loose = (lz >> q) & 1u, zero = (lz >> (3 + q)) & 1u;
                if (mode == MA_COUNT) {
                    if (loose) atomicAdd(&cnt[col], 1u);
                    if (zero) atomicAdd(&cnt[w + col], 1u);
                    if (loose && !zero) atomicAdd(&cnt[2 * w + col], 1u);
                } else {
                    cb[wave * w + col] = loose && !zero ? 1u : 0u;
                }
            }
            if (mode == MA_COUNT && lane == 0) {
                const uint32_t nu = w - W.rho;
                atomicAdd(&sums[0], nu);
                atomicAdd(&sums[1], z);
                if (nu > z) atomicAdd(&sums[2], 1u);
                atomicMax(&sums[3], nu);
            }
        } else if (mode == MA_LIST) {
            for (uint32_t col = lane; col < w; col += 64u) cb[wave * w + col] = 0;
        }
        if (mode != MA_LIST) continue;
        __syncthreads();
        if (active) {
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
                RA_EACH_BIT(m, q, c, ra_emit(W, c, (uint32_t)r, rows + ((uint64_t)c * R + W.nxt[c]) * RA_OUT_WORDS);)
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
        if (cnt[c]) atomicAdd(&totals[4 + 2 * c], (unsigned long long)cnt[c]);
        if (cnt[w + c]) atomicAdd(&totals[5 + 2 * c], (unsigned long long)cnt[w + c]);
        if (cnt[2 * w + c]) table[(uint64_t)c * a.NB + blockIdx.x] = cnt[2 * w + c];
    }
    if (t < 3 && sums[t]) atomicAdd(&totals[t], (unsigned long long)sums[t]);
    if (t == 3 && sums[3]) atomicMax(&totals[3], (unsigned long long)sums[3]);
}

// scan: block c of the grid handles column c: prefix[c][x] = sum of table[c][x' < x]
__global__ void __launch_bounds__(256) k_ra_scan(const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB) {
    extern __shared__ uint32_t ra_lds[];  // [256] partial sums
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)c * NB;
    uint32_t s = 0;
    for (uint32_t x = lo; x < hi; x++) s += row[x];
    ra_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = ra_lds[i]; ra_lds[i] = run; run += x; }
    }
    __syncthreads();
    uint32_t run = ra_lds[t];
    uint32_t* out = prefix + (uint64_t)c * NB;
    for (uint32_t x = lo; x < hi; x++) { out[x] = run; run += row[x]; }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t ra_lds_bytes(const RaArgs& a, uint32_t NW, uint32_t T) {
    const size_t S = (T + 2u) | 1u;
    return 4 * (8 + (size_t)(5 + NW) * a.width + ((size_t)a.width + a.prep_width) * S + (size_t)NW * ra_wave_words(a.width, a.K, a.n_regs, a.native_chip == CA_INTERPRET));
}

void ra_shape(RaArgs& a) {
    const size_t LDS = 160 * 1024;
    if (a.width > 192 || ra_lds_bytes(a, 1, 1) > LDS)
        throw std::invalid_argument("rank_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints and " +
                                    std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) + " interpreted registers does not fit a workgroup's LDS with one wave (" +
                                    std::to_string(ra_lds_bytes(a, 1, 1)) + " bytes: 4 x (basis w (w | 1) + raw rows K w + 128 per register + 10 w + 12 + 3 (w + prep w)), 163840 at most; at most 192 columns)");
    // the most waves per CU; among equals the larger workgroup (fewer tiles staged)
    uint32_t best = 1, best_waves = 0;
    for (uint32_t nw = 4; nw >= 1; nw >>= 1) {
        uint32_t rpw = 16;
        while (rpw > 1 && (a.n / ((uint64_t)nw * rpw) < 1024 || ra_lds_bytes(a, nw, nw * rpw) > LDS)) rpw >>= 1;
        const size_t b = ra_lds_bytes(a, nw, nw * rpw);
        if (b > LDS) continue;
        const uint32_t waves = (uint32_t)(LDS / b) * nw;
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    a.NW = best;
    uint32_t rpw = 16;
    while (rpw > 1 && (a.n / ((uint64_t)a.NW * rpw) < 1024 || ra_lds_bytes(a, a.NW, a.NW * rpw) > LDS)) rpw >>= 1;
    a.RPW = rpw;
    a.T = a.NW * a.RPW;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define RA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void ra_check(const RaArgs& a) {
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("rank_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > 192) throw std::logic_error("rank_audit: 1 to 192 columns");
    if (a.n == 0 || (a.n & (a.n - 1)) || (a.NW != 1 && a.NW != 2 && a.NW != 4) || a.RPW == 0 || a.T != a.NW * a.RPW || a.NB != (uint32_t)((a.n + a.T - 1) / a.T))
        throw std::logic_error("rank_audit: inconsistent launch shape");
    if (ra_lds_bytes(a, a.NW, a.T) > 160 * 1024) throw std::logic_error("rank_audit: the launch shape does not fit the LDS");
    // the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("rank_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    // a failed opt-in is reported here, by name, and the device is not marked: the launch after it would only name the kernel
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("rank_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) + ": " +
                                     hipGetErrorString(e));
    };
#define RA_X(C) opt_in((const void*)k_ra_audit<vchips::C>, "k_ra_audit<" #C ">");
    RA_CHIPS(RA_X)
#undef RA_X
    opt_in((const void*)k_ra_audit<CA_INTERPRET>, "k_ra_audit<CA_INTERPRET>");
    opt_in((const void*)k_ra_audit<MA_BUS_ONLY>, "k_ra_audit<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

static void ra_launch(hipStream_t st, const RaArgs& a, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows) {
    const dim3 grid(a.NB), block(64 * a.NW);
    const size_t lds = ra_lds_bytes(a, a.NW, a.T);
    switch (a.native_chip) {
#define RA_X(C) case vchips::C: VK_LAUNCH((k_ra_audit<vchips::C>), grid, block, lds, st, a, mode, totals, table, prefix, c_cut, R, rows); break;
        RA_CHIPS(RA_X)
#undef RA_X
        case CA_INTERPRET: VK_LAUNCH((k_ra_audit<CA_INTERPRET>), grid, block, lds, st, a, mode, totals, table, prefix, c_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_ra_audit<MA_BUS_ONLY>), grid, block, lds, st, a, mode, totals, table, prefix, c_cut, R, rows); break;
        default: throw std::logic_error("rank_audit: a native chip id without constraints");
    }
}

void launch_ra_count(hipStream_t st, const RaArgs& a, unsigned long long* totals, uint32_t* table) {
    ra_check(a);
    static const char* names[14] = {"k_ra_count.cpu", "k_ra_count.program", "k_ra_count.mem", "k_ra_count.add", "k_ra_count.sub", "k_ra_count.mul", "k_ra_count.div", "k_ra_count.shift",
                                    "k_ra_count.lt", "k_ra_count.com", "k_ra_count.bitwise", "k_ra_count.output", "k_ra_count.range", "k_ra_count.static_data"};
    const int id = a.native_chip;
    const char* name = id >= 0 && id < 14 ? names[id] : (id == MA_BUS_ONLY ? "k_ra_count.bus" : "k_ra_count");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width), a.evaluations);  // the profile's per-chip split: dual row evaluations as its ops
    ra_launch(st, a, MA_COUNT, totals, table, nullptr, 0, 0, nullptr);
}

void launch_ra_scan(hipStream_t st, const RaArgs& a, const uint32_t* table, uint32_t* prefix, uint32_t c_cut) {
    ra_check(a);
    if (!c_cut) return;
    ProfScope ps("k_ra_scan", st, 8.0 * (double)a.NB * c_cut);
    VK_LAUNCH(k_ra_scan, dim3(c_cut), dim3(256), 256 * 4, st, table, prefix, a.NB);
}

void launch_ra_list(hipStream_t st, const RaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows) {
    ra_check(a);
    ProfScope ps("k_ra_list", st, 0);
    ra_launch(st, a, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, c_cut, R, rows);
}

}  // namespace vk
