// Mutation audit on the device (host/mutation_audit.hpp states the contract): which cells of a witness could be changed by a delta without any
// AIR constraint or bus record noticing.  One launch family per chip; one thread per trace row r owns the mutations of row r's cells: for every
// (column c, delta d) it evaluates Air::eval with the cell changed at row r (the cell is `local`) and at row r - 1 (the cell is `next`), keeps
// only the three-word fail mask, and compares it with the baseline masks of those two rows, which it computed itself first; the bus rule comes
// from the chip's interaction descriptors (`bus` below).  The evaluation code (fail mask, folder, ma_eval, the interaction walk) is in
// mutation_eval.hpp, shared with the coverage audit (coverage_audit.hip).
//   tile    a row is read by up to 2 w D + 2 evaluations, so the workgroup's T rows plus the halo rows r - 1 and r + 1 at its edges (the wrap at
//           rows 0 and n - 1 included) are staged ONCE into LDS with coalesced column loads, [column][T + 2], main and preprocessed; every
//           evaluation reads LDS (a thread's reads of a column are consecutive words: no bank conflict).  cpu is 51 + 0 columns (52.6 KB at
//           T = 256), bitwise 79 (81.5 KB).
//   eval    the BasicMachine chips: vchips::eval_chip<CHIP> over a folder whose main(col, next) adds the delta when (col, next) is the mutated
//           cell and whose assert_zero sets bit k of the mask; ONE inlined copy per kernel (baselines and mutations are iterations of one loop).
//           Captured AIRs: the register program interpreted with its register file in LDS beside the tile.  A chip without constraints
//           (MA_BUS_ONLY) evaluates nothing.  Columns that the compiled Program never reads as local / next, or no interaction reads, skip
//           that evaluation (MaArgs::flags; wave-uniform).
//   bus     the counts of the row's interactions are evaluated once per row from the descriptors (eval_vcol's walk, on the tile): `live`, the
//           interactions that are records.  What a mutation does to a record needs no evaluation: a virtual column is affine with constant
//           weights, so two masks per column (host/mutation_audit.hpp: ma_bus_masks) say which interactions' count and which interactions'
//           fields change; detected iff the first is non-zero or the second meets `live`.  A chip of more than 32 interactions evaluates every
//           interaction before and after every mutation instead (ma_bus_detected, the definition itself).
//   slices  a chip of few workgroups is split over gridDim.y column slices (ma_column_slices: about 2048 workgroups per launch), so that a chip
//           of height 1 does not run its 2 w D + 2 evaluations on one thread; every slice stages the tile and evaluates the baselines again.
//   count   per entry (column, delta) the free / air / bus rows are reduced per wave (ballot + population count), then per workgroup in LDS; one
//           integer atomic per non-zero (entry, kind, workgroup), and the free count goes into the table [entry][workgroup].
//   scan    exclusive prefix of the table over workgroups, per listed entry.
//   list    workgroups that hold a free row of rank < R of a listed entry run the evaluation again for those entries alone, keep one bit per
//           (entry, row) in LDS, and one thread per entry walks the bits in row order: rank = prefix + position.  No atomic admits a row: the listed rows are the
//           first R in ascending order whatever the scheduling was.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, the columns a program or
// an interaction reads are checked against the trace widths in mutation_audit_plan, rows written by `list` are below n and ranks below R).
#include <stdexcept>
#include <string>
#include "mutation_eval.hpp"

namespace vk {

#ifndef VGPU_MA_WAVE_ADD
// Adds the number of lanes of this wave whose `pred` holds to *counter (LDS) with one atomic.  Called from wave-uniform control flow only.
// (An emulation without waves supplies the same contract for a wave of one lane.)
__device__ __forceinline__ void ma_wave_add(uint32_t* counter, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (pred && (b & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) atomicAdd(counter, (uint32_t)__popcll(b));  // the lowest lane that has it
}
#endif

// LDS of k_ma_audit (dynamic, one array): [0] the listing pass's flag, then the accumulators (count: [E][3] counters; list: [E][T / 32] bits
// and [E] need flags), the main tile [width][T + 2], the preprocessed tile [prep_width][T + 2], the interpreter's register file [n_regs][T]
__host__ __device__ inline uint32_t ma_acc_words(uint32_t E, uint32_t T, uint32_t mode) { return mode == MA_LIST ? E * (T >> 5) + E : 3u * E; }

// Workgroup (x, y): rows [x T, x T + T) and the columns of slice y (a.CY slices of ceil(width / CY) columns: a chip of few rows still fills
// the device, at the price of the two baselines per slice).  mode MA_COUNT: totals[3 e + {0 free, 1 air, 2 bus}] and table[e * NB + x] = free
// rows; mode MA_LIST: rows[e * R + rank] = the rank-th free row of entry e < e_cut, rank < R.
template <int CHIP>
__global__ void __launch_bounds__(256) k_ma_audit(MaArgs a, uint32_t mode, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix,
                                                  uint32_t e_cut, uint32_t R, uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t ma_lds[];
    const uint32_t T = blockDim.x, t = threadIdx.x, S = T + 2, E = a.width * a.D, TW = T >> 5;
    const uint32_t cpb = (a.width + gridDim.y - 1) / gridDim.y;
    const uint32_t c_lo = blockIdx.y * cpb < a.width ? blockIdx.y * cpb : a.width, c_hi = c_lo + cpb < a.width ? c_lo + cpb : a.width;
    const uint32_t e_lo = c_lo * a.D, e_hi = c_hi * a.D;
    const uint32_t EL = e_hi < e_cut ? e_hi : e_cut;  // the slice's entries that are listed at all: [e_lo, EL)
    const uint32_t n_acc = ma_acc_words(E, T, mode);
    uint32_t* acc = ma_lds + 1;
    uint32_t* need = acc + E * TW;  // list: entry e is walked in this workgroup
    uint32_t* tm = acc + n_acc;
    uint32_t* tp = tm + a.width * S;
    uint32_t* regs = tp + a.prep_width * S + t;
    if (mode == MA_LIST) {
        if (t == 0) ma_lds[0] = 0;
        for (uint32_t x = t; x < n_acc; x += T) acc[x] = 0;
        __syncthreads();
        // entry e belongs to thread e mod T; it is walked here when it has a free row in this workgroup and still has ranks below R to hand out
        for (uint32_t e = e_lo + t; e < EL; e += T)
            if (table[(uint64_t)e * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)e * a.NB + blockIdx.x] < R) { need[e] = 1; ma_lds[0] = 1; }
        __syncthreads();
        if (!ma_lds[0]) return;  // the whole workgroup
    } else {
        for (uint32_t x = t; x < n_acc; x += T) acc[x] = 0;
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
    const bool active = r < a.n, single = a.n == 1;
    const Fp one = Fp::one(), zero = Fp::zero();
    // the interactions of row r that are records (count != 0): bit m.  With it the bus rule needs no evaluation per mutation (ma_bus_masks)
    uint32_t live = 0;
    if (active && !a.bus_walk) {
        const uint32_t M = a.iw[0];
        for (uint32_t m = 0; m < M; m++) {
            uint32_t pos = a.iw[2 + m] + 2;
            Fp c0, c1;
            ma_vcol2(a.iw, pos, tm + t + 1, tp + t + 1, S, 0xffffffffu, zero, c0, c1);
            live |= c0.is_zero() ? 0u : 1u << m;
        }
    }
    MaMask base0, base1;
    base0.clear(); base1.clear();
    bool air = false, wanted = true;
    // iterations 0, 1: the baselines of rows r and r - 1; then two per entry (column, delta) of the slice: the cell as local, the cell as next
    const uint32_t n_it = 2 + 2 * (e_hi - e_lo);
    uint32_t c = c_lo, di = 0;
    for (uint32_t it = 0; it < n_it; it++) {
        const bool is_base = it < 2;
        const uint32_t which = it & 1u;
        const uint32_t fl = is_base ? 3u : a.flags[c];
        if (mode == MA_LIST && !is_base && which == 0) wanted = need[c * a.D + di] != 0;  // LDS, wave-uniform: entries no list of this workgroup needs are skipped
        if (CHIP != MA_BUS_ONLY) {
            const bool run = wanted && (single ? (which == 0 && (fl & 3u)) : (which == 0 ? (fl & 1u) : (fl & 2u)));  // wave-uniform
            if (run && active) {
                // which = 0: the evaluation at row r (the cell is local; for n = 1 also next), 1: at row r - 1 (the cell is next)
                const uint32_t off = which ? 0u : 1u;
                const uint64_t qr = which ? rp : r;
                const Fp d = Fp::raw(a.delta[di]);
                MaRow q;
                q.lp = tm + t + off; q.np = q.lp + 1; q.plp = tp + t + off; q.pnp = q.plp + 1;
                q.S = S;
                q.first = qr == 0 ? one : zero; q.last = qr == a.n - 1 ? one : zero; q.trans = qr == a.n - 1 ? zero : one;
                q.c = is_base ? 0xffffffffu : c;
                q.dl = which == 0 ? d : zero;
                q.dn = (which == 1 || single) ? d : zero;
                const MaMask m = ma_eval<CHIP>(a, q, regs, T);
                if (is_base) { if (which) base1 = m; else base0 = m; }
                else air = air || m.newly(which ? base1 : base0);
            }
        }
        if (is_base || which == 0) continue;
        // the entry is complete: the bus, then its three counts
        bool bus = false;
        if ((fl & 4u) && active && wanted) {
            if (a.bus_walk) bus = ma_bus_detected(a.iw, tm + t + 1, tp + t + 1, S, c, Fp::raw(a.delta[di]));
            else bus = a.flags[a.width + 2 * c] != 0 || (a.flags[a.width + 2 * c + 1] & live) != 0;
        }
        const uint32_t e = c * a.D + di;
        const bool free_ = active && !air && !bus;
        if (mode == MA_COUNT) {
            ma_wave_add(&acc[3 * e], free_);
            ma_wave_add(&acc[3 * e + 1], active && air);
            ma_wave_add(&acc[3 * e + 2], active && bus);
        } else if (free_ && wanted) {
            atomicOr(&acc[e * TW + (t >> 5)], 1u << (t & 31u));
        }
        air = false;
        if (++di == a.D) { di = 0; c++; }
    }
    __syncthreads();
    if (mode == MA_COUNT) {
        for (uint32_t x = 3 * e_lo + t; x < 3 * e_hi; x += T) {
            const uint32_t v = acc[x];
            if (!v) continue;
            atomicAdd(&totals[x], (unsigned long long)v);
            if (x % 3u == 0) table[(uint64_t)(x / 3u) * a.NB + blockIdx.x] = v;
        }
        return;
    }
    for (uint32_t e = e_lo + t; e < EL; e += T) {
        if (!need[e]) continue;
        uint32_t rank = prefix[(uint64_t)e * a.NB + blockIdx.x];
        const uint32_t* bits = acc + e * TW;  // LDS
        for (uint32_t j = 0; j < rows_here && rank < R; j++)
            if ((bits[j >> 5] >> (j & 31u)) & 1u) rows[(uint64_t)e * R + rank++] = (uint32_t)(base + j);
    }
}

// scan: block e of the grid handles entry e (when listed and not empty): prefix[e][w] = sum of table[e][w' < w]
__global__ void __launch_bounds__(256) k_ma_scan(const unsigned long long* __restrict__ totals, const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB, uint32_t e_cut) {
    extern __shared__ uint32_t ma_lds[];  // [256] partial sums
    const uint32_t e = blockIdx.x, t = threadIdx.x;
    if (e >= e_cut || totals[3 * e] == 0) return;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)e * NB;
    uint32_t s = 0;
    for (uint32_t w = lo; w < hi; w++) s += row[w];
    ma_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t v = ma_lds[i]; ma_lds[i] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = ma_lds[t];
    uint32_t* out = prefix + (uint64_t)e * NB;
    for (uint32_t w = lo; w < hi; w++) { out[w] = run; run += row[w]; }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
static size_t ma_lds_bytes(const MaArgs& a, uint32_t T, uint32_t mode) {
    const size_t E = (size_t)a.width * a.D;
    return 4 * (1 + (size_t)ma_acc_words((uint32_t)E, T, mode) + ((size_t)a.width + a.prep_width) * (T + 2) + (a.native_chip == CA_INTERPRET ? (size_t)a.n_regs * T : 0));
}

// Column slices of a launch: a chip of many workgroups gets one, a chip of few rows up to one per column (about 2048 workgroups in all)
uint32_t ma_column_slices(const MaArgs& a, uint32_t NB) {
    const uint32_t want = NB >= 2048 ? 1u : 2048u / NB;
    const uint32_t per_slice = (a.width + want - 1) / want;  // columns per slice; no slice is empty
    return (a.width + per_slice - 1) / per_slice;
}

uint32_t ma_block_threads(const MaArgs& a) {
    uint32_t T = 256;
    while (T > 64 && ma_lds_bytes(a, T, MA_LIST) > 160 * 1024) T >>= 1;
    if (ma_lds_bytes(a, T, MA_LIST) > 160 * 1024 || ma_lds_bytes(a, T, MA_COUNT) > 160 * 1024)
        throw std::invalid_argument("mutation_audit: the row tile of a chip of " + std::to_string(a.width + a.prep_width) + " columns and " + std::to_string(a.n_regs) +
                                    " program registers does not fit a workgroup's LDS (" + std::to_string(ma_lds_bytes(a, 64, MA_LIST)) + " bytes for 64 rows, 163840 at most)");
    return T;
}

#define MA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void ma_check(const MaArgs& a, uint32_t mode) {
    if (a.K > CA_MAX_CONSTRAINTS) throw std::invalid_argument("mutation_audit: the device audit handles up to " + std::to_string(CA_MAX_CONSTRAINTS) + " constraints per chip");
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("mutation_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.CY == 0 || a.CY > a.width || a.CY > 65535) throw std::logic_error("mutation_audit: 1 to width column slices");
    if (a.D == 0 || a.D > 4 || a.width == 0) throw std::logic_error("mutation_audit: 1 to 4 deltas, at least one column");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.T < 64 || a.T > 256 || (a.T & (a.T - 1)) || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("mutation_audit: inconsistent launch shape");
    if (ma_lds_bytes(a, a.T, mode) > 160 * 1024) throw std::logic_error("mutation_audit: the launch shape does not fit the LDS");
    static bool attr = false;
    if (!attr) {
#define MA_X(C) (void)hipFuncSetAttribute((const void*)k_ma_audit<vchips::C>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        MA_CHIPS(MA_X)
#undef MA_X
        (void)hipFuncSetAttribute((const void*)k_ma_audit<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_ma_audit<MA_BUS_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr = true;
    }
}

static void ma_launch(hipStream_t st, const MaArgs& a, uint32_t mode, unsigned long long* totals, uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows) {
    const dim3 grid(a.NB, a.CY), block(a.T);
    const size_t lds = ma_lds_bytes(a, a.T, mode);
    switch (a.native_chip) {
#define MA_X(C) case vchips::C: VK_LAUNCH((k_ma_audit<vchips::C>), grid, block, lds, st, a, mode, totals, table, prefix, e_cut, R, rows); break;
        MA_CHIPS(MA_X)
#undef MA_X
        case CA_INTERPRET: VK_LAUNCH((k_ma_audit<CA_INTERPRET>), grid, block, lds, st, a, mode, totals, table, prefix, e_cut, R, rows); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_ma_audit<MA_BUS_ONLY>), grid, block, lds, st, a, mode, totals, table, prefix, e_cut, R, rows); break;
        default: throw std::logic_error("mutation_audit: a native chip id without constraints");
    }
}

void launch_ma_count(hipStream_t st, const MaArgs& a, unsigned long long* totals, uint32_t* table) {
    ma_check(a, MA_COUNT);
    static const char* names[14] = {"k_ma_count.cpu", "k_ma_count.program", "k_ma_count.mem", "k_ma_count.add", "k_ma_count.sub", "k_ma_count.mul", "k_ma_count.div", "k_ma_count.shift",
                                    "k_ma_count.lt", "k_ma_count.com", "k_ma_count.bitwise", "k_ma_count.output", "k_ma_count.range", "k_ma_count.static_data"};
    const char* name = a.native_chip >= 0 && a.native_chip < 14 ? names[a.native_chip] : (a.native_chip == MA_BUS_ONLY ? "k_ma_count.bus" : "k_ma_count");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width), a.evaluations);  // the profile's per-chip split: bytes read once, row evaluations as its ops
    ma_launch(st, a, MA_COUNT, totals, table, nullptr, 0xffffffffu, 0, nullptr);
}

void launch_ma_scan(hipStream_t st, const MaArgs& a, const unsigned long long* totals, const uint32_t* table, uint32_t* prefix, uint32_t e_cut) {
    ma_check(a, MA_COUNT);
    ProfScope ps("k_ma_scan", st, 8.0 * (double)a.NB);
    VK_LAUNCH(k_ma_scan, dim3(a.width * a.D), dim3(256), 256 * 4, st, totals, table, prefix, a.NB, e_cut);
}

void launch_ma_list(hipStream_t st, const MaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows) {
    ma_check(a, MA_LIST);
    ProfScope ps("k_ma_list", st, 0);
    ma_launch(st, a, MA_LIST, nullptr, const_cast<uint32_t*>(table), prefix, e_cut, R, rows);
}

}  // namespace vk
