// Coverage audit on the device (host/coverage_audit.hpp states the contract): WHICH constraint or interaction detects each mutation of the
// mutation audit.  The evaluations are the mutation audit's, through the code both share (mutation_eval.hpp): an LDS tile of the workgroup's
// rows plus halo and wrap, one thread per row, one inlined chip eval per kernel (or the interpreted register program, or none for a bus-only
// chip), the bus rule from the per-column masks (or the walk of the definition for more than 32 interactions).  Where the mutation audit keeps
// one bit per mutation, this pass keeps the DETECTOR MASK — the newly failing constraints of rows r and r - 1 OR'd (three words), and the
// interactions whose record changes (one word per 32) — and reduces the masks of all rows to the chip's cell table
// [detector][column][delta] -> {kills, sole, first_row, first_sole_row}.  Every count is an integer sum and every row a minimum: any order of
// accumulation gives the same words.
//   wave    masks are sparse (a few detectors per detected mutation), so per mask word the wave first ORs the word over its lanes
//           (cov_wave_or); per set bit of the OR one ballot and population count gives `kills`, one more ballot on "my mask is exactly this
//           bit" gives `sole`, and the lowest set lane of each ballot — lanes are consecutive rows — gives the row minima (cov_wave_tally):
//           one lane per wave issues the LDS atomics.
//   table   beside the tile the workgroup keeps the cells of ONE column in LDS — [detector][delta][3] u32: kills | sole << 16 (a tile has at most
//           256 rows), and the two row minima as offsets into the tile — 12 (K + M) D bytes: cpu 57 x 2 x 12 = 1.4 KB beside its 52.6 KB tile,
//           54.0 KB, the mutation audit's footprint.  (The cells of every column would be 57 x 51 x 2 x 16 B = 93 KB; a quarter of them kept
//           across a persistent workgroup's tiles — 23.7 KB, four column slices, two more baselines per row and slice — measured 6.44 ms on
//           the cpu chip of a 2^20-row witness where this layout takes 5.5 ms; DESIGN.md 4e has the figures.)
//   flush   when a column's last delta is done the workgroup adds the column's non-zero cells to ITS OWN table in global memory (one table
//           per workgroup along the rows, [cells][4] u32 {kills, sole, ~first_row, ~first_sole_row}, zeroed: the minima are kept as maxima of
//           the complements so that one memset serves; the column slices of one x share the table, their cells are disjoint) and clears
//           them: two barriers per column, a handful of no-return 32-bit atomics onto addresses nobody else touches.  Flushing the columns
//           straight onto one table per chip was measured first: 4096 tiles x ~400 non-zero cells x 2-4 atomics onto ~400 addresses cost cpu
//           about 1 ms of 6.5 and doubled the bus-only launch of mem (2^22 rows).
//   tiles   workgroup x walks the row tiles x, x + GX, ..; GX x slices defaults to at most 1024 workgroups (cov_shape), so the workgroup
//           tables are at most 1024 x cells x 16 bytes whatever the height (cpu: 1024 x 5814 x 16 B = 95 MB at 2^20 rows); u32 counts
//           suffice, a workgroup sees fewer than 2^32 rows.  1024 and not the resident slots: cpu's 54.0 KB should let three workgroups share
//           a CU, yet 768 workgroups measured 6.6 ms where 512 took 5.8, 1024 5.7 and 4096 5.6 — a power of two stays balanced either way.
//   merge   the GX workgroup tables are folded onto the first 32 (k_cov_fold: table y takes y + 32, y + 64, ..), then one thread per cell
//           sums the counts and takes the extrema over those into the chip's table: [cells][2] u64, [cells][2] u32.  No cross-workgroup
//           atomic is left but `detected` (one per tile and delta).
//   slices  a chip of few workgroups is split over gridDim.y column slices exactly as in the mutation audit (ma_column_slices); every slice
//           stages the tile and evaluates the two baselines again.
//   pack    one workgroup per chip compacts the non-zero cells in ascending order (count, prefix, write — no atomic admits a cell) and sums
//           kills / sole over the columns, so that only the chip blocks and the listed cells are downloaded.
// Every index is bounded by what the host computed: mask bits below K (the program's assert count) and M (the interactions), columns inside
// the slice, cells below (K + M) width D.
#include <stdexcept>
#include <string>
#include "mutation_eval.hpp"

namespace vk {

#ifndef VGPU_COV_WAVE_HELPERS
// The three wave-level helpers; all are called from wave-uniform control flow only.  (An emulation without waves supplies the same contracts
// for a wave of one lane.)
// OR of `w` over the lanes of the wave, as a wave-uniform value.  One step per DISTINCT contribution, not per lane: lanes of a wave mutate the
// same column, so their masks mostly coincide.
__device__ __forceinline__ uint32_t cov_wave_or(uint32_t w) {
    uint32_t acc = 0;
    unsigned long long rem;
    while ((rem = __ballot((w & ~acc) != 0)) != 0) acc |= (uint32_t)__builtin_amdgcn_readlane((int)w, __ffsll((long long)rem) - 1);
    return acc;
}
// One detector's tally over the wave into its cell {kills | sole << 16, first row, first sole row} (LDS): pred = my mutation is killed by it,
// solo = and by nothing else; `row` (the row's offset in the tile) ascends with the lane.
__device__ __forceinline__ void cov_wave_tally(uint32_t* cell, bool pred, bool solo, uint32_t row) {
    const unsigned long long b = __ballot(pred), s = __ballot(pred && solo);
    const unsigned long long below = (1ull << (threadIdx.x & 63u)) - 1ull;
    if (pred && (b & below) == 0) { atomicAdd(&cell[0], (uint32_t)__popcll(b) | ((uint32_t)__popcll(s) << 16)); atomicMin(&cell[1], row); }
    if (pred && solo && (s & below) == 0) atomicMin(&cell[2], row);
}
// Adds the number of lanes whose `pred` holds to *counter (LDS)
__device__ __forceinline__ void cov_wave_count(uint32_t* counter, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (pred && (b & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) atomicAdd(counter, (uint32_t)__popcll(b));
}
#endif

constexpr uint32_t COV_CELL_WORDS = 3;  // kills | sole << 16, first_row - tile base, first_sole_row - tile base

// One word of the detector mask: bit b is detector (cell0 + b * stride)
__device__ __forceinline__ void cov_reduce_word(uint32_t* cell0, uint32_t stride, uint32_t word, bool solo, uint32_t row) {
    uint32_t any = cov_wave_or(word);
    while (any) {
        const uint32_t b = (uint32_t)__ffs((int)any) - 1u;
        any &= any - 1u;
        cov_wave_tally(cell0 + b * stride, (word >> b) & 1u, solo, row);
    }
}

// LDS of k_cov_audit (dynamic, one array): the current column's cells [K + M][D][3], detected [4], the main tile [width][T + 2], the
// preprocessed tile [prep_width][T + 2], the interpreter's register file [n_regs][T]
__host__ __device__ inline uint32_t cov_table_words(const CovArgs& v) { return (v.m.K + v.M) * v.m.D * COV_CELL_WORDS; }

// Workgroup (x, y): the row tiles x, x + gridDim.x, .. and the columns of slice y.
template <int CHIP>
__global__ void __launch_bounds__(256) k_cov_audit(CovArgs v, uint32_t* __restrict__ wg_tables, unsigned long long* __restrict__ detected) {
    extern __shared__ uint32_t cov_lds[];
    const MaArgs& a = v.m;
    const uint32_t T = blockDim.x, t = threadIdx.x, S = T + 2, TD = a.K + v.M;
    const uint32_t cpb = (a.width + gridDim.y - 1) / gridDim.y;
    const uint32_t c_lo = blockIdx.y * cpb < a.width ? blockIdx.y * cpb : a.width, c_hi = c_lo + cpb < a.width ? c_lo + cpb : a.width;
    const uint32_t n_tab = TD * a.D * COV_CELL_WORDS, dstride = a.D * COV_CELL_WORDS;
    uint32_t* tab = cov_lds;
    // this workgroup's table (shared with the other column slices of the same x)
    uint32_t* const mine = wg_tables + 4 * (uint64_t)blockIdx.x * TD * a.width * a.D;
    uint32_t* det = tab + n_tab;
    uint32_t* tm = det + 4;
    uint32_t* tp = tm + a.width * S;
    uint32_t* regs = tp + a.prep_width * S + t;
    for (uint32_t x = t; x < n_tab; x += T) tab[x] = (x % COV_CELL_WORDS) ? 0xffffffffu : 0u;
    if (t < 4) det[t] = 0;
    const Fp one = Fp::one(), zero = Fp::zero();
    const bool single = a.n == 1;
    for (uint32_t tile = blockIdx.x; tile < a.NB; tile += gridDim.x) {
        __syncthreads();  // the cells are initialised; the previous tile has no reader left
        // the tile: word j of a column is row (base + j - 1) mod n, j = 0 .. rows_here + 1
        const uint64_t base = (uint64_t)tile * T;
        const uint32_t rows_here = a.n - base < T ? (uint32_t)(a.n - base) : T;
        for (uint32_t col = 0; col < a.width; col++)
            for (uint32_t j = t; j < rows_here + 2; j += T) tm[col * S + j] = a.main[(uint64_t)col * a.mstride + ((base + j + a.n - 1) & (a.n - 1))];
        for (uint32_t col = 0; col < a.prep_width; col++)
            for (uint32_t j = t; j < rows_here + 2; j += T) tp[col * S + j] = a.prep[(uint64_t)col * a.pstride + ((base + j + a.n - 1) & (a.n - 1))];
        __syncthreads();

        const uint64_t r = base + t, rp = (r + a.n - 1) & (a.n - 1);
        const bool active = r < a.n;
        uint32_t live = 0;  // the interactions of row r that are records: bit m
        if (active && !a.bus_walk) {
            for (uint32_t m = 0; m < v.M; m++) {
                uint32_t pos = a.iw[2 + m] + 2;
                Fp c0, c1;
                ma_vcol2(a.iw, pos, tm + t + 1, tp + t + 1, S, 0xffffffffu, zero, c0, c1);
                live |= c0.is_zero() ? 0u : 1u << m;
            }
        }
        MaMask base0, base1, hit;
        base0.clear(); base1.clear(); hit.clear();
        // iterations 0, 1: the baselines of rows r and r - 1; then two per (column, delta) of the slice: the cell as local, the cell as next
        const uint32_t n_it = 2 + 2 * (c_hi - c_lo) * a.D;
        uint32_t c = c_lo, di = 0;
        for (uint32_t it = 0; it < n_it; it++) {
            const bool is_base = it < 2;
            const uint32_t which = it & 1u;
            const uint32_t fl = is_base ? 3u : a.flags[c];
            if (CHIP != MA_BUS_ONLY) {
                const bool run = single ? (which == 0 && (fl & 3u)) : (which == 0 ? (fl & 1u) : (fl & 2u));  // wave-uniform
                if (run && active) {
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
                    else {
#pragma unroll
                        for (int i = 0; i < (int)CA_MASK_WORDS; i++) hit.w[i] |= m.w[i] & ~(which ? base1.w[i] : base0.w[i]);  // newly failing at that row
                    }
                }
            }
            if (is_base || which == 0) continue;
            // the mutation's detector set is complete: its size, then one reduction per mask word
            const bool has_bus = (fl & 4u) && active;
            uint32_t size = 0, busw = 0;
#pragma unroll
            for (int i = 0; i < (int)CA_MASK_WORDS; i++) size += (uint32_t)__popc(hit.w[i]);
            if (!a.bus_walk) {
                if (has_bus) busw = a.flags[a.width + 2 * c] | (a.flags[a.width + 2 * c + 1] & live);
                size += (uint32_t)__popc(busw);
            } else {
                for (uint32_t m_lo = 0; m_lo < v.M; m_lo += 32) size += (uint32_t)__popc(has_bus ? ma_bus_changed(a.iw, tm + t + 1, tp + t + 1, S, c, Fp::raw(a.delta[di]), m_lo) : 0u);
            }
            const bool solo = size == 1;
            cov_wave_count(&det[di], size != 0);
            uint32_t* cell0 = tab + di * COV_CELL_WORDS;
            if (CHIP != MA_BUS_ONLY) {
#pragma unroll
                for (int i = 0; i < (int)CA_MASK_WORDS; i++) cov_reduce_word(cell0 + 32u * (uint32_t)i * dstride, dstride, hit.w[i], solo, t);
            }
            if (!a.bus_walk) cov_reduce_word(cell0 + a.K * dstride, dstride, busw, solo, t);
            else
                for (uint32_t m_lo = 0; m_lo < v.M; m_lo += 32)
                    cov_reduce_word(cell0 + (a.K + m_lo) * dstride, dstride, has_bus ? ma_bus_changed(a.iw, tm + t + 1, tp + t + 1, S, c, Fp::raw(a.delta[di]), m_lo) : 0u, solo, t);
            hit.clear();
            if (++di < a.D) continue;
            // the column is complete (the whole workgroup is here: the loop's control flow is uniform): flush its non-zero cells, clear them
            __syncthreads();
            for (uint32_t x = t; x < TD * a.D; x += T) {
                uint32_t* cell = tab + x * COV_CELL_WORDS;
                const uint32_t ks = cell[0];
                if (!ks) continue;
                const uint32_t tt = x / a.D, j = x - tt * a.D;
                const uint64_t g = ((uint64_t)tt * a.width + c) * a.D + j;
                atomicAdd(&mine[4 * g], ks & 0xffffu);
                atomicMax(&mine[4 * g + 2], ~((uint32_t)base + cell[1]));
                if (ks >> 16) { atomicAdd(&mine[4 * g + 1], ks >> 16); atomicMax(&mine[4 * g + 3], ~((uint32_t)base + cell[2])); }
                cell[0] = 0; cell[1] = 0xffffffffu; cell[2] = 0xffffffffu;
            }
            __syncthreads();
            di = 0; c++;
        }
        __syncthreads();
        // detected cells of the tile: at most T columns-of-the-slice per delta, so the u32 never wraps whatever the workgroup walks
        if (t < a.D && det[t]) { atomicAdd(&detected[t], (unsigned long long)det[t]); det[t] = 0; }
    }
}

constexpr uint32_t COV_FOLD = 32;  // workgroup tables left for the merge

// fold: table y < COV_FOLD takes the tables y + COV_FOLD, y + 2 COV_FOLD, .. < GX; thread per word (counts add, complemented rows take the maximum)
__global__ void __launch_bounds__(256) k_cov_fold(uint32_t* __restrict__ wg_tables, uint32_t GX, uint32_t cells) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, words = 4 * (uint64_t)cells;
    if (x >= words) return;
    uint32_t acc = wg_tables[blockIdx.y * words + x];
    const bool add = (x & 2u) == 0;
    for (uint32_t w = blockIdx.y + COV_FOLD; w < GX; w += COV_FOLD) {
        const uint32_t o = wg_tables[w * words + x];
        acc = add ? acc + o : (o > acc ? o : acc);
    }
    wg_tables[blockIdx.y * words + x] = acc;
}

// merge: thread per cell over the first `tables` workgroup tables
__global__ void __launch_bounds__(256) k_cov_merge(const uint32_t* __restrict__ wg_tables, uint32_t tables, uint32_t cells, unsigned long long* __restrict__ counts,
                                                   uint32_t* __restrict__ rows) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= cells) return;
    unsigned long long kills = 0, sole = 0;
    uint32_t first = 0, first_sole = 0;  // complements: 0 = no row
    for (uint32_t w = 0; w < tables; w++) {
        const uint32_t* c = wg_tables + 4 * ((uint64_t)w * cells + x);
        kills += c[0]; sole += c[1];
        first = c[2] > first ? c[2] : first;
        first_sole = c[3] > first_sole ? c[3] : first_sole;
    }
    counts[2 * (uint64_t)x] = kills; counts[2 * (uint64_t)x + 1] = sole;
    rows[2 * (uint64_t)x] = ~first; rows[2 * (uint64_t)x + 1] = ~first_sole;
}

// pack: one workgroup of 256 threads for the chip.  Thread t owns the cells [t chunk, t chunk + chunk): counts its non-zero ones, the
// exclusive prefix over threads gives its first rank, and it writes its cells of rank < cap.
__global__ void __launch_bounds__(256) k_cov_pack(const unsigned long long* __restrict__ counts, const uint32_t* __restrict__ rows, uint32_t TD, uint32_t W, uint32_t D, uint32_t cap,
                                                  uint32_t* __restrict__ packed) {
    extern __shared__ uint32_t cov_lds[];  // [256]
    const uint32_t t = threadIdx.x, cells = TD * W * D;
    const uint32_t chunk = (cells + 255u) / 256u;
    const uint32_t lo = t * chunk < cells ? t * chunk : cells, hi = lo + chunk < cells ? lo + chunk : cells;
    uint32_t k = 0;
    for (uint32_t x = lo; x < hi; x++) k += counts[2 * (uint64_t)x] != 0 ? 1u : 0u;
    cov_lds[t] = k;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t x = cov_lds[i]; cov_lds[i] = run; run += x; }
        packed[0] = run; packed[1] = 0;
    }
    __syncthreads();
    uint32_t rank = cov_lds[t];
    uint32_t* out = packed + 2 + 4 * (uint64_t)TD * D;
    for (uint32_t x = lo; x < hi && rank < cap; x++) {
        const unsigned long long kills = counts[2 * (uint64_t)x];
        if (!kills) continue;
        const unsigned long long sole = counts[2 * (uint64_t)x + 1];
        uint32_t* o = out + 8 * (uint64_t)rank++;
        o[0] = x; o[1] = (uint32_t)kills; o[2] = (uint32_t)(kills >> 32); o[3] = (uint32_t)sole; o[4] = (uint32_t)(sole >> 32);
        o[5] = rows[2 * (uint64_t)x]; o[6] = rows[2 * (uint64_t)x + 1]; o[7] = 0;
    }
    for (uint32_t e = t; e < TD * D; e += 256) {
        const uint32_t tt = e / D, j = e - tt * D;
        unsigned long long kills = 0, sole = 0;
        for (uint32_t c = 0; c < W; c++) { const uint64_t g = ((uint64_t)tt * W + c) * D + j; kills += counts[2 * g]; sole += counts[2 * g + 1]; }
        uint32_t* o = packed + 2 + 4 * (uint64_t)e;
        o[0] = (uint32_t)kills; o[1] = (uint32_t)(kills >> 32); o[2] = (uint32_t)sole; o[3] = (uint32_t)(sole >> 32);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
constexpr size_t COV_LDS_MAX = 160 * 1024;
constexpr uint32_t COV_WORKGROUPS = 1024;  // of a launch by default, all column slices together (see `tiles` above)

static size_t cov_tile_bytes(const CovArgs& v, uint32_t T) {
    const MaArgs& a = v.m;
    return 4 * (4 + ((size_t)a.width + a.prep_width) * (T + 2) + (a.native_chip == CA_INTERPRET ? (size_t)a.n_regs * T : 0));
}
static size_t cov_lds_bytes(const CovArgs& v, uint32_t T) { return cov_tile_bytes(v, T) + 4 * (size_t)cov_table_words(v); }

void cov_shape(CovArgs& v, uint32_t max_workgroups) {
    MaArgs& a = v.m;
    if ((uint64_t)(a.K + v.M) * a.width * a.D >= (1ull << 31)) throw std::invalid_argument("coverage_audit: the device audit handles up to 2^31 cells (detector, column, delta) per chip");
    for (uint32_t T = 256; T >= 64; T >>= 1) {
        if (cov_lds_bytes(v, T) > COV_LDS_MAX) continue;
        a.T = T;
        a.NB = (uint32_t)((a.n + T - 1) / T);
        a.CY = ma_column_slices(a, a.NB);
        const uint32_t gx = max_workgroups ? max_workgroups : (COV_WORKGROUPS / a.CY ? COV_WORKGROUPS / a.CY : 1u);
        v.GX = gx < a.NB ? gx : a.NB;
        return;
    }
    throw std::invalid_argument("coverage_audit: the row tile of a chip of " + std::to_string(a.width + a.prep_width) + " columns and " + std::to_string(a.n_regs) + " program registers with one column's cells of " +
                                std::to_string(a.K + v.M) + " detectors does not fit a workgroup's LDS (" + std::to_string(cov_lds_bytes(v, 64)) + " bytes for 64 rows, 163840 at most)");
}

#define COV_CHIPS(X)                                                                                                                         \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

void launch_cov_audit(hipStream_t st, const CovArgs& v, uint32_t* wg_tables, unsigned long long* detected) {
    const MaArgs& a = v.m;
    if (a.K > CA_MAX_CONSTRAINTS) throw std::invalid_argument("coverage_audit: the device audit handles up to " + std::to_string(CA_MAX_CONSTRAINTS) + " constraints per chip");
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("coverage_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.CY == 0 || a.CY > a.width || a.CY > 65535 || v.GX == 0 || v.GX > a.NB) throw std::logic_error("coverage_audit: 1 to width column slices, 1 to NB workgroups along the rows");
    if (a.D == 0 || a.D > 4 || a.width == 0) throw std::logic_error("coverage_audit: 1 to 4 deltas, at least one column");
    if (!a.bus_walk && v.M > 32) throw std::logic_error("coverage_audit: the bus masks hold at most 32 interactions");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.T < 64 || a.T > 256 || (a.T & (a.T - 1)) || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("coverage_audit: inconsistent launch shape");
    const size_t lds = cov_lds_bytes(v, a.T);
    if (lds > COV_LDS_MAX) throw std::logic_error("coverage_audit: the launch shape does not fit the LDS");
    static bool attr = false;
    if (!attr) {
#define COV_X(C) (void)hipFuncSetAttribute((const void*)k_cov_audit<vchips::C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_LDS_MAX);
        COV_CHIPS(COV_X)
#undef COV_X
        (void)hipFuncSetAttribute((const void*)k_cov_audit<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_cov_audit<MA_BUS_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_LDS_MAX);
        attr = true;
    }
    static const char* names[14] = {"k_cov_audit.cpu", "k_cov_audit.program", "k_cov_audit.mem", "k_cov_audit.add", "k_cov_audit.sub", "k_cov_audit.mul", "k_cov_audit.div", "k_cov_audit.shift",
                                    "k_cov_audit.lt", "k_cov_audit.com", "k_cov_audit.bitwise", "k_cov_audit.output", "k_cov_audit.range", "k_cov_audit.static_data"};
    const char* name = a.native_chip >= 0 && a.native_chip < 14 ? names[a.native_chip] : (a.native_chip == MA_BUS_ONLY ? "k_cov_audit.bus" : "k_cov_audit");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width) * a.CY, a.evaluations);  // bytes read (every slice stages the tile), row evaluations as its ops
    const dim3 grid(v.GX, a.CY), block(a.T);
    switch (a.native_chip) {
#define COV_X(C) case vchips::C: VK_LAUNCH((k_cov_audit<vchips::C>), grid, block, lds, st, v, wg_tables, detected); break;
        COV_CHIPS(COV_X)
#undef COV_X
        case CA_INTERPRET: VK_LAUNCH((k_cov_audit<CA_INTERPRET>), grid, block, lds, st, v, wg_tables, detected); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_cov_audit<MA_BUS_ONLY>), grid, block, lds, st, v, wg_tables, detected); break;
        default: throw std::logic_error("coverage_audit: a native chip id without constraints");
    }
}

void launch_cov_merge(hipStream_t st, const CovArgs& v, uint32_t* wg_tables, unsigned long long* counts, uint32_t* rows) {
    const uint32_t cells = (uint32_t)cov_cells(v);
    if (!cells) return;  // a chip without constraints and interactions
    ProfScope ps("k_cov_merge", st, 16.0 * (double)cells * v.GX);
    if (v.GX > COV_FOLD) VK_LAUNCH(k_cov_fold, dim3((4 * cells + 255) / 256, COV_FOLD), dim3(256), 0, st, wg_tables, v.GX, cells);
    VK_LAUNCH(k_cov_merge, dim3((cells + 255) / 256), dim3(256), 0, st, wg_tables, v.GX < COV_FOLD ? v.GX : COV_FOLD, cells, counts, rows);
}

void launch_cov_pack(hipStream_t st, const CovArgs& v, const unsigned long long* counts, const uint32_t* rows, uint32_t cap, uint32_t* packed) {
    ProfScope ps("k_cov_pack", st, 24.0 * (double)cov_cells(v));
    VK_LAUNCH(k_cov_pack, dim3(1), dim3(256), 256 * 4, st, counts, rows, v.m.K + v.M, v.m.width, v.m.D, cap, packed);
}

}  // namespace vk
