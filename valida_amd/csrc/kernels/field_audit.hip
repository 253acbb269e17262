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
// eval, base and record live in field_elim.hpp, which the link audit's mask kernel shares (kernels/link_audit.hip).
// LDS (u32 words): fa_lds_words below.  Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are
// powers of two, columns of programs and interactions are below the width, fields per interaction at most FA_MAX_FIELDS, rows written by
// `list` have ranks below R and slots below s_cut).
#include <mutex>
#include <stdexcept>
#include <string>
#include "field_elim.hpp"

namespace vk {

constexpr uint32_t FA_OUT_WORDS = 18;  // host/rank_audit.hpp: RA_ROW_WORDS

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
// wave's state (FaWave; field_elim.hpp: fa_wave_words).
__host__ __device__ inline uint32_t fa_head_words(const FaArgs& a) { return 8u + 3u * a.NS + 5u * a.M; }

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
