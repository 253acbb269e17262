// Link audit on the device (host/link_audit.hpp states the contract): the field audit's float mask of every live record, joined over the bus
// audit's tuples — a position that floats at every record of a tuple is open.
//   masks    k_la_masks<CHIP>: the field audit's shape and elimination (field_elim.hpp; kernels/field_audit.hip states the method): one wave per
//            workgroup, the wave takes the workgroup's T rows one after the other over a [column][S] tile with halo and wrap, fa_base once per
//            row that has a live record, fa_record per live interaction, and for a chip without constraints the row before's masks while the
//            live set repeats.  No counting tables, no listing: for every live (row, m) the mask goes to mask[first_id(chip) + row M + m], the
//            bus audit's slot id.  The host zeroes `mask` before, so the live slots of a chip that is not launched (no column: only constant
//            fields) read 0.
//   grouping the bus audit's launchers, unchanged (kernels/bus_audit.hip: records, sort, groups, reduce; the exact path after a key collision).
//   join     k_la_join: 256 consecutive sorted records per workgroup (they span groups g0 .. g0 + 255 at most, as in k_ba_reduce): AND of the
//            masks per group in LDS, then one global atomicAnd per group the workgroup touches; tmask is pre-set to all ones.  Integer
//            operations: the result does not depend on the order.
//   tally    k_la_tally: the same tiling; every record reads its tuple's mask and counts, per (chip, interaction, field), the rows where the
//            field floats and where it is open; group heads count per bus the tuples, the open tuples and per position the tuples in which it
//            is open, every record the records of those.  The floating rows are counted HERE, not in the mask pass.  Counters live in an LDS
//            table when it fits (LA_TALLY_LDS_WORDS), one u64 atomic per non-zero counter and workgroup; otherwise straight u64 atomics.
//   report   open groups are compacted (k_la_select), sorted by first record id with the bus audit's sort, and the first max_tuples get their
//            tuple recomputed from the id, their mask, their record counts and their first R (record id, mask).  Only that crosses PCIe.
// Wave primitives: fa_ballot and fa_wave_sync only (field_elim.hpp), and only in k_la_masks; an emulation without waves supplies both
// (tests/emu/link_audit_emu.cpp).  Nothing here asserts on trace contents; every index is bounded by what the host computed: heights are powers
// of two and rows are below them, a slot id is below the slot count (first_id + row M + m with row < height, m < M), columns of programs and
// interactions are below the width, group numbers are below the record count (gid of a live sorted position), a record's mask is cut to its
// interaction's fields before it indexes a counter (so field slots stay below NS and bus positions below 32), reported tuples are below n_rep
// and listed records below min(R, group size).
#include <mutex>
#include <stdexcept>
#include <string>
#include "field_elim.hpp"
#include "bus_records.hpp"

namespace vk {

// u32 words of a mask workgroup's LDS before the tile: head 8, per interaction float mask / live flag / weight rows' offset / fields
__host__ __device__ inline uint32_t la_head_words(const FaArgs& a) { return 8u + 4u * a.M; }

// Workgroup x: rows [x T, x T + T) of the chip whose records start at slot first_id
template <int CHIP>
__global__ void __launch_bounds__(64) k_la_masks(FaArgs a, uint32_t first_id, uint32_t* __restrict__ mask) {
    extern __shared__ uint32_t la_lds[];
    const uint32_t lane = threadIdx.x, w = a.width, T = a.T, S = (T + 2u) | 1u, M = a.M;
    uint32_t* fm = la_lds + 8;  // [M] the row's float mask of the interaction
    uint32_t* lv = fm + M;      // [M] the interaction is live on the row
    uint32_t* wat = lv + M;     // [M] where the interaction's weight rows are (a.wr)
    uint32_t* wnf = wat + M;    // [M] its fields
    uint32_t* tm = wnf + M;
    uint32_t* tp = tm + w * S;
    uint32_t* wv = tp + a.prep_width * S;
    FaWave W;
    W.w = w; W.BS = w | 1u; W.QS = (w + a.F) | 1u; W.WPL = (w + 63u) >> 6; W.lane = lane; W.rho = 0;
    W.slot = wv; W.row_of = wv + 4; W.irow = W.row_of + w; W.bufa = W.irow + w; W.bufb = W.bufa + w + a.F; W.basis = W.bufb + w + a.F; W.raw = W.basis + w * W.BS;
    W.quot = W.raw + a.K * w; W.qpiv = W.quot + a.F * W.QS;
    W.regs = W.qpiv + a.F + lane;
    for (uint32_t x = lane; x < la_head_words(a); x += 64u) la_lds[x] = 0;
    __syncthreads();
    for (uint32_t m = lane; m < M; m += 64u) { const uint32_t at = a.wr[2 + m]; wat[m] = at; wnf[m] = a.wr[at]; }
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

    uint32_t live_prev = 0;  // wave-uniform
    bool have_prev = false;
    for (uint32_t j = 0; j < rows_here; j++) {
        const uint64_t r = base + j;
        uint32_t live = 0;
        bool any_live = false;
        for (uint32_t m = 0; m < M; m++) {
            uint32_t pos = a.iw[2 + m] + 2;
            const bool l = !fa_vcol(a.iw, pos, tm + j + 1, tp + j + 1, S).is_zero();
            if (lane == 0) lv[m] = l ? 1u : 0u;
            if (m < 32u) live |= l ? 1u << m : 0u;
            any_live = any_live || l;
        }
        const bool reuse = CHIP == MA_BUS_ONLY && M <= 32u && have_prev && live == live_prev;
        live_prev = live; have_prev = true;
        fa_wave_sync();
        if (!reuse && any_live) {  // a row without a live record has no mask to write: its base is never built
            fa_base<CHIP>(a, W, tm, tp, S, j, r);
            for (uint32_t m = 0; m < M; m++) {
                if (!lv[m]) continue;  // wave-uniform
                const uint32_t mk = fa_record(a, W, wat[m], wnf[m]);
                if (lane == 0) fm[m] = mk;
            }
            fa_wave_sync();
        }
        const uint32_t slot0 = first_id + (uint32_t)r * M;  // below the slot count: the host refused 2^32 - 1 slots and more
        for (uint32_t m = lane; m < M; m += 64u)
            if (lv[m]) mask[slot0 + m] = fm[m];
        fa_wave_sync();  // lv and fm are written again for the next row
    }
}

// ---- join, tally, select, report: over the bus audit's sorted records ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_la_join(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ gid, uint32_t n_live,
                                                 uint32_t* __restrict__ tmask) {
    extern __shared__ uint32_t la_lds[];  // [256] the AND of local group l, [256] the workgroup holds a record of it
    uint32_t* s_and = la_lds;
    uint32_t* s_hit = la_lds + 256;
    const uint64_t first = (uint64_t)blockIdx.x * 256, i = first + threadIdx.x;
    s_and[threadIdx.x] = 0xffffffffu; s_hit[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t g0 = first < n_live ? gid[first] - 1 : 0u;  // the block's 256 records span groups g0 .. g0 + 255 at most
    if (i < n_live) {
        const uint32_t l = gid[i] - 1 - g0;
        atomicAnd(&s_and[l], mask[ids[i]]);
        s_hit[l] = 1;
    }
    __syncthreads();
    if (s_hit[threadIdx.x]) atomicAnd(&tmask[(uint64_t)g0 + threadIdx.x], s_and[threadIdx.x]);
}

// lt: [0] NS = fields of the whole machine; chip c: lt[4 + c] = where in lt its interactions' first field slots are.
// tally (u64): [s] floating rows of field slot s, [NS + s] open rows, then per bus slot b at 2 NS + 66 b: [0] tuples [1] open tuples
// [2 + j] tuples in which position j is open [34 + j] the records of those.  lds_words = 2 NS + 66 buses when the table fits the LDS, else 0.
constexpr uint32_t LA_BUS_WORDS = 66, LA_TALLY_LDS_WORDS = 12 * 1024;
__global__ void __launch_bounds__(256) k_la_tally(const uint32_t* __restrict__ d, const uint32_t* __restrict__ lt, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ mask,
                                                  const uint32_t* __restrict__ gid, const uint32_t* __restrict__ head_pos, const uint32_t* __restrict__ tmask, uint32_t n_live,
                                                  uint32_t lds_words, unsigned long long* __restrict__ tally) {
    extern __shared__ uint32_t la_lds[];  // [lds_words] this workgroup's counters
    for (uint32_t x = threadIdx.x; x < lds_words; x += 256u) la_lds[x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_live) {
        const uint32_t id = ids[i], g = gid[i] - 1;
        const uint32_t c = ba_chip_of(d, id);
        const BaChip chip = ba_chip(d, c);
        const uint32_t m = (id - chip.first_id) % chip.M;
        const uint32_t* ie = d + chip.table + 4 * m;
        const uint32_t bus = ie[2], nf = ie[3], NS = lt[0];
        const uint32_t cut = nf >= 32u ? 0xffffffffu : (1u << nf) - 1u;
        const uint32_t fmk = mask[id] & cut, open = tmask[g] & fmk;  // a tuple's mask is below every record's: open is the tuple's mask
        const uint32_t slot = lt[lt[4 + c] + m], bb = 2u * NS + LA_BUS_WORDS * bus;
        const bool head = head_pos[g] == (uint32_t)i;
#define LA_ADD(x)                                                   \
    do {                                                            \
        if (lds_words) atomicAdd(&la_lds[(x)], 1u);                 \
        else atomicAdd(&tally[(x)], (unsigned long long)1);         \
    } while (0)
        for (uint32_t b = fmk; b; b &= b - 1) LA_ADD(slot + (uint32_t)__builtin_ctz(b));
        for (uint32_t b = open; b; b &= b - 1) {
            const uint32_t j = (uint32_t)__builtin_ctz(b);
            LA_ADD(NS + slot + j);
            LA_ADD(bb + 34u + j);
            if (head) LA_ADD(bb + 2u + j);
        }
        if (head) {
            LA_ADD(bb);
            if (open) LA_ADD(bb + 1u);
        }
#undef LA_ADD
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < lds_words; x += 256u)
        if (la_lds[x]) atomicAdd(&tally[x], (unsigned long long)la_lds[x]);
}

// appends (first record id, group) of at most cap open groups; counters[4]: the append cursor (zeroed)
__global__ void __launch_bounds__(256) k_la_select(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ head_pos, const uint32_t* __restrict__ tmask, uint32_t n_groups,
                                                   uint32_t cap, unsigned long long* __restrict__ ukeys, uint32_t* __restrict__ uvals, uint32_t* __restrict__ counters) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups || !tmask[g]) return;
    const uint32_t at = atomicAdd(&counters[4], 1u);
    if (at < cap) { ukeys[at] = ids[head_pos[g]]; uvals[at] = (uint32_t)g; }
}

// out, per reported tuple t (stride = 8 + wmax + 2 R words): [0] bus slot [1] records listed [2] tuple mask [3] send records [4] receive records
// [5..7] 0, wmax padded fields, then R x (record id, record mask)
__global__ void __launch_bounds__(64) k_la_report(const uint32_t* __restrict__ d, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ head_pos,
                                                  const uint32_t* __restrict__ nrec, const uint32_t* __restrict__ tmask, const uint32_t* __restrict__ uvals, uint32_t n_rep, uint32_t R,
                                                  uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_rep) return;
    const uint32_t wmax = d[2], stride = 8 + wmax + 2 * R;
    uint32_t* o = out + (uint64_t)t * stride;
    const uint64_t g = uvals[t];
    const uint32_t hp = head_pos[g];
    BaRef r = ba_ref(d, ids[hp]);
    const uint64_t size = (uint64_t)nrec[2 * g] + nrec[2 * g + 1];
    const uint32_t listed = size < R ? (uint32_t)size : R;
    o[0] = r.bus_slot; o[1] = listed; o[2] = tmask[g]; o[3] = nrec[2 * g]; o[4] = nrec[2 * g + 1]; o[5] = 0; o[6] = 0; o[7] = 0;
    for (uint32_t j = 0; j < wmax; j++) o[8 + j] = j < r.n_fields ? ba_next_field(d, r) : 0u;
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t id = k < listed ? ids[hp + k] : 0u;
        o[8 + wmax + 2 * k] = id; o[8 + wmax + 2 * k + 1] = k < listed ? mask[id] : 0u;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t la_lds_bytes(const FaArgs& a, uint32_t T) {
    const size_t S = (T + 2u) | 1u;
    return 4 * ((size_t)la_head_words(a) + ((size_t)a.width + a.prep_width) * S + fa_wave_words(a, a.native_chip == CA_INTERPRET));
}

void la_shape(FaArgs& a) {
    const size_t LDS = 160 * 1024;
    if (a.F > FA_MAX_FIELDS)
        throw std::invalid_argument("link_audit: an interaction of " + std::to_string(a.F) + " fields; the device pass keeps a record's float mask in one word: at most " +
                                    std::to_string(FA_MAX_FIELDS) + " fields per interaction");
    if (a.width > 192 || la_lds_bytes(a, 1) > LDS)
        throw std::invalid_argument("link_audit: a chip of " + std::to_string(a.width) + " columns, " + std::to_string(a.K) + " constraints, " + std::to_string(a.M) + " interactions (" +
                                    std::to_string(a.F) + " fields at most in one record) and " + std::to_string(a.native_chip == CA_INTERPRET ? a.n_regs : 0u) +
                                    " interpreted registers does not fit a workgroup's LDS with one wave (" + std::to_string(la_lds_bytes(a, 1)) +
                                    " bytes: 4 x (basis w (w | 1) + raw rows K w + quotient F ((w + F) | 1) + 128 per register + 4 w + 3 F + 12 + 4 interactions + 3 (w + prep w)), 163840 at most; "
                                    "at most 192 columns)");
    // the field audit's choice: 16 rows per workgroup (64 for a chip without constraints), fewer while the chip has under 1024 workgroups or the
    // tile does not fit
    uint32_t t = a.K ? 16 : 64;
    while (t > 1 && (a.n / t < 1024 || la_lds_bytes(a, t) > LDS)) t >>= 1;
    a.T = t;
    a.NB = (uint32_t)((a.n + a.T - 1) / a.T);
}

#define LA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void la_check(const FaArgs& a) {
    if ((a.K == 0) != (a.native_chip == MA_BUS_ONLY)) throw std::logic_error("link_audit: a chip without constraints is audited on its bus alone, every other by its eval");
    if (a.width == 0 || a.width > 192 || a.F > FA_MAX_FIELDS) throw std::logic_error("link_audit: 1 to 192 columns, at most 32 fields per interaction");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.T == 0 || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("link_audit: inconsistent launch shape");
    if (la_lds_bytes(a, a.T) > 160 * 1024) throw std::logic_error("link_audit: the launch shape does not fit the LDS");
    // the opt-in to more than 64 KB of dynamic LDS is a property of the function on one device: once per device, whichever thread comes first
    static std::mutex mu;
    static uint64_t done = 0;  // bit d: device d has it
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) throw std::runtime_error("link_audit: no current device");
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done >> dev) & 1u)) return;
    auto opt_in = [&](const void* f, const char* kernel) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess)
            throw std::runtime_error(std::string("link_audit: hipFuncSetAttribute(") + kernel + ", hipFuncAttributeMaxDynamicSharedMemorySize, 163840) failed on device " + std::to_string(dev) + ": " +
                                     hipGetErrorString(e));
    };
#define LA_X(C) opt_in((const void*)k_la_masks<vchips::C>, "k_la_masks<" #C ">");
    LA_CHIPS(LA_X)
#undef LA_X
    opt_in((const void*)k_la_masks<CA_INTERPRET>, "k_la_masks<CA_INTERPRET>");
    opt_in((const void*)k_la_masks<MA_BUS_ONLY>, "k_la_masks<MA_BUS_ONLY>");
    if (dev < 64) done |= 1ull << dev;
}

void launch_la_masks(hipStream_t st, const FaArgs& a, uint32_t first_id, uint32_t* mask) {
    la_check(a);
    if (!a.M) return;  // no interaction, no record
    const int id = a.native_chip;
    const char* name = id >= 0 ? "k_la_masks.native" : (id == MA_BUS_ONLY ? "k_la_masks.bus" : "k_la_masks.interpret");
    ProfScope ps(name, st, 4.0 * (double)a.n * (a.width + a.prep_width), a.evaluations);
    const dim3 grid(a.NB), block(64);
    const size_t lds = la_lds_bytes(a, a.T);
    switch (a.native_chip) {
#define LA_X(C) case vchips::C: VK_LAUNCH((k_la_masks<vchips::C>), grid, block, lds, st, a, first_id, mask); break;
        LA_CHIPS(LA_X)
#undef LA_X
        case CA_INTERPRET: VK_LAUNCH((k_la_masks<CA_INTERPRET>), grid, block, lds, st, a, first_id, mask); break;
        case MA_BUS_ONLY: VK_LAUNCH((k_la_masks<MA_BUS_ONLY>), grid, block, lds, st, a, first_id, mask); break;
        default: throw std::logic_error("link_audit: a native chip id without constraints");
    }
}

static unsigned la_blocks(uint64_t n, uint64_t per = 256) { return (unsigned)((n + per - 1) / per); }

void launch_la_join(hipStream_t st, const uint32_t* ids, const uint32_t* mask, const uint32_t* gid, uint32_t n_live, uint32_t* tmask) {
    if (!n_live) return;
    ProfScope ps("k_la_join", st, 12.0 * n_live);
    VK_LAUNCH(k_la_join, dim3(la_blocks(n_live)), dim3(256), 512 * 4, st, ids, mask, gid, n_live, tmask);
}
void launch_la_tally(hipStream_t st, const uint32_t* desc, const uint32_t* lt, const uint32_t* ids, const uint32_t* mask, const uint32_t* gid, const uint32_t* head_pos, const uint32_t* tmask,
                     uint32_t n_live, uint32_t n_fields, uint32_t n_buses, unsigned long long* tally) {
    if (!n_live) return;
    const uint64_t words = la_tally_words(n_fields, n_buses);
    const uint32_t lds_words = words <= LA_TALLY_LDS_WORDS ? (uint32_t)words : 0u;
    ProfScope ps("k_la_tally", st, 20.0 * n_live);
    VK_LAUNCH(k_la_tally, dim3(la_blocks(n_live)), dim3(256), (size_t)(lds_words ? lds_words : 1u) * 4, st, desc, lt, ids, mask, gid, head_pos, tmask, n_live, lds_words, tally);
}
void launch_la_select(hipStream_t st, const uint32_t* ids, const uint32_t* head_pos, const uint32_t* tmask, uint32_t n_groups, uint32_t cap, unsigned long long* ukeys, uint32_t* uvals,
                      uint32_t* counters) {
    if (!n_groups) return;
    ProfScope ps("k_la_select", st, 8.0 * n_groups);
    VK_LAUNCH(k_la_select, dim3(la_blocks(n_groups)), dim3(256), 0, st, ids, head_pos, tmask, n_groups, cap, ukeys, uvals, counters);
}
void launch_la_report(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* mask, const uint32_t* head_pos, const uint32_t* nrec, const uint32_t* tmask,
                      const uint32_t* uvals, uint32_t n_rep, uint32_t R, uint32_t* out) {
    if (!n_rep) return;
    ProfScope ps("k_la_report", st, 64.0 * n_rep);
    VK_LAUNCH(k_la_report, dim3(la_blocks(n_rep, 64)), dim3(64), 0, st, desc, ids, mask, head_pos, nrec, tmask, uvals, n_rep, R, out);
}

}  // namespace vk
