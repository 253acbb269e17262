// Constraint audit on the device (host/constraint_audit.hpp states the contract): which AIR constraints of a witness fail, on which rows, with
// which value — check_constraints (machine/src/check_constraints.rs:14-84) made exact and complete.  One thread per trace row, one launch per
// chip that has constraints; columns come from the column-major working layout (a wave's load of a column is one contiguous request), `next`
// is row + 1 mod n of the same column.  Two realisations of Air::eval, the same bits:
//   * the BasicMachine chips: vchips::eval_chip<CHIP> instantiated over a folder whose assert_zero sets bit k of a three-word fail mask
//     (bitwise has 88 constraints, lt 60, cpu 53) and keeps nothing else per constraint;
//   * captured AIRs: the register program of air/symbolic.hpp interpreted with its register file in LDS (slot-major), OP_ASSERT setting the bit.
//
//   count   every row's mask; per-constraint failing-row counts and the rows-with-any-failure count are reduced per wave (ca_wave_add, the
//           file's only wave-level code), then per workgroup in LDS; one global atomic per non-zero (workgroup, constraint) entry, and that
//           entry goes into the chip's count table [constraint][workgroup].  A clean witness issues no atomic and writes nothing.
//   scan    only for a chip with a listed failing constraint: exclusive prefix of the table over workgroups, per listed constraint.
//   list    workgroups in which a listed constraint fails and whose prefix is below R = max_rows_per_constraint re-evaluate their rows, put
//           the masks in LDS, and one thread per constraint walks them in row order: rank = prefix + position, rows of rank < R are written
//           at their rank.  The listed rows are the first R in ascending order whatever the scheduling was.
//   values  one thread per listed (constraint, rank): the chip evaluated once more on that row, the constraint's value kept, canonical.
// Scratch: 8 bytes per (constraint, workgroup) = at most 8 K / T bytes per row (T = rows per workgroup: 256, less for an interpreted program
// with a large register file), K + 1 u64 totals per chip, and 8 R bytes per constraint of a chip that fails.
// Nothing here asserts on trace contents; every index is bounded by what the host computed (heights are powers of two, the columns a program
// loads are checked against the trace widths in constraint_audit_plan, rows written by `list` are below n and ranks below R).
#include <stdexcept>
#include "launch.hpp"
#include "../chips/basic_machine.hpp"

namespace vk {

#ifndef VGPU_CA_WAVE_ADD
// Adds the number of lanes of this wave whose `pred` holds to *counter (LDS) with one atomic, and returns that number to every lane.
// Called from wave-uniform control flow only.  (An emulation without waves supplies the same contract for a wave of one lane.)
__device__ __forceinline__ uint32_t ca_wave_add(uint32_t* counter, bool pred) {
    const unsigned long long b = __ballot(pred);
    const uint32_t c = (uint32_t)__popcll(b);
    if (pred && (b & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) atomicAdd(counter, c);  // the lowest lane that has it
    return c;
}
#endif

struct CaMask {
    uint32_t w[CA_MASK_WORDS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < (int)CA_MASK_WORDS; i++) w[i] = 0;
    }
    __device__ __forceinline__ void set(uint32_t k, bool on) {
        const uint32_t b = on ? 1u << (k & 31u) : 0u;  // selects, not w[k >> 5]: a run-time k would put the mask in scratch
        w[0] |= k < 32u ? b : 0u;
        w[1] |= (k >= 32u && k < 64u) ? b : 0u;
        w[2] |= k >= 64u ? b : 0u;
    }
    __device__ __forceinline__ bool any() const {
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < (int)CA_MASK_WORDS; i++) o |= w[i];
        return o != 0;
    }
};
// bit k of a three-word mask, by selects: indexing the words by a run-time k would put the mask in scratch
__device__ __forceinline__ bool ca_bit(const uint32_t (&m)[CA_MASK_WORDS], uint32_t k) {
    static_assert(CA_MASK_WORDS == 3, "ca_bit selects among three words");
    const uint32_t w = k < 32u ? m[0] : (k < 64u ? m[1] : m[2]);
    return (w >> (k & 31u)) & 1u;
}

// the chips' eval templates over the trace domain: assert_zero records a bit (and, when asked for one constraint's value, that value)
struct AuditFolder {
    using Expr = Fp;
    const uint32_t* __restrict__ main_p;
    const uint32_t* __restrict__ main_n;
    uint64_t mstride;
    const uint32_t* __restrict__ prep_p;
    const uint32_t* __restrict__ prep_n;
    uint64_t pstride;
    Fp first, last, trans;
    uint32_t k, want;
    Fp value;
    CaMask mask;
    __device__ __forceinline__ Fp constant(uint32_t c) const { return Fp::from_canonical(c); }
    __device__ __forceinline__ Fp main(int col, bool next) const { return Fp::raw((next ? main_n : main_p)[(uint64_t)col * mstride]); }
    __device__ __forceinline__ Fp preprocessed(int col, bool next) const { return Fp::raw((next ? prep_n : prep_p)[(uint64_t)col * pstride]); }
    __device__ __forceinline__ Fp is_first_row() const { return first; }
    __device__ __forceinline__ Fp is_last_row() const { return last; }
    __device__ __forceinline__ Fp is_transition() const { return trans; }
    __device__ __forceinline__ void assert_zero(const Fp& e) {
        mask.set(k, !e.is_zero());
        if (k == want) value = e;
        k++;
    }
};

// Row `r` of the chip: its fail mask; with want < K also the value of constraint `want`.  CHIP: a vchips::ChipId, or CA_INTERPRET for the
// register program (regs: this thread's slot of the LDS register file, slot stride S).
template <int CHIP>
__device__ __forceinline__ CaMask ca_eval_row(const CaArgs& a, uint64_t r, uint32_t want, Fp* value, uint32_t* regs, uint32_t S) {
    const uint64_t nx = (r + 1) & (a.n - 1);
    const Fp first = r == 0 ? Fp::one() : Fp::zero(), last = r == a.n - 1 ? Fp::one() : Fp::zero(), trans = r == a.n - 1 ? Fp::zero() : Fp::one();
    if (CHIP >= 0) {
        AuditFolder f;
        f.main_p = a.main + r; f.main_n = a.main + nx; f.mstride = a.mstride;
        f.prep_p = a.prep + r; f.prep_n = a.prep + nx; f.pstride = a.pstride;
        f.first = first; f.last = last; f.trans = trans;
        f.k = 0; f.want = want; f.value = Fp::zero();
        f.mask.clear();
        vchips::eval_chip(CHIP, f);  // CHIP is a compile-time constant: the switch folds to the one chip
        if (value) *value = f.value;
        return f.mask;
    }
    CaMask mask;
    mask.clear();
    Fp val = Fp::zero();
    uint32_t k = 0;
#define CA_GET(i) (regs[(uint32_t)(i) * S])
#define CA_SET(i, v) (regs[(uint32_t)(i) * S] = (v))
    for (uint32_t pc = 0; pc < a.n_instrs; pc++) {
        const vair::Instr in = a.prog[pc];
        switch (in.op) {
            case vair::OP_CONST: CA_SET(in.dst, (uint32_t)in.a | ((uint32_t)in.b << 16)); break;
            case vair::OP_LOAD_MAIN: CA_SET(in.dst, a.main[(uint64_t)in.a * a.mstride + (in.flag ? nx : r)]); break;
            case vair::OP_LOAD_PREP: CA_SET(in.dst, a.prep[(uint64_t)in.a * a.pstride + (in.flag ? nx : r)]); break;
            case vair::OP_SEL_FIRST: CA_SET(in.dst, first.v); break;
            case vair::OP_SEL_LAST: CA_SET(in.dst, last.v); break;
            case vair::OP_SEL_TRANS: CA_SET(in.dst, trans.v); break;
            case vair::OP_ADD: { const uint32_t x = CA_GET(in.a), y = CA_GET(in.b); CA_SET(in.dst, (Fp::raw(x) + Fp::raw(y)).v); } break;
            case vair::OP_SUB: { const uint32_t x = CA_GET(in.a), y = CA_GET(in.b); CA_SET(in.dst, (Fp::raw(x) - Fp::raw(y)).v); } break;
            case vair::OP_MUL: { const uint32_t x = CA_GET(in.a), y = CA_GET(in.b); CA_SET(in.dst, (Fp::raw(x) * Fp::raw(y)).v); } break;
            case vair::OP_NEG: { const uint32_t x = CA_GET(in.a); CA_SET(in.dst, (-Fp::raw(x)).v); } break;
            case vair::OP_ASSERT: { const Fp x = Fp::raw(CA_GET(in.a)); mask.set(k, !x.is_zero()); if (k == want) val = x; k++; } break;
            default: break;  // OP_NOP padding
        }
    }
#undef CA_GET
#undef CA_SET
    if (value) *value = val;
    return mask;
}

// LDS of the kernels below (dynamic, one array): [0, CA_LDS_HEAD) counters / flags, then what the kernel says
constexpr uint32_t CA_LDS_HEAD = CA_MAX_CONSTRAINTS + 2;

// count: totals[k] (k < K: failing rows of constraint k; k == K: rows failing anything) and table[k * NB + workgroup]
template <int CHIP>
__global__ void __launch_bounds__(256) k_ca_count(CaArgs a, unsigned long long* __restrict__ totals, uint32_t* __restrict__ table) {
    extern __shared__ uint32_t ca_lds[];  // [CA_LDS_HEAD] counts, then the interpreter's register file [n_regs][blockDim.x]
    const uint32_t T = blockDim.x, t = threadIdx.x;
    for (uint32_t k = t; k <= a.K; k += T) ca_lds[k] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * T + t;
    CaMask m;
    m.clear();
    if (r < a.n) m = ca_eval_row<CHIP>(a, r, 0xffffffffu, nullptr, ca_lds + CA_LDS_HEAD + t, T);
    if (ca_wave_add(&ca_lds[a.K], m.any()))  // wave-uniform: a wave without a failing row does nothing more
        for (uint32_t k = 0; k < a.K; k++) ca_wave_add(&ca_lds[k], ca_bit(m.w, k));
    __syncthreads();
    for (uint32_t k = t; k <= a.K; k += T) {
        const uint32_t c = ca_lds[k];
        if (!c) continue;
        atomicAdd(&totals[k], (unsigned long long)c);
        if (k < a.K) table[(uint64_t)k * a.NB + blockIdx.x] = c;
    }
}

// scan: block k of the grid handles constraint k (when listed): prefix[k][w] = sum of table[k][w' < w]
__global__ void __launch_bounds__(256) k_ca_scan(const uint32_t* __restrict__ table, uint32_t* __restrict__ prefix, uint32_t NB, CaListed listed) {
    extern __shared__ uint32_t ca_lds[];  // [256] partial sums
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (!ca_bit(listed.w, k)) return;
    const uint32_t chunk = (NB + 255u) / 256u;
    const uint32_t lo = t * chunk < NB ? t * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    const uint32_t* row = table + (uint64_t)k * NB;
    uint32_t s = 0;
    for (uint32_t w = lo; w < hi; w++) s += row[w];
    ca_lds[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 256; i++) { const uint32_t v = ca_lds[i]; ca_lds[i] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = ca_lds[t];
    uint32_t* out = prefix + (uint64_t)k * NB;
    for (uint32_t w = lo; w < hi; w++) { out[w] = run; run += row[w]; }
}

// list: rows[k * R + rank] = the rank-th failing row of listed constraint k, rank < R
template <int CHIP>
__global__ void __launch_bounds__(256) k_ca_list(CaArgs a, const uint32_t* __restrict__ table, const uint32_t* __restrict__ prefix, CaListed listed, uint32_t R,
                                                 uint32_t* __restrict__ rows) {
    extern __shared__ uint32_t ca_lds[];  // [0] flag, [CA_LDS_HEAD ..) masks [CA_MASK_WORDS][T], then the interpreter's register file
    const uint32_t T = blockDim.x, t = threadIdx.x;
    if (t == 0) ca_lds[0] = 0;
    __syncthreads();
    // constraint k belongs to thread k mod T; it is walked here when it is listed, fails in this workgroup, and still has ranks below R to hand out
    for (uint32_t k = t; k < a.K; k += T)
        if (ca_bit(listed.w, k) && table[(uint64_t)k * a.NB + blockIdx.x] != 0 && prefix[(uint64_t)k * a.NB + blockIdx.x] < R) ca_lds[0] = 1;
    __syncthreads();
    if (!ca_lds[0]) return;  // the whole workgroup
    uint32_t* masks = ca_lds + CA_LDS_HEAD;
    const uint64_t r = (uint64_t)blockIdx.x * T + t;
    CaMask m;
    m.clear();
    if (r < a.n) m = ca_eval_row<CHIP>(a, r, 0xffffffffu, nullptr, masks + CA_MASK_WORDS * T + t, T);
#pragma unroll
    for (int i = 0; i < (int)CA_MASK_WORDS; i++) masks[i * T + t] = m.w[i];
    __syncthreads();
    for (uint32_t k = t; k < a.K; k += T) {
        if (!ca_bit(listed.w, k) || table[(uint64_t)k * a.NB + blockIdx.x] == 0) continue;
        const uint32_t* mw = masks + (k >> 5) * T;  // LDS
        uint32_t rank = prefix[(uint64_t)k * a.NB + blockIdx.x];
        for (uint32_t j = 0; j < T && rank < R; j++)
            if ((mw[j] >> (k & 31u)) & 1u) rows[(uint64_t)k * R + rank++] = (uint32_t)((uint64_t)blockIdx.x * T + j);
    }
}

// values: thread (k, rank) of a listed constraint evaluates rows[k * R + rank] and keeps constraint k's value (canonical)
template <int CHIP>
__global__ void __launch_bounds__(256) k_ca_values(CaArgs a, const unsigned long long* __restrict__ totals, CaListed listed, uint32_t R, const uint32_t* __restrict__ rows,
                                                   uint32_t* __restrict__ values) {
    extern __shared__ uint32_t ca_lds[];  // the interpreter's register file [n_regs][blockDim.x]
    const uint32_t T = blockDim.x, t = threadIdx.x;
    const uint64_t id = (uint64_t)blockIdx.x * T + t;
    const uint32_t k = (uint32_t)(id / R), rank = (uint32_t)(id % R);
    if (k >= a.K || !ca_bit(listed.w, k) || (unsigned long long)rank >= totals[k]) return;
    const uint32_t row = rows[id];
    if (row >= a.n) return;  // cannot happen (list wrote it); keeps the loads in bounds whatever the buffer holds
    Fp v = Fp::zero();
    ca_eval_row<CHIP>(a, row, k, &v, ca_lds + t, T);
    values[id] = v.canonical();
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
uint32_t ca_block_threads(const CaArgs& a) {
    if (a.native_chip != CA_INTERPRET) return 256;
    uint32_t T = 256;
    while (T > 64 && (size_t)(a.n_regs + CA_MASK_WORDS) * T * 4 + CA_LDS_HEAD * 4 > 64 * 1024) T >>= 1;
    if ((size_t)(a.n_regs + CA_MASK_WORDS) * T * 4 + CA_LDS_HEAD * 4 > 160 * 1024) throw std::invalid_argument("constraint_audit: the constraint program needs more registers than a workgroup's LDS holds");
    return T;
}

#define CA_CHIPS(X)                                                                                                                          \
    X(CHIP_CPU) X(CHIP_ADD) X(CHIP_SUB) X(CHIP_MUL) X(CHIP_SHIFT) X(CHIP_LT) X(CHIP_COM) X(CHIP_BITWISE) X(CHIP_OUTPUT) X(CHIP_STATIC_DATA)

static void ca_check(const CaArgs& a) {
    if (a.K == 0 || a.K > CA_MAX_CONSTRAINTS) throw std::invalid_argument("constraint_audit: the device audit handles 1.." + std::to_string(CA_MAX_CONSTRAINTS) + " constraints per chip");
    if (a.n == 0 || (a.n & (a.n - 1)) || a.NB != (uint32_t)((a.n + a.T - 1) / a.T)) throw std::logic_error("constraint_audit: inconsistent launch shape");
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)k_ca_count<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_ca_list<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute((const void*)k_ca_values<CA_INTERPRET>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr = true;
    }
}

void launch_ca_count(hipStream_t st, const CaArgs& a, unsigned long long* totals, uint32_t* table) {
    ca_check(a);
    const dim3 grid(a.NB), block(a.T);
    static const char* names[14] = {"k_ca_count.cpu", "k_ca_count.program", "k_ca_count.mem", "k_ca_count.add", "k_ca_count.sub", "k_ca_count.mul", "k_ca_count.div", "k_ca_count.shift",
                                    "k_ca_count.lt", "k_ca_count.com", "k_ca_count.bitwise", "k_ca_count.output", "k_ca_count.range", "k_ca_count.static_data"};
    ProfScope ps(a.native_chip >= 0 && a.native_chip < 14 ? names[a.native_chip] : "k_ca_count", st, 4.0 * (double)a.n * (a.width + a.prep_width));  // the profile's per-chip split
    switch (a.native_chip) {
#define CA_X(C) case vchips::C: VK_LAUNCH((k_ca_count<vchips::C>), grid, block, CA_LDS_HEAD * 4, st, a, totals, table); break;
        CA_CHIPS(CA_X)
#undef CA_X
        case CA_INTERPRET: VK_LAUNCH((k_ca_count<CA_INTERPRET>), grid, block, (CA_LDS_HEAD + (size_t)a.n_regs * a.T) * 4, st, a, totals, table); break;
        default: throw std::logic_error("constraint_audit: a native chip id without constraints");
    }
}

void launch_ca_scan(hipStream_t st, const CaArgs& a, const uint32_t* table, uint32_t* prefix, const CaListed& listed) {
    ca_check(a);
    ProfScope ps("k_ca_scan", st, 8.0 * (double)a.NB);
    VK_LAUNCH(k_ca_scan, dim3(a.K), dim3(256), 256 * 4, st, table, prefix, a.NB, listed);
}

void launch_ca_list(hipStream_t st, const CaArgs& a, const uint32_t* table, const uint32_t* prefix, const CaListed& listed, uint32_t R, uint32_t* rows) {
    ca_check(a);
    const dim3 grid(a.NB), block(a.T);
    const size_t lds = (CA_LDS_HEAD + (size_t)CA_MASK_WORDS * a.T) * 4;
    ProfScope ps("k_ca_list", st, 0);
    switch (a.native_chip) {
#define CA_X(C) case vchips::C: VK_LAUNCH((k_ca_list<vchips::C>), grid, block, lds, st, a, table, prefix, listed, R, rows); break;
        CA_CHIPS(CA_X)
#undef CA_X
        case CA_INTERPRET: VK_LAUNCH((k_ca_list<CA_INTERPRET>), grid, block, lds + (size_t)a.n_regs * a.T * 4, st, a, table, prefix, listed, R, rows); break;
        default: throw std::logic_error("constraint_audit: a native chip id without constraints");
    }
}

void launch_ca_values(hipStream_t st, const CaArgs& a, const unsigned long long* totals, const CaListed& listed, uint32_t R, const uint32_t* rows, uint32_t* values) {
    ca_check(a);
    const uint64_t n_threads = (uint64_t)a.K * R;
    const dim3 grid((unsigned)((n_threads + a.T - 1) / a.T)), block(a.T);
    ProfScope ps("k_ca_values", st, 0);
    switch (a.native_chip) {
#define CA_X(C) case vchips::C: VK_LAUNCH((k_ca_values<vchips::C>), grid, block, 4, st, a, totals, listed, R, rows, values); break;
        CA_CHIPS(CA_X)
#undef CA_X
        case CA_INTERPRET: VK_LAUNCH((k_ca_values<CA_INTERPRET>), grid, block, ((size_t)a.n_regs * a.T + 1) * 4, st, a, totals, listed, R, rows, values); break;
        default: throw std::logic_error("constraint_audit: a native chip id without constraints");
    }
}

}  // namespace vk
