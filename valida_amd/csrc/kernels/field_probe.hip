// Field probe: the primitives of field.hpp, butterfly.hpp and poseidon_perm.hpp — the very functions the kernels call, so on the device the
// carry-out / v_cndmask corrections and the signed products through __mulhi are what runs — applied to operands the caller chooses, one work
// item per operand tuple.  Operands and results are RAW STORED WORDS: nothing converts them on the way in or out, so a test can hand a
// primitive the extreme words of its domain (0, p - 1, the lazy range up to 2p - 1, a reduction's largest high word) that seeded canonical
// inputs reach with probability 2^-31 (tests/test_field_edges_gpu.py; the same source under tools/hipemu: tests/test_field_edges_cpu.py).
// Operands come from memory, so nothing folds.  Word k of item i sits at in[k * n + i] / out[k * n + i].  Test hook (vgpu_field_probe);
// nothing in the proving path launches it.
#include "launch.hpp"
#include "poseidon_perm.hpp"
#include <stdexcept>

namespace vk {

bool field_probe_shape(uint32_t op, int* in_words, int* out_words) {
    static const int shape[FIELD_PROBE_OPS][2] = {
        {1, 1}, {2, 1}, {2, 1}, {2, 1}, {1, 1}, {2, 1}, {2, 1}, {2, 1}, {1, 1}, {1, 1}, {1, 1},  // reduce_once .. inv
        {10, 5}, {5, 5}, {6, 5}, {5, 5},                                                         // Ext5
        {18, 16}, {18, 16}, {18, 16}, {18, 16},                                                  // butterflies<4>
        {2, 1}, {1, 1}, {2, 1},                                                                  // signed products, S-box
        {16, 16}, {16, 16},                                                                      // permutation
    };
    if (op >= (uint32_t)FIELD_PROBE_OPS) return false;
    *in_words = shape[op][0];
    *out_words = shape[op][1];
    return true;
}

void field_probe_check_twiddle_range(uint32_t op, const uint32_t* in_host, uint64_t n) {
    if (op < (uint32_t)FP_BFLY_DIT_LB0 || op > (uint32_t)FP_BFLY_DIF) return;
    const bool lb0 = op == (uint32_t)FP_BFLY_DIT_LB0 || op == (uint32_t)FP_BFLY_DIF_LB0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t low = in_host[16 * n + i], lowbits = in_host[17 * n + i];
        if (lowbits > 10 || low >= (1u << lowbits) || (lb0 && lowbits != 0)) throw std::invalid_argument("field probe: low / lowbits outside the twiddle tables");
    }
}

template <int OP>
__global__ void __launch_bounds__(256) k_field_probe(const uint32_t* __restrict__ in, uint64_t n, DeviceTables tb, PoseidonTab tab, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto a = [&](int k) { return in[(uint64_t)k * n + i]; };
    auto put = [&](int k, uint32_t v) { out[(uint64_t)k * n + i] = v; };
    auto ext = [&](int k0) { Ext5 e; for (int k = 0; k < 5; k++) e.c[k] = Fp::raw(a(k0 + k)); return e; };
    auto put_e = [&](const Ext5& e) { for (int k = 0; k < 5; k++) put(k, e.c[k].v); };
    if constexpr (OP == FP_REDUCE_ONCE) put(0, vg::reduce_once(a(0)));
    else if constexpr (OP == FP_SUB_MOD) put(0, vg::sub_mod(a(0), a(1)));
    else if constexpr (OP == FP_ADD) put(0, (Fp::raw(a(0)) + Fp::raw(a(1))).v);
    else if constexpr (OP == FP_SUB) put(0, (Fp::raw(a(0)) - Fp::raw(a(1))).v);
    else if constexpr (OP == FP_NEG) put(0, (-Fp::raw(a(0))).v);
    else if constexpr (OP == FP_MUL) put(0, (Fp::raw(a(0)) * Fp::raw(a(1))).v);
    else if constexpr (OP == FP_MONTY_REDUCE) put(0, vg::monty_reduce(((uint64_t)a(1) << 32) | a(0)));
    else if constexpr (OP == FP_MONTY_REDUCE_WIDE) put(0, vg::monty_reduce_wide(((uint64_t)a(1) << 32) | a(0)));
    else if constexpr (OP == FP_FROM_CANONICAL) put(0, Fp::from_canonical(a(0)).v);
    else if constexpr (OP == FP_CANONICAL) put(0, Fp::raw(a(0)).canonical());
    else if constexpr (OP == FP_INV) put(0, Fp::raw(a(0)).inv().v);
    else if constexpr (OP == FP_EXT_MUL) put_e(ext(0) * ext(5));
    else if constexpr (OP == FP_EXT_SQUARE) put_e(ext(0).square());
    else if constexpr (OP == FP_EXT_SCALE) put_e(ext(0) * Fp::raw(a(5)));
    else if constexpr (OP == FP_EXT_INV) put_e(ext(0).inv());
    else if constexpr (OP >= FP_BFLY_DIT_LB0 && OP <= FP_BFLY_DIF) {
        // words 16, 17: low and lowbits, 0, 0 in the LB0 forms.  Nothing here or in the launcher checks them against the twiddle tables' size: the caller
        // runs field_probe_check_twiddle_range on its host copy of the operands first (capi.cpp: vgpu_field_probe; tests/emu/field_probe_emu.cpp)
        constexpr bool DIT = OP == FP_BFLY_DIT_LB0 || OP == FP_BFLY_DIT, LB0 = OP == FP_BFLY_DIT_LB0 || OP == FP_BFLY_DIF_LB0;
        Fp x[16];
#pragma unroll
        for (int g = 0; g < 16; g++) x[g] = Fp::raw(a(g));
        butterflies<4, DIT, LB0>(x, DIT ? tb.twc : tb.itwc, (int)a(16), (int)a(17));
#pragma unroll
        for (int g = 0; g < 16; g++) put(g, x[g].v);
    }
    else if constexpr (OP == FP_MONTY_SIGNED) put(0, (uint32_t)monty_signed((int64_t)(((uint64_t)a(1) << 32) | a(0))));
    else if constexpr (OP == FP_SBOX) put(0, poseidon_sbox(Fp::raw(a(0))).v);
    else if constexpr (OP == FP_SBOX_PLUS) put(0, poseidon_sbox_plus(Fp::raw(a(0)), a(1)).v);
    else {  // FP_PERMUTE (the tables the library dispatches for this context), FP_PERMUTE_PLAIN (tab.opt == nullptr)
        Fp st[16];
#pragma unroll
        for (int g = 0; g < 16; g++) st[g] = Fp::raw(a(g));
        poseidon16_permute(st, tab);
#pragma unroll
        for (int g = 0; g < 16; g++) put(g, st[g].v);
    }
}

template <int OP>
static void probe_op(hipStream_t st, uint32_t op, const uint32_t* in, uint64_t n, const DeviceTables& tb, const PoseidonTab& tab, uint32_t* out) {
    if constexpr (OP < FIELD_PROBE_OPS) {
        if (op == (uint32_t)OP) { VK_LAUNCH(k_field_probe<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n, tb, tab, out); return; }
        probe_op<OP + 1>(st, op, in, n, tb, tab, out);
    }
}

void launch_field_probe(hipStream_t st, uint32_t op, const uint32_t* in_dev, uint64_t n, const DeviceTables& tb, const uint32_t* pos_dev, bool sparse, uint32_t* out_dev) {
    int iw, ow;
    if (!field_probe_shape(op, &iw, &ow)) throw std::invalid_argument("field probe: unknown op");
    if (!n) return;
    if (n > (1ull << 24)) throw std::invalid_argument("field probe: at most 2^24 items per launch");
    ProfScope ps("k_field_probe", st, 0.0);
    probe_op<0>(st, op, in_dev, n, tb, tab_of(pos_dev, sparse && op != (uint32_t)FP_PERMUTE_PLAIN), out_dev);
}

}  // namespace vk
