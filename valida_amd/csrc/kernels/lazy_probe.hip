// Lazy-sum probe: vg::fold_hi, the Ext5 product and the lazily folded sums of field.hpp (vg::LazyAcc / vg::ExtAcc) — the very functions the
// reduced openings, the quotient's folder and the permutation kernels call — on operands the caller chooses, one work item per tuple, in the
// manner of field_probe.hip: operands and results are RAW STORED WORDS, word k of item i at in[k * n + i] / out[k * n + i], operands come from
// memory so nothing folds.  The sums are instantiated per LENGTH, fully unrolled, because that is how the kernels use them: the fold state of a
// sum is then a compile-time constant at every multiply-add; LP_LIN_DOT_LOOP is the same sum in a rolled loop (the state a run-time scalar), as
// the row kernel of the reduced openings has it.  Test hook (vgpu_lazy_probe); nothing in the proving path launches it.
//   LP_FOLD_HI       (lo, hi)                      -> (lo, hi) of fold_hi(hi 2^32 + lo); hi < 2p
//   LP_EXT_MUL       a[5], b[5]                    -> a * b
//   LP_LIN_DOT       n x { A_c[5], v_c }           -> sum_c A_c * v_c     (Ext5 x base word), n = 1 .. 17 and 34
//   LP_EXT_DOT       n x { A_k[5], C_k[5] }        -> sum_k A_k * C_k     (Ext5 x Ext5), n = 1 .. 8
//   LP_LIN_DOT_LOOP  n x { A_c[5], v_c }           -> the same as LP_LIN_DOT, rolled, n = 1 .. 64
#include "launch.hpp"
#include <stdexcept>

namespace vk {

bool lazy_probe_shape(uint32_t op, uint32_t terms, int* in_words, int* out_words) {
    switch (op) {
        case LP_FOLD_HI: if (terms != 0) return false; *in_words = 2; *out_words = 2; return true;
        case LP_EXT_MUL: if (terms != 0) return false; *in_words = 10; *out_words = 5; return true;
        case LP_LIN_DOT: if (!((terms >= 1 && terms <= 17) || terms == 34)) return false; *in_words = 6 * (int)terms; *out_words = 5; return true;
        case LP_EXT_DOT: if (terms < 1 || terms > 8) return false; *in_words = 10 * (int)terms; *out_words = 5; return true;
        case LP_LIN_DOT_LOOP: if (terms < 1 || terms > 64) return false; *in_words = 6 * (int)terms; *out_words = 5; return true;
        default: return false;
    }
}

template <int OP, int N>
__global__ void __launch_bounds__(256) k_lazy_probe(const uint32_t* __restrict__ in, uint64_t n, uint32_t terms, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto a = [&](int k) { return in[(uint64_t)k * n + i]; };
    auto put = [&](int k, uint32_t v) { out[(uint64_t)k * n + i] = v; };
    auto ext = [&](int k0) { Ext5 e; for (int k = 0; k < 5; k++) e.c[k] = Fp::raw(a(k0 + k)); return e; };
    auto put_e = [&](const Ext5& e) { for (int k = 0; k < 5; k++) put(k, e.c[k].v); };
    if constexpr (OP == LP_FOLD_HI) {
        const uint64_t t = vg::fold_hi(((uint64_t)a(1) << 32) | a(0));
        put(0, (uint32_t)t);
        put(1, (uint32_t)(t >> 32));
    } else if constexpr (OP == LP_EXT_MUL) {
        put_e(ext(0) * ext(5));
    } else if constexpr (OP == LP_LIN_DOT) {
        vg::ExtAcc acc = vg::ExtAcc::zero();
#pragma unroll
        for (int c = 0; c < N; c++) acc.mac(ext(6 * c), Fp::raw(a(6 * c + 5)));
        put_e(acc.reduce());
    } else if constexpr (OP == LP_EXT_DOT) {
        vg::ExtAcc acc = vg::ExtAcc::zero();
#pragma unroll
        for (int c = 0; c < N; c++) acc.mac(ext(10 * c), ext(10 * c + 5));
        put_e(acc.reduce());
    } else {
        vg::ExtAcc acc = vg::ExtAcc::zero();
#pragma unroll 1
        for (uint32_t c = 0; c < terms; c++) acc.mac(ext(6 * (int)c), Fp::raw(a(6 * (int)c + 5)));
        put_e(acc.reduce());
    }
}

template <int OP, int N, int NMAX>
static void lazy_probe_terms(hipStream_t st, uint32_t terms, const uint32_t* in, uint64_t n, uint32_t* out) {
    if constexpr (N <= NMAX) {
        if (terms == (uint32_t)N) { VK_LAUNCH((k_lazy_probe<OP, N>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n, terms, out); return; }
        lazy_probe_terms<OP, N + 1, NMAX>(st, terms, in, n, out);
    }
}

void launch_lazy_probe(hipStream_t st, uint32_t op, uint32_t terms, const uint32_t* in_dev, uint64_t n, uint32_t* out_dev) {
    int iw, ow;
    if (!lazy_probe_shape(op, terms, &iw, &ow)) throw std::invalid_argument("lazy probe: unknown op or length");
    if (!n) return;
    if (n > (1ull << 24)) throw std::invalid_argument("lazy probe: at most 2^24 items per launch");
    ProfScope ps("k_lazy_probe", st, 0.0);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    switch (op) {
        case LP_FOLD_HI: VK_LAUNCH((k_lazy_probe<LP_FOLD_HI, 0>), grid, block, 0, st, in_dev, n, terms, out_dev); break;
        case LP_EXT_MUL: VK_LAUNCH((k_lazy_probe<LP_EXT_MUL, 0>), grid, block, 0, st, in_dev, n, terms, out_dev); break;
        case LP_LIN_DOT:
            if (terms == 34) VK_LAUNCH((k_lazy_probe<LP_LIN_DOT, 34>), grid, block, 0, st, in_dev, n, terms, out_dev);
            else lazy_probe_terms<LP_LIN_DOT, 1, 17>(st, terms, in_dev, n, out_dev);
            break;
        case LP_EXT_DOT: lazy_probe_terms<LP_EXT_DOT, 1, 8>(st, terms, in_dev, n, out_dev); break;
        default: VK_LAUNCH((k_lazy_probe<LP_LIN_DOT_LOOP, 0>), grid, block, 0, st, in_dev, n, terms, out_dev); break;
    }
}

}  // namespace vk
