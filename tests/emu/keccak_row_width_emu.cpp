// The compile-time row widths of valida_amd/csrc/kernels/merkle.hip (hash_row<Cols, N>, k_keccak_leaves<Cols, N>, k_keccak_compress<N>) compiled for
// the HOST under tools/hipemu, next to the run-time width (N = 0) of the same source: as tests/emu/keccak_emu.cpp, -DVK_ALIGNBIT_NOP=0.
// hash_row is instantiated here for the widths of the product's tables AND for the widths where padding can go wrong (1, 2, 32, 33, 34, 35);
// the product's launchers are reached too, so their dispatch on n_elems runs.  Checked against the oracle's Keccak MMCS
// (tests/test_keccak_row_width_cpu.py).  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include "../../valida_amd/csrc/kernels/merkle.hip"

namespace vk {
uint32_t lds[16];
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using vg::Fp;

// every width of VK_LEAF_WIDTHS / VK_INJECT_WIDTHS plus the padding edge cases
#define EMU_WIDTHS(X) X(1) X(2) X(10) X(14) X(20) X(25) X(32) X(33) X(34) X(35) X(40) X(51) X(55) X(61) X(67) X(95)

namespace {
// row-major canonical h x w -> column-major Montgomery, and the column pointers
struct Columns {
    std::vector<uint32_t> data;
    std::vector<const uint32_t*> ptr;
    uint64_t h;
    Columns(const uint32_t* rows, uint64_t h_, int w) : data((size_t)h_ * w + 1), h(h_) {
        for (uint64_t r = 0; r < h; r++) for (int j = 0; j < w; j++) data[(size_t)j * h + r] = Fp::from_canonical(rows[r * w + j]).v;
        for (int j = 0; j < w; j++) ptr.push_back(data.data() + (size_t)j * h);
    }
};
template <class Cols> bool rows_fixed(const Cols cols, int w, uint64_t h, uint32_t* digests) {
    for (uint64_t r = 0; r < h; r++) {
        uint32_t d[8];
        switch (w) {
#define X(W) case W: vk::hash_row<Cols, W>(cols, w, r, d); break;
            EMU_WIDTHS(X)
#undef X
            default: return false;
        }
        memcpy(digests + 8 * r, d, 32);
    }
    return true;
}
}  // namespace

extern "C" {
// digests[r] = H(row r) of the row-major canonical matrix `rows` (h x w).  mode 0: hash_row<PtrCols, 0>, 1: hash_row<PtrCols, w>,
// 2: hash_row<StridedCols, w> (0, or -1: no instance of that width here); 3 / 4: the product's dispatch on n_elems over a column list / a strided
// matrix, returning the width compiled into the kernel instance it launched (0: the generic one); 5 / 6: launch_keccak_leaves / _strided themselves.
int emu_row_digests(int mode, const uint32_t* rows, uint64_t h, int w, uint32_t* digests) {
    Columns c(rows, h, w);
    if (mode == 0) {
        for (uint64_t r = 0; r < h; r++) {
            uint32_t d[8];
            vk::hash_row<vk::PtrCols, 0>(vk::PtrCols{c.ptr.data()}, w, r, d);
            memcpy(digests + 8 * r, d, 32);
        }
        return 0;
    }
    if (mode == 1) return rows_fixed(vk::PtrCols{c.ptr.data()}, w, h, digests) ? 0 : -1;
    if (mode == 2) return rows_fixed(vk::StridedCols{c.data.data(), h}, w, h, digests) ? 0 : -1;
    if (mode == 3) return vk::launch_leaves_instance(nullptr, vk::PtrCols{c.ptr.data()}, w, h, digests);
    if (mode == 4) return vk::launch_leaves_instance(nullptr, vk::StridedCols{c.data.data(), h}, w, h, digests);
    if (mode == 5) { vk::launch_keccak_leaves(nullptr, c.ptr.data(), w, h, digests); return 0; }
    if (mode == 6) { vk::launch_keccak_leaves_strided(nullptr, c.data.data(), h, w, h, digests); return 0; }
    return -2;
}
// next[i] = C(C(prev[2 i], prev[2 i + 1]), H(row i of low)) for the n_out rows of the row-major canonical matrix `low` (n_out x w).
// mode 0: k_keccak_compress<0>, 1: k_keccak_compress<w>, 3: the product's dispatch (returns the instance's width), 5: launch_keccak_compress itself
int emu_compress_layer(int mode, const uint32_t* prev, const uint32_t* low, uint64_t n_out, int w, uint32_t* next) {
    Columns c(low, n_out, w);
    const dim3 grid((unsigned)((n_out + 255) / 256)), block(256);
    if (mode == 0) { hipLaunchKernelGGL(vk::k_keccak_compress<0>, grid, block, 0, nullptr, prev, c.ptr.data(), w, n_out, next); return 0; }
    if (mode == 3) return vk::launch_compress_instance(nullptr, prev, c.ptr.data(), w, n_out, next);
    if (mode == 5) { vk::launch_keccak_compress(nullptr, prev, c.ptr.data(), w, n_out, next); return 0; }
    if (mode != 1) return -2;
    switch (w) {
#define X(W) case W: hipLaunchKernelGGL(vk::k_keccak_compress<W>, grid, block, 0, nullptr, prev, c.ptr.data(), w, n_out, next); return 0;
        EMU_WIDTHS(X)
#undef X
    }
    return -1;
}
}
