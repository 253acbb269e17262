// The trace kernels of valida_amd/csrc/kernels/tracegen.hip — the very source — compiled for the HOST under tools/hipemu and run on operation
// logs: k_tracegen_cpu against the host's CpuChip::generate_trace (tests/test_executable_cpu.py), and every kernel but the radix sort against
// the Python reference on the synthetic corpus (tests/test_tracegen_edges_cpu.py).  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#define HIPEMU_STATIC_SHARED 1  // the histograms' static LDS tables: one per workgroup, zeroed by the kernel itself before its first barrier
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

// the radix sort's scatter needs a wave primitive the emulator does not model (__ballot): compiled, never launched here.  The histograms
// need only barriers and atomics: a block's fibers run one at a time, so a plain read-modify-write is atomic.
inline unsigned long long __ballot(int) { throw std::runtime_error("hipemu: wave intrinsic (__ballot) reached"); }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }  // fibers of one block never interleave inside a call
enum { hipErrorInvalidValue = 1 };
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { std::memset(p, v, n); return hipSuccess; }

#include "../../valida_amd/csrc/kernels/tracegen.hip"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

template <class F> static int emu_run(uint64_t height, uint64_t w, uint32_t* out, F&& launch) {
    try {
        std::vector<uint32_t> cols(height * w);
        launch(vk::DMatView{cols.data(), height, w, height});
        for (uint64_t r = 0; r < height; r++)
            for (uint64_t c = 0; c < w; c++) out[r * w + c] = vg::Fp::raw(cols[c * height + r]).canonical();
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

extern "C" {
// out (height x NUM_COLS, row-major canonical) = the cpu trace k_tracegen_cpu writes for the logs (C ABI images: vgpu_cpu_op_t, vgpu_mem_op_t).
// Returns 0, or -1 when the emulator refused (a wave primitive reached, an out-of-bounds access under HIPEMU_CHECKS).
int emu_tracegen_cpu(const uint32_t* ops, uint64_t n, const uint32_t* mem, uint64_t n_mem, uint64_t height, uint32_t* out) {
    try {
        const uint64_t w = vchips::cpu::NUM_COLS;
        std::vector<uint32_t> cols(height * w);
        vk::launch_tracegen_cpu(nullptr, (const vk::TgCpuOp*)ops, n, (const vk::TgMemOp*)mem, n_mem, vk::DMatView{cols.data(), height, w, height});
        for (uint64_t r = 0; r < height; r++)
            for (uint64_t c = 0; c < w; c++) out[r * w + c] = vg::Fp::raw(cols[c * height + r]).canonical();
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

// ---- the other generators: out = the trace, row-major canonical (height x the chip's width); -1 when the emulator refused ----------------
// chip: a vchips::ChipId of add / sub / lt / bitwise (k_tracegen_alu) or mul / div / shift / com (k_tracegen_alu2)
int emu_tracegen_alu(int chip, const uint32_t* ops, uint64_t n, uint64_t height, uint64_t width, uint32_t* out) {
    using namespace vchips;
    if (chip_info(chip).width != (int)width) return -2;
    const bool first = chip == CHIP_ADD || chip == CHIP_SUB || chip == CHIP_LT || chip == CHIP_BITWISE;
    return emu_run(height, width, out, [&](vk::DMatView t) {
        if (first) vk::launch_tracegen_alu(nullptr, chip, (const vk::TgAluOp*)ops, n, t);
        else vk::launch_tracegen_alu2(nullptr, chip, (const vk::TgAluOp*)ops, n, t);
    });
}
// order: the memory log's (addr, issue order) permutation, computed by the caller (k_rs_scatter is device-only)
int emu_tracegen_mem(const uint32_t* mem, const uint32_t* order, uint64_t n, const uint32_t* static_cells, uint64_t n_static, uint64_t height, uint32_t* out) {
    return emu_run(height, vchips::mem::NUM_COLS, out, [&](vk::DMatView t) {
        VK_LAUNCH(vk::k_tracegen_mem, dim3(vk::blocks_for(height)), dim3(256), 0, nullptr, (const vk::TgMemOp*)mem, order, n, static_cells, n_static, t);
    });
}
int emu_tracegen_output(const uint32_t* vals, const uint32_t* row0, uint64_t n, uint64_t n_rows, uint64_t height, uint32_t* out) {
    return emu_run(height, vchips::output::NUM_COLS, out, [&](vk::DMatView t) { vk::launch_tracegen_output(nullptr, (const vk::TgOutOp*)vals, row0, n, n_rows, t); });
}
int emu_tracegen_idle(int mode, const uint32_t* static_cells, uint64_t n_static, uint64_t height, uint64_t width, uint32_t* out) {
    return emu_run(height, width, out, [&](vk::DMatView t) { vk::launch_tracegen_idle(nullptr, mode, static_cells, n_static, t); });
}
int emu_tracegen_counts(const uint32_t* counts, uint64_t n_counts, int with_counter, uint64_t height, uint32_t* out) {
    return emu_run(height, with_counter ? 2 : 1, out, [&](vk::DMatView t) {
        VK_LAUNCH(vk::k_tracegen_counts, dim3(vk::blocks_for(height)), dim3(256), 0, nullptr, counts, n_counts, with_counter, t);
    });
}
// k_tg_range_histogram + k_tracegen_counts, as launch_tracegen_range chains them (the grid capped at 1024 blocks)
int emu_tracegen_range(const uint32_t* ops, uint64_t n, const uint32_t* mem, uint64_t n_mem, uint32_t* out) {
    std::vector<uint32_t> counts(256, 0xdeadbeefu);
    return emu_run(256, vchips::range::NUM_COLS, out, [&](vk::DMatView t) {
        if (vk::launch_tracegen_range(nullptr, (const vk::TgCpuOp*)ops, n, (const vk::TgMemOp*)mem, n_mem, counts.data(), t) != hipSuccess) throw std::runtime_error("launch");
    });
}
// k_tg_pc_histogram + k_tracegen_counts, as launch_tracegen_program chains them
int emu_tracegen_program(const uint32_t* ops, uint64_t n, uint64_t padded_n, uint32_t rom_len, uint64_t height, uint32_t* out) {
    std::vector<uint32_t> counts(rom_len > 256 ? rom_len : 256, 0xdeadbeefu);
    return emu_run(height, vchips::program::NUM_COLS, out, [&](vk::DMatView t) {
        if (vk::launch_tracegen_program(nullptr, (const vk::TgCpuOp*)ops, n, padded_n, rom_len, counts.data(), t) != hipSuccess) throw std::runtime_error("launch");
    });
}
}
