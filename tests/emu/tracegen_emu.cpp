// The cpu trace kernel of valida_amd/csrc/kernels/tracegen.hip (k_tracegen_cpu) — the very source — compiled for the HOST under tools/hipemu
// and run on the VM's operation logs; checked against the host's CpuChip::generate_trace (tests/test_executable_cpu.py).  Test infrastructure;
// nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

// the other kernels of the file (histograms, the radix sort) need wave and atomic primitives the emulator does not model; they are compiled,
// never launched here
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
}
