// The lazy-sum probe of valida_amd/csrc/kernels/lazy_probe.hip compiled for the HOST under tools/hipemu: the very kernel source with the plain C++
// form of reduce_once (the device compiles carry-out + v_cndmask inline assembly in its place), run on the corpus of tests/lazy_corpus.py against
// its plain-integer reference before any GPU minute is spent (tests/test_lazy_sums_cpu.py).  Test infrastructure; nothing in the product links it.
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include "../../valida_amd/csrc/kernels/lazy_probe.hip"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

extern "C" {
// out = op on n items (the layout of vgpu_lazy_probe).  Returns 0, or 1 on an error
int emu_lazy_probe(uint32_t op, uint32_t terms, const uint32_t* in, uint64_t n, uint32_t* out) {
    try {
        vk::launch_lazy_probe(nullptr, op, terms, in, n, out);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_lazy_probe: %s\n", e.what());
        return 1;
    }
}
// words per item of `op` at length `terms` as the kernel source has them (vk::lazy_probe_shape); 0: no such op / length
int emu_lazy_probe_shape(uint32_t op, uint32_t terms, int* in_words, int* out_words) { return vk::lazy_probe_shape(op, terms, in_words, out_words) ? 1 : 0; }
}
