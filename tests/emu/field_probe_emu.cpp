// The field probe of valida_amd/csrc/kernels/field_probe.hip compiled for the HOST under tools/hipemu: the very kernel source with the plain
// C++ forms of reduce_once / sub_mod / the signed products (the device compiles inline assembly and __mulhi in their place), run on the corpus
// of tests/edge_corpus.py against tests/field_ref.py before any GPU minute is spent (tests/test_field_edges_cpu.py): corpus and reference
// agree, every operand is in its domain.  Test infrastructure; nothing in the product links it.
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include "../../valida_amd/csrc/kernels/field_probe.hip"
#include "../../valida_amd/csrc/host/poseidon_opt.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

namespace {
struct Tables {
    std::vector<uint32_t> image;
    vk::DeviceTables tb{};
    Tables() : image(vk::device_tables_words()) {
        vk::build_device_tables(tb, image.data());
        vk::bind_device_tables(tb, image.data());
    }
};
Tables& tables() { static Tables t; return t; }
}  // namespace

extern "C" {
// out = op on n items (the layout of vgpu_field_probe).  Returns 0, or 1 on an error; *sparse = the sparse-round tables were valid, i.e. op
// `permute` ran the schedule the library dispatches
int emu_field_probe(const uint32_t* rc480, uint32_t op, const uint32_t* in, uint64_t n, uint32_t* out, int* sparse) {
    try {
        vhost::Poseidon16 p(rc480);
        bool sp = false;
        const std::vector<uint32_t> pos = vhost::poseidon_device_image(rc480, p, sp);
        vk::field_probe_check_twiddle_range(op, in, n);
        vk::launch_field_probe(nullptr, op, in, n, tables().tb, pos.data(), sp, out);
        if (sparse) *sparse = sp ? 1 : 0;
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_field_probe: %s\n", e.what());
        return 1;
    }
}
// words per item of `op` as the kernel source has them (vk::field_probe_shape); 0 when `op` is past the last one
int emu_field_probe_shape(uint32_t op, int* in_words, int* out_words) { return vk::field_probe_shape(op, in_words, out_words) ? 1 : 0; }
}
