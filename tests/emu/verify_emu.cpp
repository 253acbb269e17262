// The batched verifier's kernels (valida_amd/csrc/kernels/verify.hip) compiled for the HOST under tools/hipemu, driven by the product's host
// half (host/verify_batch.hpp: plans, packing, first-failure resolution): vgpu_verify_batch with the device stage replaced by the same
// kernels launched through the emulator.  Checked against vgpu_verify (tests/test_verify_batch_emu_cpu.py).  Built with -DVK_ALIGNBIT_NOP=0
// (the no-op rides on an inline-asm statement only the device compiler understands).  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include "../../valida_amd/csrc/kernels/verify.hip"
#include "../../valida_amd/csrc/host/poseidon_opt.hpp"
#include "../../valida_amd/csrc/host/verify_batch.hpp"

namespace vk {
uint32_t lds[16];
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

// the layout of the library's machine handle (valida_amd/csrc/capi.cpp): the test hands in a vgpu_machine_t* of the loaded library, built
// from the same headers
struct vgpu_machine { vhost::MachineDesc desc; };

extern "C" {
// Machine::verify of n proofs through the emulated kernels.  status[i]: 0 accepted, 1 rejected with its message in msgs + i * msg_cap
// (NUL-terminated, truncated to msg_cap - 1 bytes).  Returns 0, or -1 when the call itself failed (the message in msgs).
int emu_verify_batch(const void* machine, uint32_t log_blowup, uint32_t num_queries, uint32_t pow_bits, uint32_t hash_kind, uint32_t observe_final_poly,
                     const uint32_t* rc480, const uint32_t* const* proofs, const uint64_t* n_words, const uint32_t* prep_commits, uint32_t n, uint64_t chunk_words,
                     int32_t* status, char* msgs, uint64_t msg_cap) {
    try {
        vhost::Poseidon16 perm(rc480);
        bool sparse = false;
        const std::vector<uint32_t> pos = vhost::poseidon_device_image(rc480, perm, sparse);
        vhost::FriParams fri;
        fri.log_blowup = log_blowup; fri.num_queries = num_queries; fri.pow_bits = pow_bits;
        fri.observe_final_poly = observe_final_poly != 0; fri.hash_kind = (int)hash_kind;
        vhost::VerifyStage stage = [&](const vhost::VerifyChunk& c) {
            std::vector<uint32_t> buf(c.total_words()), flags(c.n_flags, 0xFFFFFFFFu);
            for (const vhost::VerifyChunk::Span& sp : c.spans) memcpy(buf.data() + sp.at, sp.words, sp.n * 4);
            memcpy(buf.data() + c.proof_words, c.buf.data(), c.buf.size() * 4);
            vk::launch_verify_chunk(nullptr, c.args(buf.data(), flags.data(), (int)hash_kind, pos.data(), sparse));
            for (uint32_t f : flags) if (f > 1) throw std::runtime_error("a flag was not written");
            return flags;
        };
        const auto res = vhost::verify_machine_batch(static_cast<const vgpu_machine*>(machine)->desc, fri, perm, proofs, n_words, prep_commits, n, stage,
                                                     chunk_words ? chunk_words : vhost::VERIFY_CHUNK_WORDS_DEFAULT);
        for (uint32_t i = 0; i < n; i++) {
            status[i] = res[i].ok ? 0 : 1;
            snprintf(msgs + i * msg_cap, msg_cap, "%s", res[i].msg.c_str());
        }
        return 0;
    } catch (const std::exception& e) {
        snprintf(msgs, msg_cap, "%s", e.what());
        return -1;
    }
}
}
