// Constant columns in the fused LDE, on the HOST: k_ingest with its column flags (valida_amd/csrc/kernels/layout.hip), k_lde_colmap, k_lde_fill_const
// and the mapped three-pass LDE (valida_amd/csrc/kernels/ntt.hip) — the very kernel sources — run under tools/hipemu, as tests/emu/ntt_emu.cpp runs
// the unmapped ones.  A program of its own (own main), built by tests/test_lde_const_columns_cpu.py with AddressSanitizer + UBSan and run directly.
//   lde_colmap_emu CASES.bin
// CASES.bin (32-bit words): [number of cases], then per case [log_n, w, log_blowup, shift], the matrix (n x w row-major canonical), the expected
// constant-column mask (w words, 1 = every row equals row 0) and the expected committed LDE ((n << log_blowup) x w row-major canonical: the oracle's).
// Per case, with and without the map: the LDE equals the expected one word for word; the flags equal the mask; the map lists the live and the constant
// columns ascending; the scratch matrices are used compactly (no pass writes a scratch column >= live_count: with every column constant no transform
// launch touches memory at all).  Exit status 0 = every check held.
#define HIPEMU_CHECKS 1
#define HIPEMU_STACK_BYTES (32 * 1024)  // these kernels keep a few dozen words per thread; under AddressSanitizer a switch costs in proportion to the stack
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

#include "../../valida_amd/csrc/kernels/ntt.hip"
#include "../../valida_amd/csrc/kernels/layout.hip"  // defines vk::g_profiler / vk::g_scope

namespace vk {
uint32_t lds[48 * 1024];  // the workgroup's dynamic LDS (`extern __shared__ uint32_t lds[]` of every kernel resolves to this)
}  // namespace vk

namespace {
using vg::Fp;
constexpr uint32_t UNTOUCHED = 0xDEADBEEFu;  // no field element: above p

struct Tables {
    std::vector<uint32_t> image;
    vk::DeviceTables tb{};
    Tables() : image(vk::device_tables_words()) {
        vk::build_device_tables(tb, image.data());
        vk::bind_device_tables(tb, image.data());
    }
};

int failures = 0;
void fail(const char* what, uint32_t log_n, uint32_t w, uint32_t lb, bool mapped, long at = -1) {
    fprintf(stderr, "lde_colmap_emu: %s (2^%u x %u, blowup 2^%u, %s, at %ld)\n", what, log_n, w, lb, mapped ? "with the map" : "without a map", at);
    failures++;
}

void run_case(const Tables& T, uint32_t log_n, uint32_t w, uint32_t lb, uint32_t shift, const uint32_t* m, const uint32_t* const_mask, const uint32_t* want) {
    const uint64_t n = 1ull << log_n, L = n << lb;
    const int k = (int)log_n;
    std::vector<uint32_t> lt(vk::lde_tables_words(k, (int)lb));
    vk::build_lde_tables(k, (int)lb, Fp::from_canonical(shift), lt.data());
    const size_t n_lo = (size_t)1 << vk::lde_k_lo(k);
    const vk::LdeTables ltv{lt.data(), lt.data() + ((size_t)1 << lb) * n_lo};
    for (int mapped = 0; mapped < 2; mapped++) {
        // ingest: with the flags (zeroed first, as the prover zeroes them) / plain
        std::vector<uint32_t> nat(n * w, UNTOUCHED), varies(w, 0);
        vk::launch_ingest(nullptr, m, vk::DMatView{nat.data(), n, w, n}, false, mapped ? varies.data() : nullptr);
        for (uint64_t r = 0; r < n; r++)
            for (uint32_t j = 0; j < w; j++)
                if (nat[j * n + r] != Fp::from_canonical(m[r * w + j]).v) { fail("ingest: wrong element", log_n, w, lb, mapped, (long)(r * w + j)); return; }
        std::vector<uint32_t> colmap(vk::lde_colmap_words(w), UNTOUCHED);
        uint32_t live_count = w;
        if (mapped) {
            for (uint32_t j = 0; j < w; j++)
                if ((varies[j] != 0) != (const_mask[j] == 0)) fail("flags differ from (m == m[0]).all(0)", log_n, w, lb, true, j);
            for (uint32_t j = 0; j < w; j++)
                if (varies[j] > 1) fail("a flag is neither 0 nor 1", log_n, w, lb, true, j);
            vk::launch_lde_colmap(nullptr, varies.data(), w, colmap.data());
            live_count = colmap[vk::COLMAP_LIVE_COUNT];
            const uint32_t const_count = colmap[vk::COLMAP_CONST_COUNT];
            uint32_t nl = 0, nc = 0;
            for (uint32_t j = 0; j < w; j++) {
                if (const_mask[j]) { if (nc >= const_count || colmap[vk::COLMAP_LIVE + w + nc] != j) fail("map: constant list", log_n, w, lb, true, j); nc++; }
                else { if (nl >= live_count || colmap[vk::COLMAP_LIVE + nl] != j) fail("map: live list", log_n, w, lb, true, j); nl++; }
            }
            if (nl != live_count || nc != const_count) fail("map: counts", log_n, w, lb, true);
            for (uint32_t j = live_count; j < w; j++) if (colmap[vk::COLMAP_LIVE + j] != UNTOUCHED) fail("map: wrote past the live list", log_n, w, lb, true, j);
            for (uint32_t j = const_count; j < w; j++) if (colmap[vk::COLMAP_LIVE + w + j] != UNTOUCHED) fail("map: wrote past the constant list", log_n, w, lb, true, j);
        }
        std::vector<uint32_t> lde(L * w, UNTOUCHED), s1(k > 12 ? n * w : 1, UNTOUCHED), s2(k > 12 ? L * w : 1, UNTOUCHED);
        vk::launch_lde_natural(nullptr, vk::DMatView{nat.data(), n, w, n}, vk::DMatView{lde.data(), L, w, L}, (int)lb, T.tb, ltv, vk::DMatView{s1.data(), n, w, n},
                               vk::DMatView{s2.data(), L, w, L}, mapped ? colmap.data() : nullptr);
        for (uint64_t r = 0; r < L; r++)
            for (uint32_t j = 0; j < w; j++) {
                const uint32_t got = lde[j * L + r];
                if (got == UNTOUCHED || Fp::raw(got).canonical() != want[r * w + j]) { fail("LDE differs from the oracle's", log_n, w, lb, mapped, (long)(r * w + j)); return; }
            }
        if (k > 12) {  // compact scratch: columns [0, live_count) written in full, the rest never
            for (uint32_t j = 0; j < w; j++) {
                const bool used = j < live_count;
                for (uint64_t r = 0; r < n; r++) if ((s1[j * n + r] != UNTOUCHED) != used) { fail("scratch S1 is not compact", log_n, w, lb, mapped, (long)j); return; }
                for (uint64_t r = 0; r < L; r++) if ((s2[j * L + r] != UNTOUCHED) != used) { fail("scratch S2 is not compact", log_n, w, lb, mapped, (long)j); return; }
            }
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: lde_colmap_emu CASES.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> buf;
    uint32_t chunk[4096];
    for (size_t got; (got = fread(chunk, 4, 4096, f)) > 0;) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    if (buf.empty()) { fprintf(stderr, "lde_colmap_emu: empty case file\n"); return 2; }
    const Tables T;
    size_t pos = 1;
    uint32_t done = 0;
    try {
        for (uint32_t c = 0; c < buf[0]; c++) {
            if (pos + 4 > buf.size()) { fprintf(stderr, "lde_colmap_emu: truncated case file\n"); return 2; }
            const uint32_t log_n = buf[pos], w = buf[pos + 1], lb = buf[pos + 2], shift = buf[pos + 3];
            pos += 4;
            const size_t n = (size_t)1 << log_n, need = n * w + w + (n << lb) * w;
            if (log_n > 16 || w == 0 || w > 64 || lb > 3 || pos + need > buf.size()) { fprintf(stderr, "lde_colmap_emu: bad or truncated case %u\n", c); return 2; }
            run_case(T, log_n, w, lb, shift, buf.data() + pos, buf.data() + pos + n * w, buf.data() + pos + n * w + w);
            pos += need;
            done++;
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "lde_colmap_emu: %s\n", e.what());
        return 1;
    }
    for (auto& fb : hipemu::sched().fib) { free(fb.stack); fb.stack = nullptr; }  // the emulator keeps its fiber stacks for the process's lifetime
    printf("lde_colmap_emu: %u cases, each with and without the map, %d failures, %lu barriers\n", done, failures, hipemu::sched().barriers);
    return failures ? 1 : 0;
}
