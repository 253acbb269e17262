// The interpreters of valida_amd/csrc/kernels/quotient.hip — the very source — compiled for the HOST under tools/hipemu: k_quotient<0, 1, 2>,
// k_quotient_general<0, 1, 2> and k_check_constraints<INTERPRET>, launched through the file's own launch_quotient / launch_check_constraints
// (so the choice of kernel, the workgroup size and the dynamic LDS are the product's), on LDEs the oracle made, for AIRs captured into
// air/symbolic.hpp's DAG and lowered by vair::compile (tests/test_air_programs_cpu.py compares the chunk matrix with the oracle's quotient).
// The one- and two-bank register files are ext_vector_type vectors: this harness is compiled by clang++ as a plain host compiler.  The
// thread-per-point kernels of the compiled chips (k_quotient_pt: a DPP exchange) are instantiated but never launched here, and the
// natural-order store's static LDS tile (heights from 2^9 with 256 threads) is per fiber under this build: the tests keep natural order
// below 2^9.  Test infrastructure; nothing in the product links it.
#define HIPEMU_CHECKS 1
#define VGPU_QUOT_PT_WAVES 0  // no occupancy attribute on k_quotient_pt: a host function takes none
#include <hip/hip_runtime.h>  // tools/hipemu/hip/hip_runtime.h (first on the include path)

template <class T> inline T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }  // fibers of one block never interleave inside a call

#include "../../valida_amd/csrc/kernels/launch.hpp"
// which kernel a launcher picked, with what shape: recorded at the launch itself
static const char* emu_last_kernel = "";
static size_t emu_last_lds = 0;
static unsigned emu_last_threads = 0;
#undef VK_LAUNCH
#define VK_LAUNCH(kernel, grid, block, lds, stream, ...)                                \
    do {                                                                                \
        emu_last_kernel = #kernel; emu_last_lds = (size_t)(lds); emu_last_threads = dim3(block).x; \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);              \
    } while (0)

namespace vk {
uint32_t regs[40 * 1024];  // the kernels' dynamic LDS (160 KiB), stale between workgroups as on the device
}  // namespace vk

#include "../../valida_amd/csrc/kernels/quotient.hip"
#include "../../valida_amd/csrc/host/machine.hpp"

namespace vk {
thread_local Profiler* g_profiler = nullptr;
thread_local ProfScope* g_scope = nullptr;
}  // namespace vk

using vg::Fp;
using vg::Ext5;

namespace {
struct EmuAir { vair::Dag dag; };
std::vector<uint32_t> working(const uint32_t* m, uint64_t h, uint64_t w) {  // column-major Montgomery: the prover's working layout
    std::vector<uint32_t> c(h * w);
    for (uint64_t r = 0; r < h; r++)
        for (uint64_t k = 0; k < w; k++) c[k * h + r] = Fp::from_canonical(m[r * w + k]).v;
    return c;
}
Ext5 ext_of(const uint32_t* w) { Ext5 e; for (int k = 0; k < 5; k++) e.c[k] = Fp::from_canonical(w[k]); return e; }
void put_ext(std::vector<uint32_t>& pool, const Ext5& e) { for (int k = 0; k < 5; k++) pool.push_back(e.c[k].v); }
// [K powers of alpha, constraint k scaled by alpha^(K-1-k)][cumulative sum] of an AIR without interactions (K = asserts + 3)
uint32_t consts_of(const vair::Program& p, const Ext5& alpha, const Ext5& cum, std::vector<uint32_t>& pool) {
    const uint32_t K = p.num_asserts + 3;
    std::vector<Ext5> ap(K);
    Ext5 x = Ext5::one();
    for (uint32_t k = 0; k < K; k++) { ap[K - 1 - k] = x; x *= alpha; }
    for (auto& e : ap) put_ext(pool, e);
    put_ext(pool, cum);
    return K;
}
void report(uint32_t* info, char* kernel, uint64_t cap) {
    info[0] = emu_last_threads; info[1] = (uint32_t)emu_last_lds;
    if (kernel && cap) { strncpy(kernel, emu_last_kernel, cap - 1); kernel[cap - 1] = 0; }
}
}  // namespace

extern "C" {
// The capture, straight into the DAG (handles are node ids here; the product's handle table is capi.cpp's and is tested through libvgpu.so)
void* emu_air_new(uint32_t width, uint32_t prep_width) { auto* a = new EmuAir(); a->dag.width = (int)width; a->dag.prep_width = (int)prep_width; return a; }
void emu_air_free(void* a) { delete (EmuAir*)a; }
uint32_t emu_air_constant(void* a, uint32_t c) { return ((EmuAir*)a)->dag.constant(c); }
uint32_t emu_air_variable(void* a, uint32_t is_prep, uint32_t col, uint32_t is_next) { return ((EmuAir*)a)->dag.var(is_prep != 0, (int)col, is_next != 0); }
uint32_t emu_air_is_first_row(void* a) { return ((EmuAir*)a)->dag.selector(vair::N_FIRST); }
uint32_t emu_air_is_last_row(void* a) { return ((EmuAir*)a)->dag.selector(vair::N_LAST); }
uint32_t emu_air_is_transition(void* a) { return ((EmuAir*)a)->dag.selector(vair::N_TRANS); }
uint32_t emu_air_add(void* a, uint32_t x, uint32_t y) { return ((EmuAir*)a)->dag.add(x, y); }
uint32_t emu_air_sub(void* a, uint32_t x, uint32_t y) { return ((EmuAir*)a)->dag.sub(x, y); }
uint32_t emu_air_mul(void* a, uint32_t x, uint32_t y) { return ((EmuAir*)a)->dag.mul(x, y); }
uint32_t emu_air_neg(void* a, uint32_t x) { return ((EmuAir*)a)->dag.neg(x); }
void emu_air_assert_zero(void* a, uint32_t x) { ((EmuAir*)a)->dag.constraints.push_back(x); }

// launch_quotient on the oracle's committed LDEs (row-major canonical, rows bit-reversed, (n << lqd) rows: log_blowup = lqd) of an AIR without
// interactions (perm = the running-sum column alone).  out: n x (5 << lqd) canonical words, row-major.  info: [threads, dynamic LDS bytes,
// registers, instructions].  Returns 0, or -1 with the reason on stderr.
int64_t emu_quotient(void* air, uint32_t log_n, uint32_t lqd, const uint32_t* main_lde, const uint32_t* prep_lde, const uint32_t* perm_lde, const uint32_t* alpha5, const uint32_t* cum5,
                     int natural, uint32_t* out, uint32_t* info, char* kernel, uint64_t kernel_cap) {
    try {
        const vair::Dag& dag = ((EmuAir*)air)->dag;
        const vair::Program prog = vair::compile(dag);
        if (prog.instrs.size() % 4) throw std::runtime_error("the program is not padded to whole quads: the VGPR interpreters fetch four instructions at a time");
        const uint64_t n = 1ull << log_n, L = n << lqd;
        std::vector<uint32_t> m = working(main_lde, L, (uint64_t)dag.width), e = working(perm_lde, L, 5), p;
        if (dag.prep_width) p = working(prep_lde, L, (uint64_t)dag.prep_width);
        std::vector<uint32_t> pool, iw = vk::encode_interactions({}), tbw(vk::device_tables_words());
        vk::DeviceTables tb{};
        vk::build_device_tables(tb, tbw.data());
        vk::bind_device_tables(tb, tbw.data());
        vk::QuotientArgs a{};
        a.K = consts_of(prog, ext_of(alpha5), ext_of(cum5), pool);
        a.main_lde = {m.data(), L, (uint64_t)dag.width, L};
        a.perm_lde = {e.data(), L, 5, L};
        a.prep_lde = dag.prep_width ? vk::DMatView{p.data(), L, (uint64_t)dag.prep_width, L} : vk::DMatView{nullptr, 0, 0, 0};
        a.log_n = (int)log_n;
        a.prog = prog.instrs.data(); a.n_instrs = (uint32_t)prog.instrs.size(); a.n_regs = prog.num_regs; a.n_air_asserts = prog.num_asserts;
        a.native_chip = vk::QuotientArgs::INTERPRET;
        a.iw = iw.data(); a.consts = pool.data();
        const Fp s = Fp::from_canonical(vg::GENERATOR);  // as Prover::fill_quotient_args
        a.coset_shift = s.v; a.coset_shift_inv = s.inv().v;
        a.lqd = (int)lqd;
        const Fp sn = s.exp_power_of_2(log_n), wq = vg::two_adic_generator(lqd);
        Fp wp = Fp::one();
        for (unsigned r = 0; r < (1u << lqd); r++) { Fp z = sn * wp - Fp::one(); a.zh[r] = z.v; a.zh_inv[r] = z.inv().v; wp *= wq; }
        a.g_inv = vg::two_adic_generator(log_n).inv().v;
        const uint64_t cols = 5ull << lqd;
        std::vector<uint32_t> q(n * cols, 0xdeadbeefu);
        a.out = {q.data(), n, cols, n};
        a.out_natural = natural;
        for (auto& w : vk::regs) w = 0xdeadbeefu;  // a register must be written before it is read
        vk::launch_quotient(nullptr, a, tb);
        for (uint64_t r = 0; r < n; r++)
            for (uint64_t c = 0; c < cols; c++) out[r * cols + c] = Fp::raw(q[c * n + r]).canonical();
        report(info, kernel, kernel_cap);
        info[2] = prog.num_regs; info[3] = (uint32_t)prog.instrs.size();
        return 0;
    } catch (const std::exception& ex) {
        fprintf(stderr, "quotient_emu: %s\n", ex.what());
        return -1;
    }
}

// launch_check_constraints on a witness (row-major canonical, n rows) of an AIR without interactions: the first failing (row << 16 | code), -1
// when every constraint holds on every row, -2 on an error.
int64_t emu_check(void* air, uint32_t log_n, const uint32_t* main, const uint32_t* prep, uint32_t* info, char* kernel, uint64_t kernel_cap) {
    try {
        const vair::Dag& dag = ((EmuAir*)air)->dag;
        const vair::Program prog = vair::compile(dag);
        const uint64_t n = 1ull << log_n;
        std::vector<uint32_t> m = working(main, n, (uint64_t)dag.width), e(5 * n, 0), p;
        if (dag.prep_width) p = working(prep, n, (uint64_t)dag.prep_width);
        std::vector<uint32_t> pool, iw = vk::encode_interactions({});
        Ext5 fold;  // the check folds the constraints with powers of a transcript value: any value that is no root of the row's polynomial
        for (int k = 0; k < 5; k++) fold.c[k] = Fp::from_canonical(0x1234567u * (uint32_t)(k + 1) % vg::P);
        vk::QuotientArgs a{};
        a.K = consts_of(prog, fold, Ext5::zero(), pool);
        a.main_lde = {m.data(), n, (uint64_t)dag.width, n};
        a.perm_lde = {e.data(), n, 5, n};
        a.prep_lde = dag.prep_width ? vk::DMatView{p.data(), n, (uint64_t)dag.prep_width, n} : vk::DMatView{nullptr, 0, 0, 0};
        a.log_n = (int)log_n;
        a.prog = prog.instrs.data(); a.n_instrs = (uint32_t)prog.instrs.size(); a.n_regs = prog.num_regs; a.n_air_asserts = prog.num_asserts;
        a.native_chip = vk::QuotientArgs::INTERPRET;
        a.iw = iw.data(); a.consts = pool.data();
        unsigned long long first_bad = ~0ull;
        for (auto& w : vk::regs) w = 0xdeadbeefu;
        vk::launch_check_constraints(nullptr, a, &first_bad);
        report(info, kernel, kernel_cap);
        info[2] = prog.num_regs; info[3] = (uint32_t)prog.instrs.size();
        return first_bad == ~0ull ? -1 : (int64_t)first_bad;
    } catch (const std::exception& ex) {
        fprintf(stderr, "quotient_emu: %s\n", ex.what());
        return -2;
    }
}
}
