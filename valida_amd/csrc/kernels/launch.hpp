// Host-callable launchers of the gfx950 kernels (definitions in the .hip files of this directory).
#pragma once
#include <vector>
#include "device_common.hpp"
#include "profiler.hpp"
#include "../air/symbolic.hpp"
#include "verify_args.hpp"

namespace vk {

struct QuotientArgs {
    DMatView main_lde, perm_lde, prep_lde;  // bit-reversed LDEs (prep_lde.data may be null)
    int log_n;                               // trace height 2^log_n; quotient domain 2^(log_n + 1)
    const vair::Instr* prog;
    uint32_t n_instrs, n_regs, n_air_asserts;
    const uint32_t* iw;          // encoded interactions
    const uint32_t* consts;      // Ext5 words: [K alpha powers][M bus alphas][max_fields betas][cumulative_sum]
    uint32_t K;                  // total number of folded constraints = n_air_asserts + M + 3
    uint32_t coset_shift, coset_shift_inv;      // s = 31 (Montgomery), s^-1
    int lqd;                     // log_quotient_degree: quotient domain 2^(log_n + lqd); 1 for every reference chip
    uint32_t zh_inv[8];          // 1 / zh[r]
    uint32_t zh[8];              // Z_H on the 2^lqd cosets of the quotient domain: zh[r] = s^n w_Q^r - 1 for natural index = r mod 2^lqd
    uint32_t g_inv;              // g_n^{-1}  (subgroup_last)
    DMatView out;                // n x (5 << lqd), row for natural i stored at position bitrev_k(i) — or, out_natural (log_quotient_degree 1 only), at position i
    int out_natural;             // the chunk matrix in NATURAL row order: the following commitment round extends it through the fused LDE (no bit-reversed input path)
    // BasicMachine chip whose eval template is compiled into a native kernel (vchips::ChipId), or INTERPRET for
    // the register-program interpreter (AIRs captured at run time through vgpu_air_*)
    static constexpr int INTERPRET = -2;
    int native_chip;
    // Where the NEXT row of a point is read from: column 0 of main / perm / preprocessed LDEs with the strides of the views above, and the
    // distance of the next row in natural index inside that LDE.  One GPU: the same LDEs, 2^lqd (the launchers fill these in when they
    // are left null / zero).  A proof sharded over several GPUs (host/sharded_prover.cpp) evaluates a row range of the LDE, i.e. the
    // sub-coset s w_L^e H_{L/W}: the successors of its points form ANOTHER sub-coset, a different rank's row range, at the same or the
    // following natural index.
    const uint32_t* main_nx;
    const uint32_t* perm_nx;
    const uint32_t* prep_nx;
    uint32_t next_step_p1;  // 1 + that distance (0 = not set; the distance itself may be 0)
    // defaults of the single-GPU case
    QuotientArgs normalised() const {
        QuotientArgs b = *this;
        if (!b.main_nx) b.main_nx = b.main_lde.data;
        if (!b.perm_nx) b.perm_nx = b.perm_lde.data;
        if (!b.prep_nx) b.prep_nx = b.prep_lde.data;
        if (!b.next_step_p1) b.next_step_p1 = 1u + (1u << (b.lqd > 0 ? b.lqd : 1));
        return b;
    }
};

// The interpreters with an LDS register file (programs of more than 64 registers) keep it slot-major, reg[slot][thread], and shrink the
// workgroup down to INTERP_LDS_MIN_THREADS (one wave) before the file stops fitting: a program may hold as many registers as one wave's
// file fits the dynamic LDS the kernel may have.  k_quotient<0> (log_quotient_degree 1) shares the CU's 160 KiB with its 10 KiB static
// transpose tile of the natural-order store; k_quotient_general<0> and k_check_constraints<INTERPRET> have no static LDS.  These figures are
// the kernels' dynamic-LDS limits (hipFuncSetAttribute), what their launches size by, and what vgpu_machine_push_air refuses above.
constexpr uint32_t INTERP_LDS_MIN_THREADS = 64;
constexpr uint32_t INTERP_LDS_BYTES_PAIR = 148 * 1024, INTERP_LDS_BYTES_GENERAL = 160 * 1024;
constexpr uint32_t INTERP_LDS_MAX_REGS_PAIR = INTERP_LDS_BYTES_PAIR / (4 * INTERP_LDS_MIN_THREADS);        // 592: k_quotient<0>
constexpr uint32_t INTERP_LDS_MAX_REGS_GENERAL = INTERP_LDS_BYTES_GENERAL / (4 * INTERP_LDS_MIN_THREADS);  // 640: k_quotient_general<0>
// the largest register file every kernel that runs an AIR of this log_quotient_degree holds
constexpr uint32_t interp_lds_max_regs(unsigned lqd) { return lqd == 1 ? INTERP_LDS_MAX_REGS_PAIR : INTERP_LDS_MAX_REGS_GENERAL; }
// threads per workgroup of an LDS-file interpreter launch: 256 while the file fits 64 KiB, halved down to one wave
inline unsigned interp_lds_threads(uint32_t n_regs) {
    unsigned threads = 256;
    while (threads > INTERP_LDS_MIN_THREADS && (size_t)n_regs * threads * 4 > 64 * 1024) threads >>= 1;
    return threads;
}

// layout.hip
// varies (optional, dst.width words, ZEROED on `st` before this launch): varies[j] = 1 afterwards iff some row of column j differs from row 0
// — every row is compared, as field elements; the constant-column detection of the fused LDE (launch_lde_colmap).  Widths up to ingest_flags_max_width.
void launch_ingest(hipStream_t st, const uint32_t* src_dev, DMatView dst, bool bitrev, uint32_t* varies = nullptr);
constexpr uint64_t INGEST_FLAGS_MAX_WIDTH = 512;  // one more LDS row (the Montgomery forms of row 0) beside the 64-row tile
void launch_bitrev_rows(hipStream_t st, DMatView src, DMatView dst);
void launch_clock_probe(hipStream_t st, uint64_t* out3, uint32_t iters);  // out3: page-locked host memory (device-visible); see vgpu_shader_clock_probe
// n_cols columns of Wq = 2^log_wq blocks of `rows` rows (block r in the natural order of the sub-coset bitrev(r)) -> columns in global natural order
void launch_interleave_blocks(hipStream_t st, const uint32_t* src, uint32_t* dst, uint64_t rows, uint32_t log_wq, uint64_t n_cols);
void launch_export_rows(hipStream_t st, DMatView src, uint64_t row0, uint64_t nrows, uint32_t* dst_dev);
// field_probe.hip (test hook): primitive `op` of field.hpp / butterfly.hpp / poseidon_perm.hpp on n operand tuples of raw stored words, word k of item i
// at in[k * n + i] / out[k * n + i].  The butterfly ops read twiddles at tw[(1 << (lowbits + st)) - 1 + low + (k << lowbits)], st < 4, k < 8: the
// CALLER keeps low < 2^lowbits and lowbits <= 10 (the compact tables cover stages 1..14), and low = lowbits = 0 in the LB0 forms — the launcher
// sees device memory only and checks nothing; field_probe_check_twiddle_range does it on the HOST copy of the operands before they are uploaded
// (vgpu_field_probe and the emulation harness both call it) and throws std::invalid_argument.
enum FieldProbeOp {
    FP_REDUCE_ONCE = 0, FP_SUB_MOD, FP_ADD, FP_SUB, FP_NEG, FP_MUL, FP_MONTY_REDUCE, FP_MONTY_REDUCE_WIDE, FP_FROM_CANONICAL, FP_CANONICAL, FP_INV,
    FP_EXT_MUL, FP_EXT_SQUARE, FP_EXT_SCALE, FP_EXT_INV, FP_BFLY_DIT_LB0, FP_BFLY_DIT, FP_BFLY_DIF_LB0, FP_BFLY_DIF, FP_MONTY_SIGNED, FP_SBOX, FP_SBOX_PLUS,
    FP_PERMUTE, FP_PERMUTE_PLAIN, FIELD_PROBE_OPS
};
bool field_probe_shape(uint32_t op, int* in_words, int* out_words);  // words per item; false: unknown op
void field_probe_check_twiddle_range(uint32_t op, const uint32_t* in_host, uint64_t n);
void launch_field_probe(hipStream_t st, uint32_t op, const uint32_t* in_dev, uint64_t n, const DeviceTables& tb, const uint32_t* pos_dev, bool sparse, uint32_t* out_dev);
// lazy_probe.hip (test hook): fold_hi, the Ext5 product and the lazily folded sums of field.hpp (LazyAcc / ExtAcc) on n operand tuples of raw stored
// words, laid out as the field probe's.  `terms` = the length of a sum (0 for the two ops that have none); shapes and lengths: lazy_probe_shape.
enum LazyProbeOp { LP_FOLD_HI = 0, LP_EXT_MUL, LP_LIN_DOT, LP_EXT_DOT, LP_LIN_DOT_LOOP, LAZY_PROBE_OPS };
bool lazy_probe_shape(uint32_t op, uint32_t terms, int* in_words, int* out_words);  // words per item; false: unknown op or a length the op is not built for
void launch_lazy_probe(hipStream_t st, uint32_t op, uint32_t terms, const uint32_t* in_dev, uint64_t n, uint32_t* out_dev);
// ntt.hip
void launch_intt(hipStream_t st, DMatView m, const DeviceTables& tb);
void launch_coset_ntt(hipStream_t st, DMatView coeffs, DMatView dst, uint64_t dst_row0, Fp shift, const DeviceTables& tb);
// natural-order evaluations -> committed (bit-reversed) LDE in 3 fused passes (1 for heights <= 2^12); lt: build_lde_tables(k, log_blowup, shift)
// colmap (optional; heights above 2^12 only, ignored below): the column map launch_lde_colmap wrote on `st` — the passes transform its live columns
// only (the scratch matrices used compactly) and k_lde_fill_const fills every constant column of `lde` with the column's row 0.  nullptr = every column.
void launch_lde_natural(hipStream_t st, DMatView nat, DMatView lde, int log_blowup, const DeviceTables& tb, const LdeTables& lt, DMatView s1, DMatView s2,
                        const uint32_t* colmap = nullptr);
// The column map of a `width`-column matrix, 2 + 2 width words: [live_count, const_count, live[0 .. width) ascending, const[0 .. width) ascending]
// (only the first live_count / const_count entries of each list are written).  One workgroup, from the flags launch_ingest left in `varies`.
constexpr uint32_t COLMAP_LIVE_COUNT = 0, COLMAP_CONST_COUNT = 1, COLMAP_LIVE = 2;  // const[] starts at COLMAP_LIVE + width
inline size_t lde_colmap_words(uint64_t width) { return 2 + 2 * (size_t)width; }
void launch_lde_colmap(hipStream_t st, const uint32_t* varies, uint64_t width, uint32_t* colmap);
// verify.hip: the per-query checks of a chunk of Machine::verify plans (k_verify_open, k_verify_fold, k_verify_tree in that order on `st`)
void launch_verify_chunk(hipStream_t st, const VerifyChunkArgs& a);
// merkle.hip
void launch_keccak_leaves(hipStream_t st, const uint32_t* const* cols_dev, int n_elems, uint64_t n_rows, uint32_t* digests);
void launch_keccak_leaves_strided(hipStream_t st, const uint32_t* base, uint64_t stride, int n_elems, uint64_t n_rows, uint32_t* digests);
void launch_keccak_compress(hipStream_t st, const uint32_t* prev, const uint32_t* const* cols_dev, int n_elems, uint64_t n_out, uint32_t* next);
// The sibling digests of the two BOTTOM layers of a tree that did not keep them (DeviceTree::drop_bottom), recomputed at query time from the committed rows.
// jobs: 8 words each (merkle.hip, k_keccak_bottom_q); indices_dev: the sampled query indices; dst: the proof tail being gathered.
void launch_keccak_bottom_q(hipStream_t st, const uint32_t* jobs_dev, uint32_t n_jobs, const uint32_t* indices_dev, uint32_t* dst);
void launch_poseidon_bottom_q(hipStream_t st, const uint32_t* pos_dev, bool sparse, const uint32_t* jobs_dev, uint32_t n_jobs, const uint32_t* indices_dev, uint32_t* dst);
constexpr int KECCAK_TOP_MAX_LEVELS = 11;  // first_len <= 1024
struct KeccakTopArgs {
    const uint32_t* prev;  // layer with 2 * first_len digests
    uint64_t first_len;    // parents in the first computed layer (power of two <= 1024)
    int levels;            // layers computed: first_len, first_len/2, ..., 1
    uint32_t* out[KECCAK_TOP_MAX_LEVELS];
    const uint32_t* const* cols[KECCAK_TOP_MAX_LEVELS];  // injected matrices' columns per layer (or null)
    int n_elems[KECCAK_TOP_MAX_LEVELS];
    // Optional epilogue (FRI commit phase): the workgroup's first wave runs the DuplexChallenger step on the root it has just written —
    // observe it, sample beta — instead of a k_fri_challenge launch of its own behind the tree (challenger_dev.hpp; arguments as
    // launch_fri_challenge's).  ch_pos == nullptr: none.
    // Optional prologue (trees over ONE strided matrix of <= 512 rows, i.e. the small FRI layers): the launch hashes the leaves itself
    // into `prev` (leaf_rows rows of leaf_elems elements, columns leaf_base + k * leaf_stride) instead of a leaf launch of its own before it.
    const uint32_t* leaf_base = nullptr;
    uint64_t leaf_stride = 0;
    int leaf_elems = 0;
    uint64_t leaf_rows = 0;  // 0: none; else 2 * first_len
    // launch_keccak_levels only: parents of the first layer per WORKGROUP (a power of two <= 256 dividing first_len; the grid is
    // first_len / block_len workgroups, each walks its own sub-tree `levels` <= log2(block_len) + 1 layers down).  0: first_len (one workgroup)
    uint64_t block_len = 0;
    const uint32_t* ch_pos = nullptr;
    uint32_t* ch_state = nullptr;
    uint32_t* ch_beta5 = nullptr;
    uint32_t* ch_commit8 = nullptr;
};
void launch_keccak_top(hipStream_t st, const KeccakTopArgs& a);
// Several consecutive layers of the latency-bound middle of a tree (256 < parents <= 32768) in ONE launch: a workgroup per 64 parents of the
// first layer, the digests handed from layer to layer through LDS (merkle.hip: k_keccak_levels_pair).  keccak_levels_fused(len): whether a
// layer of `len` parents may go into such a launch (lane-pair kernels on, VGPU_KECCAK_LEVELS != 0); keccak_levels_take_leaves(n_rows):
// whether the launch can also hash the leaves of a single strided matrix of n_rows rows itself (KeccakTopArgs::leaf_*).
constexpr uint64_t KECCAK_LEVELS_BLOCK_LEN = 64;
void launch_keccak_levels(hipStream_t st, const KeccakTopArgs& a);
bool keccak_levels_fused(uint64_t len);
bool keccak_levels_take_leaves(uint64_t n_rows);
bool keccak_top_takes_leaves(uint64_t n_rows);  // whether launch_keccak_top can hash the leaves of a tree of n_rows rows itself (KeccakTopArgs::leaf_*)
// poseidon_mmcs.hip — the same tree with PaddingFreeSponge / TruncatedPermutation over Poseidon-16 (hash kind 1).
// pos_dev: [480 round constants][16 circulant MDS coefficients], Montgomery (the table the device challenger uses)
void launch_poseidon_leaves(hipStream_t st, const uint32_t* pos_dev, bool sparse, const uint32_t* const* cols_dev, int n_elems, uint64_t n_rows, uint32_t* digests);
void launch_poseidon_leaves_strided(hipStream_t st, const uint32_t* pos_dev, bool sparse, const uint32_t* base, uint64_t stride, int n_elems, uint64_t n_rows, uint32_t* digests);
void launch_poseidon_compress(hipStream_t st, const uint32_t* pos_dev, bool sparse, const uint32_t* prev, const uint32_t* const* cols_dev, int n_elems, uint64_t n_out, uint32_t* next);
// the layers of at most 16384 parents: launches of 16-row workgroups, each walking its sub-tree up to five layers down (one permutation per 16-lane row);
// layers group by log2(parents) / 5, the group that ends at the root is one workgroup and may carry the FRI challenger step (a.ch_*)
bool poseidon_levels_take(uint64_t parents);
int poseidon_levels_group(uint64_t parents);
void launch_poseidon_levels(hipStream_t st, const uint32_t* pos_dev, bool sparse, const KeccakTopArgs& a);
void launch_poseidon_top(hipStream_t st, const uint32_t* pos_dev, bool sparse, const KeccakTopArgs& a);  // first_len <= 16: the last group alone (sharded commitments)
// perm.hip
uint64_t perm_scratch_words(uint64_t n);
void launch_add_ext_const(hipStream_t st, uint32_t* data, uint64_t stride, uint64_t n, const uint32_t* off5_dev);  // 5 columns += 5 Montgomery constants
// native_chip: vchips::ChipId when the AIR is one of the in-tree BasicMachine chips (its interactions are compiled into the kernel), anything else = the encoded walk
void launch_perm_trace(hipStream_t st, DMatView main, DMatView prep, const uint32_t* iw_dev, const uint32_t* chal_dev, uint32_t M, DMatView perm,
                       uint32_t* scratch, int native_chip = -2);
// quotient.hip
void launch_quotient(hipStream_t st, const QuotientArgs& a, const DeviceTables& tb);
// Debug check on the trace domain: `a` carries the NATURAL-order traces in main_lde / perm_lde / prep_lde (log_n = log height);
// *first_bad_dev (initialised to ~0) receives min over failures of (row << 16 | code), see quotient.hip.
void launch_check_constraints(hipStream_t st, const QuotientArgs& a, unsigned long long* first_bad_dev);
// tracegen.hip — device images of the VM's operation logs (C ABI twins: vgpu_cpu_op_t, vgpu_mem_op_t, vgpu_alu_op_t)
struct TgCpuOp { uint32_t pc, fp, opcode; int32_t operands[5]; uint32_t kind, has_imm, imm, mem_first; };
struct TgMemOp { uint32_t clk, addr, value, is_write; };
struct TgAluOp { uint32_t opcode, a, b, c; };  // a = result, b / c = inputs, as u32 values of the big-endian Words
struct TgOutOp { uint32_t clk, byte; };          // OutputChip::values entry
enum { TG_CPU_STORE32 = 0, TG_CPU_LOAD32, TG_CPU_JAL, TG_CPU_JALV, TG_CPU_BEQ, TG_CPU_BNE, TG_CPU_IMM32, TG_CPU_BUS, TG_CPU_BUS_LEFT_IMM, TG_CPU_STOP,
       TG_CPU_LOADFP, TG_CPU_LOAD_U8, TG_CPU_LOAD_S8, TG_CPU_STORE_U8, TG_CPU_READ_ADVICE };
void launch_tracegen_cpu(hipStream_t st, const TgCpuOp* ops, uint64_t n, const TgMemOp* mem, uint64_t n_mem, DMatView t);
size_t tracegen_mem_sort_scratch_bytes(uint64_t n);
hipError_t launch_tracegen_mem(hipStream_t st, const TgMemOp* mem, uint64_t n, const uint32_t* static_cells, uint64_t n_static, uint32_t* keys2, uint32_t* idx2,
                               void* sort_tmp, size_t sort_tmp_bytes, DMatView t);
void launch_tracegen_alu(hipStream_t st, int chip, const TgAluOp* ops, uint64_t n, DMatView t);
void launch_tracegen_idle(hipStream_t st, int mode, const uint32_t* static_cells, uint64_t n_static, DMatView t);  // 0 zeros, 1 mul counter, 2 static data
// range: the byte histogram of the words range_check()'ed on execute — the results of add, sub, mul, mulhs, mulhu, div, sdiv instructions
// (alu_u32/src/{add,sub,mul,div}/mod.rs), read from the cpu log's bus operations and the memory write of their cycle
hipError_t launch_tracegen_range(hipStream_t st, const TgCpuOp* ops, uint64_t n, const TgMemOp* mem, uint64_t n_mem, uint32_t* counts, DMatView t);
// mul / div / shift / com from their logs (chip = CHIP_MUL .. ); output from the tape and the host-computed first row of every window
void launch_tracegen_alu2(hipStream_t st, int chip, const TgAluOp* ops, uint64_t n, DMatView t);
void launch_tracegen_output(hipStream_t st, const TgOutOp* vals, const uint32_t* row0, uint64_t n, uint64_t n_rows, DMatView t);
hipError_t launch_tracegen_program(hipStream_t st, const TgCpuOp* ops, uint64_t n, uint64_t padded_n, uint32_t rom_len, uint32_t* counts, DMatView t);
// bus_audit.hip — the passes of the bus audit (host/bus_audit.hpp: contract, descriptor layout `desc`; Prover::bus_audit drives them).
// n = record slots = sum over chips of height x interactions.  keys2 / ids2: [2 n] ping-pong halves; cnt, gid, head_pos: [n]; sums, nrec: [2 n];
// counters: [8 + buses] words; sort / scan scratch: the word counts below.
size_t bus_audit_sort_scratch_words(uint64_t n);
size_t bus_audit_scan_scratch_words(uint64_t n);
void launch_ba_records(hipStream_t st, const uint32_t* desc, uint32_t chip, uint64_t height, uint32_t width, uint32_t M, uint32_t hash_bits, unsigned long long* keys, uint32_t* ids,
                       uint32_t* cnt, uint32_t* live_out);
void launch_ba_iota(hipStream_t st, uint32_t* ids, uint64_t n);
void launch_ba_rekey(hipStream_t st, const uint32_t* desc, uint32_t chunk, const uint32_t* ids, const uint32_t* cnt, unsigned long long* keys, uint64_t n);
int launch_ba_sort(hipStream_t st, unsigned long long* keys2, uint32_t* vals2, uint64_t n, uint32_t* counts, const int* shifts, int n_shifts, int half);
void launch_ba_groups(hipStream_t st, const uint32_t* desc, const unsigned long long* keys, const uint32_t* ids, uint64_t n, bool exact, uint32_t* gid, uint32_t* head_pos,
                      uint32_t* scan_tmp, uint32_t* counters);
void launch_ba_reduce(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* cnt, const uint32_t* gid, const uint32_t* head_pos, uint64_t n, bool check,
                      unsigned long long* sums, uint32_t* nrec, uint32_t* counters);
void launch_ba_select(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* head_pos, const unsigned long long* sums, uint64_t n_groups_max, bool collect,
                      uint32_t cap, unsigned long long* ukeys, uint32_t* uvals, uint32_t* counters);
void launch_ba_report(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* cnt, const uint32_t* head_pos, const unsigned long long* sums, const uint32_t* nrec,
                      const uint32_t* uvals, uint32_t n_rep, uint32_t R, uint32_t* out);
// constraint_audit.hip — the passes of the constraint audit (host/constraint_audit.hpp: contract; Prover::constraint_audit drives them), per chip.
// totals: [K + 1] u64 (zeroed), table / prefix: [K][NB] u32 (table zeroed), rows / values: [K][R] u32.
constexpr uint32_t CA_MAX_CONSTRAINTS = 96, CA_MASK_WORDS = 3;  // the fail mask of a row: bitwise has 88 constraints, lt 60, cpu 53
constexpr int CA_INTERPRET = -2;                                 // QuotientArgs::INTERPRET
struct CaListed { uint32_t w[CA_MASK_WORDS]; };                   // bit k: constraint k of the chip is listed in the report
struct CaArgs {
    const uint32_t* main;  // column-major working layout (Montgomery), natural row order
    uint64_t mstride;
    const uint32_t* prep;  // null for a chip without preprocessed columns
    uint64_t pstride;
    uint64_t n;            // height, a power of two
    uint32_t width, prep_width;
    const vair::Instr* prog;
    uint32_t n_instrs, n_regs, K;  // K = constraints of the chip, 1..CA_MAX_CONSTRAINTS
    int native_chip;               // a vchips::ChipId with constraints, or CA_INTERPRET
    uint32_t T, NB;                // rows per workgroup (ca_block_threads) and workgroups = ceil(n / T)
};
uint32_t ca_block_threads(const CaArgs& a);
void launch_ca_count(hipStream_t st, const CaArgs& a, unsigned long long* totals, uint32_t* table);
void launch_ca_scan(hipStream_t st, const CaArgs& a, const uint32_t* table, uint32_t* prefix, const CaListed& listed);
void launch_ca_list(hipStream_t st, const CaArgs& a, const uint32_t* table, const uint32_t* prefix, const CaListed& listed, uint32_t R, uint32_t* rows);
void launch_ca_values(hipStream_t st, const CaArgs& a, const unsigned long long* totals, const CaListed& listed, uint32_t R, const uint32_t* rows, uint32_t* values);
// mutation_audit.hip — the passes of the mutation audit (host/mutation_audit.hpp: contract; Prover::mutation_audit drives them), per chip.
// An ENTRY of a chip is e = column * D + delta index, E = width * D of them.  totals: [E][3] u64 {free, air, bus} (zeroed), table / prefix:
// [E][NB] u32 free rows per workgroup and their exclusive prefix (table zeroed), rows: [E][R] u32.
constexpr int MA_BUS_ONLY = -1;  // a chip without constraints: only its interactions are walked
constexpr uint32_t MA_COUNT = 0, MA_LIST = 1;
struct MaArgs {
    const uint32_t* main;  // column-major working layout (Montgomery), natural row order
    uint64_t mstride;
    const uint32_t* prep;  // null for a chip without preprocessed columns
    uint64_t pstride;
    uint64_t n;            // height, a power of two
    uint32_t width, prep_width;
    const vair::Instr* prog;
    uint32_t n_instrs, n_regs, K;  // K = constraints of the chip, 0..CA_MAX_CONSTRAINTS
    const uint32_t* iw;            // the chip's interactions (interactions.hpp: encode_interactions)
    const uint32_t* flags;         // [width] MA_COL_* of host/mutation_audit.hpp: bit 0 read as local, bit 1 as next, bit 2 by an interaction;
                                   // then [width][2] the bus masks of the column (ma_bus_masks): interactions whose count / some field changes
    uint32_t bus_walk;             // 1: more than 32 interactions, no masks: every interaction is evaluated per mutation
    uint32_t CY;                   // column slices = gridDim.y (ma_column_slices)
    uint32_t D, delta[4];          // the deltas, Montgomery
    int native_chip;               // a vchips::ChipId with constraints, CA_INTERPRET, or MA_BUS_ONLY
    uint32_t T, NB;                // rows per workgroup (ma_block_threads) and workgroups = ceil(n / T)
    double evaluations;            // Air::eval row evaluations of the counting pass (ma_evaluations): the profile's `ops` column of k_ma_count.*
};
uint32_t ma_block_threads(const MaArgs& a);
uint32_t ma_column_slices(const MaArgs& a, uint32_t NB);
void launch_ma_count(hipStream_t st, const MaArgs& a, unsigned long long* totals, uint32_t* table);
// entries below e_cut with a free row are listed
void launch_ma_scan(hipStream_t st, const MaArgs& a, const unsigned long long* totals, const uint32_t* table, uint32_t* prefix, uint32_t e_cut);
void launch_ma_list(hipStream_t st, const MaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows);
// pair_audit.hip — the passes of the pair audit (host/pair_audit.hpp: contract; Prover::pair_audit drives them), per chip.  The launch shape and
// the single mutations are the mutation audit's (MaArgs; m.CY = pair slices = gridDim.y).  An ENTRY of a chip is e = p * D * D + q for coupled
// pair p (ascending (c1, c2)) and delta pair q = i * D + j; E = P * D * D.  totals: [E][2] u64 {free, compensated}, then [16] u64 per q the sum
// over ALL pairs c1 < c2 of the rows where both single mutations are free, then [16] u64 the same sum over the coupled pairs (their difference
// is the uncoupled pairs' exact `free`) (all zeroed); table / prefix: [E][NB] u32 compensated rows per workgroup and their exclusive prefix
// (table zeroed); rows: [E][R] u32.
constexpr uint32_t PA_SLICE_ENTRIES = 1024;  // entries a workgroup accumulates in LDS: 8 KB of counters, 36 KB of row bits at 256 rows
struct PaArgs {
    MaArgs m;
    const uint32_t* pairs;   // [P] c1 | c2 << 16 (pa_coupled_pairs)
    const uint32_t* pmasks;  // [E][2] the bus masks of the entry (pa_bus_masks): interactions whose count / some field changes
    uint32_t P, PPS;         // coupled pairs; pairs per slice (pa_shape): slice y walks pairs [y PPS, y PPS + PPS)
};
inline uint64_t pa_totals_words(const PaArgs& v) { return 2 * (2ull * v.P * v.m.D * v.m.D + 32); }  // u32 words of the u64 totals
// Rows per workgroup, workgroups, pairs per slice and slices of a chip's launch; throws std::invalid_argument when no tile of the chip fits the LDS
void pa_shape(PaArgs& v);
void launch_pa_count(hipStream_t st, const PaArgs& v, unsigned long long* totals, uint32_t* table);
// entries below e_cut with a compensated row are listed
void launch_pa_scan(hipStream_t st, const PaArgs& v, const unsigned long long* totals, const uint32_t* table, uint32_t* prefix, uint32_t e_cut);
void launch_pa_list(hipStream_t st, const PaArgs& v, const uint32_t* table, const uint32_t* prefix, uint32_t e_cut, uint32_t R, uint32_t* rows);
// rank_audit.hip — the passes of the rank audit (host/rank_audit.hpp: contract; Prover::rank_audit drives them), per chip.  One wave per trace
// row, NW waves per workgroup, each wave RPW rows: T = NW * RPW rows per workgroup, NB workgroups.  totals: u64 [0] sum of nullities, [1] sum of
// zero columns, [2] coupled rows, [3] max nullity, then per column [4 + 2 c] loose rows, [5 + 2 c] zero rows (all zeroed); table / prefix:
// [width][NB] u32 coupled rows of the column per workgroup and their exclusive prefix (table zeroed); rows: [width][R][18] u32 (zeroed).
struct RaArgs {
    const uint32_t* main;  // column-major working layout (Montgomery), natural row order
    uint64_t mstride;
    const uint32_t* prep;  // null for a chip without preprocessed columns
    uint64_t pstride;
    uint64_t n;            // height, a power of two
    uint32_t width, prep_width;
    const vair::Instr* prog;
    uint32_t n_instrs, n_regs, K;  // K = constraints of the chip
    const uint32_t* iw;            // the chip's interactions (interactions.hpp: encode_interactions): the counts, for liveness
    const uint32_t* wr;            // the interaction rows of the Jacobian (host/rank_audit.hpp: ra_weight_rows)
    int native_chip;               // a vchips::ChipId with constraints, CA_INTERPRET, or MA_BUS_ONLY
    uint32_t NW, RPW, T, NB;       // ra_shape
    double evaluations;            // dual row evaluations of the counting pass at most (full rank ends a row early): the profile's `ops`
};
inline uint64_t ra_totals_words(const RaArgs& a) { return 2 * (4ull + 2ull * a.width); }  // u32 words of the u64 totals
// Waves per workgroup, rows per wave and workgroups of a chip's launch; throws std::invalid_argument when the chip does not fit the LDS with one wave
void ra_shape(RaArgs& a);
size_t ra_lds_bytes(const RaArgs& a, uint32_t NW, uint32_t T);
void launch_ra_count(hipStream_t st, const RaArgs& a, unsigned long long* totals, uint32_t* table);
// columns below c_cut with a coupled row are listed
void launch_ra_scan(hipStream_t st, const RaArgs& a, const uint32_t* table, uint32_t* prefix, uint32_t c_cut);
void launch_ra_list(hipStream_t st, const RaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows);
// step_audit.hip — the passes of the step audit (host/step_audit.hpp: contract; Prover::step_audit drives them), per chip: the rank audit's launch
// shape and inputs plus the steps (Montgomery).  totals: u64 [0] confirmed rows, [1] refuted rows, [2 + s] passes of step s, then per column
// [6 + 4 c] loose, zero, exact, coupled-and-exact rows (all zeroed); table / prefix: [width][NB] u32 listable rows of the column per workgroup and
// their exclusive prefix (table zeroed; the scan is launch_ra_scan); rows: [width][R][20] u32 (zeroed).
struct SaArgs {
    RaArgs r;  // evaluations: dual plus plain row evaluations at most
    uint32_t n_steps, steps[4];
};
inline uint64_t sa_totals_words(const SaArgs& a) { return 2 * (6ull + 4ull * a.r.width); }  // u32 words of the u64 totals
void sa_shape(SaArgs& a);  // ra_shape for this audit's LDS; throws std::invalid_argument when the chip does not fit
size_t sa_lds_bytes(const SaArgs& a, uint32_t NW, uint32_t T);
void launch_sa_count(hipStream_t st, const SaArgs& a, unsigned long long* totals, uint32_t* table);
void launch_sa_list(hipStream_t st, const SaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R, uint32_t* rows);
// invariant_audit.hip — the passes of the invariant audit (host/invariant_audit.hpp: contract; Prover::invariant_audit drives them), per chip.
// Phase 1: NB1 workgroups of one wave eliminate RB consecutive augmented rows (1, M[r][0..w)) each into a reduced basis; part: per workgroup
// w + 1 pivot flags and [w + 1][w + 1] basis rows (row p: the row of pivot column p; rows of other columns are not written).  The merge (a tree
// of fan IA_MERGE_FAN, one wave per node) eliminates them into one basis; inv: [0] rho_A, [1] d, [2 + c] pivot flag of augmented column c, then d vectors of w + 1 Montgomery
// words, the i-th non-pivot column's canonical invariant.  Phase 2: the rank audit's launch shape and inputs plus the d invariants;
// totals: u64 [i] free rows of invariant i (zeroed); table / prefix: [d][NB] u32 free rows per workgroup and their exclusive prefix (table
// zeroed; the scan is launch_ra_scan); rows: [d][R] u32.
struct IaArgs {
    RaArgs r;             // evaluations: the rank audit's dual row evaluations at most
    uint32_t d;           // invariants of the chip (known after the merge)
    const uint32_t* vec;  // inv + 2 + (w + 1): the merge's vectors, row stride w + 1
    uint32_t RB, NB1;     // ia_basis_shape
};
constexpr uint32_t IA_MAX_WIDTH = 191, IA_MAX_WORKGROUPS = 2048, IA_TILE_ROWS = 32, IA_MERGE_FAN = 16;
// the workgroups' slots and, behind them, the spare slots of the merge tree's second level (the levels ping-pong)
inline uint64_t ia_part_words(const IaArgs& a) { return ((uint64_t)a.NB1 + (a.NB1 + IA_MERGE_FAN - 1) / IA_MERGE_FAN) * (a.r.width + 1ull) * (a.r.width + 2ull); }
inline uint64_t ia_inv_words(const IaArgs& a) { return 2ull + (a.r.width + 1ull) * (a.r.width + 1ull); }
inline uint64_t ia_totals_words(const IaArgs& a) { return 2ull * a.d; }  // u32 words of the u64 totals
size_t ia_basis_lds_bytes(uint32_t width);
void ia_basis_shape(IaArgs& a);  // RB and NB1 from the height; throws std::invalid_argument when the chip's basis does not fit the LDS
void launch_ia_basis(hipStream_t st, const IaArgs& a, uint32_t* part);
void launch_ia_merge(hipStream_t st, const IaArgs& a, uint32_t* part, uint32_t* inv);  // part is overwritten by the levels of the tree
void ia_shape(IaArgs& a);  // ra_shape for this audit's LDS with a.d invariants; throws std::invalid_argument when the chip does not fit
size_t ia_lds_bytes(const IaArgs& a, uint32_t NW, uint32_t T);
void launch_ia_count(hipStream_t st, const IaArgs& a, unsigned long long* totals, uint32_t* table);
void launch_ia_list(hipStream_t st, const IaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows);
// transition_audit.hip — the passes of the transition audit (host/transition_audit.hpp: contract; Prover::transition_audit drives them), per chip.
// A WINDOW r = 0 .. n - 2 is the row (1, M[r][0..w), M[r + 1][0..w)) of AW = 2 w + 1 window columns.  Flags: per window column j >= 1 the OR of
// TA_OUTSIDE / TA_ANY0 / TA_ANY1 over the windows, flags [AW] u32 and ones [AW] u64 the windows on which the column is 1 (both zeroed).  Phase 1:
// grid (NB1, G): workgroup (x, g), one wave, eliminates the windows [x RB, x RB + RB) on which gate g holds into a reduced basis; part: per gate
// NB1 + ceil(NB1 / 16) slots of AW pivot flags and [AW][AW] basis rows (the invariant audit's slot with w + 1 replaced by AW); the merge (a tree of
// fan IA_MERGE_FAN, gates over gridDim.y) leaves per gate at inv + g ta_inv_words: [0] rho, [1] d, [2 + c] pivot flag of window column c, then d
// vectors of AW Montgomery words.  Phase 2: the rank audit's launch shape and inputs plus the E listed entries: evec [E][2 w] (the `local` part of
// the vector, then the `next` part), egate [E][4] (gate column, gate value as a Montgomery word, bit 0 / 1: the local / next part is non-zero, 0);
// bits [n][2][EW] u32, EW = ceil(E / 32): bit e of [r][0]: window r exists, the entry's gate holds on it and the local part is outside the row
// space of J_r; of [r][1]: the same for window r - 1 and the next part.  Count / list: grid (NB2, ceil(E / 256)), thread <-> entry, WPB windows per
// workgroup: free at window r = [r][0] | [r + 1][1]; totals [E] u64 (zeroed), table / prefix [E][NB2] u32, rows [E][R] u32.
struct TaArgs {
    RaArgs r;               // evaluations: the rank audit's dual row evaluations at most
    uint32_t RB, NB1;       // ta_basis_shape: windows per phase-1 slice, slices
    uint32_t G;             // audited gates of the chip
    const uint32_t* gates;  // [G][2] window column (0: every window), value as a Montgomery word
    uint32_t E, EC;         // listed entries; entries staged in LDS at a time (ta_shape)
    const uint32_t* evec;
    const uint32_t* egate;
    uint32_t WPB, NB2;      // ta_shape: windows per workgroup of the count and list passes, workgroups
};
constexpr uint32_t TA_MAX_WINDOW = 184, TA_TILE_WINDOWS = 32, TA_BOOL_ROWS = 4096;
inline uint64_t ta_slot_words(const TaArgs& a) { return (2ull * a.r.width + 1) * (2ull * a.r.width + 2); }
inline uint64_t ta_gate_slots(const TaArgs& a) { return (uint64_t)a.NB1 + (a.NB1 + IA_MERGE_FAN - 1) / IA_MERGE_FAN; }
inline uint64_t ta_part_words(const TaArgs& a) { return (uint64_t)a.G * ta_gate_slots(a) * ta_slot_words(a); }
inline uint64_t ta_inv_words(const TaArgs& a) { return 2ull + (2ull * a.r.width + 1) * (2ull * a.r.width + 1); }
inline uint64_t ta_bits_words(const TaArgs& a) { return a.r.n * 2ull * ((a.E + 31u) / 32u); }
size_t ta_basis_lds_bytes(uint32_t width);
void ta_basis_shape(TaArgs& a, uint32_t gates);  // RB and NB1 for at most `gates` gates; throws std::invalid_argument when 2 w + 1 > TA_MAX_WINDOW
void launch_ta_flags(hipStream_t st, const TaArgs& a, uint32_t* flags, unsigned long long* ones);
void launch_ta_basis(hipStream_t st, const TaArgs& a, uint32_t* part);
void launch_ta_merge(hipStream_t st, const TaArgs& a, uint32_t* part, uint32_t* inv);  // part is overwritten by the levels of the tree
void ta_shape(TaArgs& a);  // ra_shape for this audit's LDS with a.E entries (0: the fit with one entry staged is checked); throws std::invalid_argument when the chip does not fit
size_t ta_lds_bytes(const TaArgs& a, uint32_t NW, uint32_t T, uint32_t EC);
void launch_ta_enforce(hipStream_t st, const TaArgs& a, uint32_t* bits);
void launch_ta_count(hipStream_t st, const TaArgs& a, const uint32_t* bits, unsigned long long* totals, uint32_t* table);
void launch_ta_scan(hipStream_t st, const TaArgs& a, const uint32_t* table, uint32_t* prefix);
void launch_ta_list(hipStream_t st, const TaArgs& a, const uint32_t* bits, const uint32_t* table, const uint32_t* prefix, uint32_t R, uint32_t* rows);
// product_audit.hip — the passes of the product audit (host/product_audit.hpp: contract; Prover::product_audit drives them), per chip.  The
// pivots are the invariant audit's (launch_ia_basis, launch_ia_merge: inv [2 + c]); pcols [rho]: the augmented pivot columns ascending (pcols[0] =
// 0, the constant; pcols[t] - 1 is a main column), q = rho - 1 independent columns, m = q (q + 1) / 2 pairs p <-> (ti, tj), 1 <= ti <= tj <= q,
// lexicographic.  Basis rows: NB2 workgroups of one wave eliminate RS consecutive rows each over the rho compacted columns and write the rows that
// raised the rank to a slot of rho + 1 words ([0] how many, then the rows ascending); the merge (a tree of fan IA_MERGE_FAN, one wave per node)
// inserts the slots' rows in order and keeps the ones that raise the rank: slot 0 of its result holds the rho first-independent rows.  Solve: G
// [rho][rho] the basis rows over Pi, inv [rho][rho] its inverse (aug: 2 rho^2 words of pool scratch, or null when pq_solve_in_lds(rho)), status
// [0] != 0: singular.  beta [m][rho], flags [m] (set to 1 by launch_pq_beta).  Sweep: pair list [n_list] (null: the pairs 0 .. n_list - 1), rows
// [0, n_rows): a mismatch stores 0 into flags[pair].  Compact: the listed pairs (null: 0 .. n_in - 1) whose flag is set, in order, and their count.
// Enforce: the rank audit's launch shape and inputs plus the E relations as sparse lists: eoff [E + 1] word offsets into ewords, entry e = main
// columns i, j, then (column, -beta as a Montgomery word) pairs; gstart [G + 1] the first entry of each group (a group is staged in LDS at a time:
// at most GE entries and GW words); totals: u64 [2 e] free rows, [2 e + 1] flat rows of relation e (zeroed); table / prefix: [E][NB] u32 free rows
// per workgroup and their exclusive prefix (table zeroed; the scan is launch_ra_scan); rows: [i_cut][R] u32.
struct PqArgs {
    RaArgs r;               // evaluations: the rank audit's dual row evaluations at most
    uint32_t rho;           // |Pi|
    const uint32_t* pcols;
    uint32_t RS, NB2;       // pq_rows_shape: rows per slice of the basis-row phase, slices
    uint32_t E, G, GE, GW;  // relations; groups, the most entries and the most words of a group
    const uint32_t *eoff, *ewords, *gstart;
};
constexpr uint32_t PQ_TILE_ROWS = 64, PQ_TILE_PAIRS = 32, PQ_PREFIX_ROWS = 256, PQ_GROUP_ENTRIES = 512, PQ_GROUP_WORDS = 8192;
inline uint64_t pq_pairs(uint32_t rho) { return rho ? (uint64_t)(rho - 1) * rho / 2 : 0; }
inline uint64_t pq_rows_words(const PqArgs& a) { return ((uint64_t)a.NB2 + (a.NB2 + IA_MERGE_FAN - 1) / IA_MERGE_FAN) * (a.rho + 1ull); }
inline bool pq_solve_in_lds(uint32_t rho) { return 4ull * (16ull + rho + 2ull * rho * rho) <= 160ull * 1024; }
inline uint64_t pq_totals_words(const PqArgs& a) { return 4ull * a.E; }  // u32 words of the u64 totals
void pq_rows_shape(PqArgs& a);  // RS and NB2 from the height and rho
void launch_pq_rows(hipStream_t st, const PqArgs& a, uint32_t* part);
void launch_pq_rowmerge(hipStream_t st, const PqArgs& a, uint32_t* part, uint32_t* rows);  // part is overwritten by the levels of the tree; rows [rho + 1]
void launch_pq_solve(hipStream_t st, const PqArgs& a, const uint32_t* rows, uint32_t* aug, uint32_t* G, uint32_t* inv, uint32_t* status);
void launch_pq_beta(hipStream_t st, const PqArgs& a, const uint32_t* G, const uint32_t* inv, uint32_t* beta, uint32_t* flags);
void launch_pq_sweep(hipStream_t st, const PqArgs& a, const char* name, uint64_t n_rows, const uint32_t* beta, const uint32_t* list, uint32_t n_list, uint32_t* flags);
void launch_pq_compact(hipStream_t st, const uint32_t* flags, const uint32_t* list, uint32_t n_in, uint32_t* out, uint32_t* count);
void launch_pq_gather(hipStream_t st, const PqArgs& a, const uint32_t* beta, const uint32_t* list, uint32_t n_list, uint32_t* out);
void pq_shape(PqArgs& a);  // ra_shape for this audit's LDS with a.E relations in groups of a.GE entries and a.GW words; throws std::invalid_argument when the chip does not fit
size_t pq_lds_bytes(const PqArgs& a, uint32_t NW, uint32_t T);
void launch_pq_count(hipStream_t st, const PqArgs& a, unsigned long long* totals, uint32_t* table);
void launch_pq_list(hipStream_t st, const PqArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t i_cut, uint32_t R, uint32_t* rows);
// domain_audit.hip — the passes of the domain audit (host/domain_audit.hpp: contract; Prover::domain_audit drives them), per chip.  A SLOT is a
// main column of an audited chip or a bus position record; a VIRTUAL COLUMN of a chip is a main column or an (interaction, field) gated by the
// interaction's count.  vt [NV][4]: kind (0 main column, 1 field), the main column or the word offset of the field vcol in iw, the word offset of
// the count vcol in iw, the slot.  tot [slots][5] u64: ~min, max, non-zero, wide, live (zeroed); bitmaps [slots][2048] u32 (zeroed); cls
// [slots][8] u32: distinct, class, dense, bits, narrow, min, max, 0.  Guard: gt = [0] items I, [1] W, item_at [W + 1], then per item (ascending
// column) the word offset of its interaction's count vcol in iw, its kind (host/domain_audit.hpp: DM_*), its appearance or ~0; gtot [5 W + A] u64:
// per column guarded, sent, received, mixed, unguarded non-zero rows, then per appearance its live rows (zeroed); table / prefix [W][NB] u32 the
// unguarded non-zero rows of a narrow column per workgroup and their exclusive prefix (table zeroed; the scan is launch_ra_scan over
// da_scan_args); rows [c_cut][R][2] u32 (row, canonical value).
constexpr uint32_t DA_TILE = 256, DA_MAX_SLICES = 2048, DA_BITMAP_WORDS = 2048, DA_TOT = 5, DA_CLS = 8, DA_GUARD_LDS_WORDS = 16 * 1024;
struct DaArgs {
    const uint32_t* main;  // column-major working layout (Montgomery), natural row order
    uint64_t mstride;
    const uint32_t* prep;  // null for a chip without preprocessed columns
    uint64_t pstride;
    uint64_t n;            // height, a power of two
    uint32_t width, prep_width;
    const uint32_t* iw;    // the chip's interactions (interactions.hpp: encode_interactions)
    const uint32_t* vt;
    uint32_t NV;           // virtual columns scanned = gridDim.y
    uint32_t TPS, S;       // da_shape: tiles of DA_TILE rows per slice, slices = gridDim.x
    const uint32_t* gt;
    uint32_t GW, A;        // words of gt; appearances
    uint32_t slot0;        // the slot of main column 0 (an audited chip's main columns have consecutive slots)
    uint32_t NB;           // workgroups of the guard pass = ceil(n / DA_TILE)
};
void da_shape(DaArgs& a, uint32_t max_slices = DA_MAX_SLICES);  // TPS, S, NB from the height
inline uint64_t da_guard_lds_words(const DaArgs& a) { return (uint64_t)a.GW + 5ull * a.width + a.A + 16; }
RaArgs da_scan_args(const DaArgs& a);  // what launch_ra_scan takes for table rows of NB words
void launch_da_scan(hipStream_t st, const DaArgs& a, unsigned long long* tot, uint32_t* bitmaps);
void launch_da_classify(hipStream_t st, const unsigned long long* tot, const uint32_t* bitmaps, uint32_t* cls, uint32_t n_slots, uint32_t max_bits);
void launch_da_guard(hipStream_t st, const DaArgs& a, uint32_t mode, const uint32_t* cls, unsigned long long* gtot, uint32_t* table, const uint32_t* prefix, uint32_t c_cut, uint32_t R,
                     uint32_t* rows);
// memory_audit.hip — the passes of the memory audit (host/memory_audit.hpp: contract; Prover::memory_audit drives them).  desc: the bus audit's
// descriptor (host/bus_audit.hpp).  mt: [0] entries, per entry (a chip with receives on the audited bus) 4 words: chip, first slot, receives R,
// the word offset in mt of its R interaction indices.  A slot is first_slot + row * R + k; n slots in all.  keys2 / ids2: [2 n] ping-pong halves
// for launch_ba_sort; tot: [MM_KEY_TOT] u64 (zeroed); rec: [MM_REC][n_live] u32; mark: [n_live]; block_before: [memory_audit_scan_blocks(n_live)];
// cnt: [MM_JUDGE_TOT] u64 (zeroed); table: [ceil(n_live / 256)] u32; out: [max_findings][MM_OUT] u32.
constexpr uint32_t MM_TILE = 256, MM_KEY_TOT = 5, MM_SCAN_ITEMS = 8, MM_SCAN_BLOCK = MM_SCAN_ITEMS * 256, MM_JUDGE_TOT = 16, MM_REC = 7, MM_NFIELDS = 8, MM_OUT = 16;
enum : uint32_t { MM_COUNT = 0, MM_LIST = 1 };
size_t memory_audit_scan_blocks(uint64_t n);
void launch_mm_keys(hipStream_t st, const uint32_t* desc, const uint32_t* mt, uint32_t entry, uint64_t height, uint32_t R, unsigned long long* keys, uint32_t* ids,
                    unsigned long long* tot);
void launch_mm_gather(hipStream_t st, const uint32_t* desc, const uint32_t* mt, const unsigned long long* keys, const uint32_t* ids, uint64_t n_live, uint64_t n, uint32_t* rec,
                      uint32_t* mark);
void launch_mm_scan(hipStream_t st, uint32_t* mark, uint64_t n_live, uint32_t* block_before);
// MM_COUNT: the counters and the findings per workgroup; MM_LIST (after it): scans the table in place and lists the first max_findings
void launch_mm_judge(hipStream_t st, uint32_t mode, const uint32_t* rec, const uint32_t* ids, const uint32_t* incl, const uint32_t* block_before, uint64_t n_live, uint64_t n,
                     unsigned long long* cnt, uint32_t* table, uint32_t max_findings, uint32_t* out);
// the memory audit's one-workgroup scan on its own: `a` [total] becomes its exclusive maximum (is_max) or sum, in place
void launch_mm_scan_words(hipStream_t st, uint32_t* a, uint64_t total, int is_max);
// program_audit.hip — the passes of the program audit (host/program_audit.hpp: contract; Prover::program_audit drives them).  The traces are
// working-layout views (column-major Montgomery): fmain the fetching chip's main trace [H rows], tmain / tprep the table chip's main and
// preprocessed traces [T rows].  counts: [T] u32 (zeroed); tot: [PG_TOT] u64 (zeroed); hard_tab, wrap_tab: [ceil(H / 256)]; tabs:
// [4][ceil(T / 256)]; out: [listed][PG_OUT] u32; ranges: [listed][2].
constexpr uint32_t PG_SLICE = 32768, PG_HIST_RUN = 4096, PG_TOT = 16, PG_OUT = 20, PG_LDS_TABLE_WORDS = 2048;
enum : uint32_t { PG_COUNT = 0, PG_LIST = 1 };
struct PgArgs {
    const uint32_t* fmain; uint64_t fstride, H;
    const uint32_t* tmain; uint64_t tmstride;
    const uint32_t* tprep; uint64_t tpstride;
    uint32_t T, rom_len, n_fields, pc_col, key_col, mult_col, lds_table, pad;
    uint32_t field_cols[8], table_cols[8];
};
// whether the judge stages the table's word columns in LDS: (n_fields + 1) * T words within PG_LDS_TABLE_WORDS.  A workgroup gathers at most
// 256 * n_fields words, so a copy much larger than that costs more than the gathers it saves.
bool program_audit_lds_table(uint32_t n_fields, uint64_t T);
void launch_pg_hist(hipStream_t st, const uint32_t* pc_col, uint64_t H, uint32_t T, uint32_t* counts);
// PG_COUNT: the counters and the two tables; PG_LIST (after it): scans the tables in place and lists
void launch_pg_judge(hipStream_t st, const PgArgs& a, uint32_t mode, unsigned long long* tot, uint32_t* hard_tab, uint32_t* wrap_tab, uint32_t hard_base, uint32_t max_hard,
                     uint32_t max_wrapped, uint32_t* out_hard, uint32_t* out_wrap);
void launch_pg_table(hipStream_t st, const PgArgs& a, uint32_t mode, const uint32_t* counts, unsigned long long* tot, uint32_t* tabs, uint32_t mult_base, uint32_t max_hard,
                     uint32_t max_ranges, uint32_t* out_hard, uint32_t* ranges);
// arithmetic_audit.hip — the passes of the arithmetic audit (host/arithmetic_audit.hpp: contract; Prover::arithmetic_audit drives them).  desc:
// the bus audit's descriptor (host/bus_audit.hpp).  An entry is (chip, interaction m) with `height` rows; its slots are first_slot + row and its
// workgroups block_base + ceil(row / 256) in the two tables.  verdict: [slots] u32 (written whole); tot: per entry [AR_TOT] u64 (zeroed);
// hard_tab, soft_tab: [workgroups of all entries] (written whole); out: [listed][AR_OUT] u32.
constexpr uint32_t AR_TOT = 32, AR_OUT = 24;
void launch_ar_judge(hipStream_t st, const uint32_t* desc, uint32_t chip, uint32_t m, uint64_t height, uint32_t first_slot, uint32_t block_base, uint32_t* verdict,
                     unsigned long long* tot, uint32_t* hard_tab, uint32_t* soft_tab);
// both tables become their own exclusive prefixes (the memory audit's one-workgroup scan)
void launch_ar_scan(hipStream_t st, uint32_t* hard_tab, uint32_t* soft_tab, uint64_t n_blocks);
void launch_ar_list(hipStream_t st, const uint32_t* desc, uint32_t chip, uint32_t m, uint32_t is_send, uint64_t height, uint32_t first_slot, uint32_t block_base,
                    const uint32_t* verdict, const uint32_t* hard_pre, const uint32_t* soft_pre, uint32_t max_hard, uint32_t max_soft, uint32_t* out_hard, uint32_t* out_soft);
// field_audit.hip — the passes of the field audit (host/field_audit.hpp: contract; Prover::field_audit drives them), per chip.  One wave per
// trace row, one wave per workgroup, T rows per workgroup one after the other, NB workgroups.  A SLOT of a chip is (interaction, field) in
// order, NS of them.  totals: u64 [0] live records, [1] floating fields, [2] rows with a floating field, [3 + m] live rows of interaction m,
// [3 + M + s] floating rows of slot s (all zeroed); table / prefix: [NS][NB] u32 floating rows of the slot per workgroup and their exclusive
// prefix (table zeroed); rows: [NS][R][18] u32 (zeroed).
constexpr uint32_t FA_MAX_FIELDS = 32;  // fields per interaction: a record's float mask is one word
struct FaArgs {
    const uint32_t* main;  // column-major working layout (Montgomery), natural row order
    uint64_t mstride;
    const uint32_t* prep;  // null for a chip without preprocessed columns
    uint64_t pstride;
    uint64_t n;            // height, a power of two
    uint32_t width, prep_width;
    const vair::Instr* prog;
    uint32_t n_instrs, n_regs, K;  // K = constraints of the chip
    const uint32_t* iw;            // the chip's interactions (interactions.hpp: encode_interactions): the counts, for liveness
    const uint32_t* wr;            // the interaction rows of the Jacobian (host/rank_audit.hpp: ra_weight_rows)
    uint32_t M, NS, F;             // interactions, slots, the most fields of one interaction
    int native_chip;               // a vchips::ChipId with constraints, CA_INTERPRET, or MA_BUS_ONLY
    uint32_t T, NB;                // fa_shape
    double evaluations;            // dual row evaluations of the counting pass at most: the profile's `ops`
};
inline uint64_t fa_totals_words(const FaArgs& a) { return 2 * (3ull + a.M + a.NS); }  // u32 words of the u64 totals
// Rows per workgroup and workgroups of a chip's launch; throws std::invalid_argument when the chip does not fit the LDS with one wave
void fa_shape(FaArgs& a);
size_t fa_lds_bytes(const FaArgs& a, uint32_t T);
void launch_fa_count(hipStream_t st, const FaArgs& a, unsigned long long* totals, uint32_t* table);
// slots below s_cut with a floating row are listed
void launch_fa_scan(hipStream_t st, const FaArgs& a, const uint32_t* table, uint32_t* prefix, uint32_t s_cut);
void launch_fa_list(hipStream_t st, const FaArgs& a, const uint32_t* table, const uint32_t* prefix, uint32_t s_cut, uint32_t R, uint32_t* rows);
// link_audit.hip — the passes of the link audit (host/link_audit.hpp: contract; Prover::link_audit drives them).  The mask pass runs per chip
// with the field audit's arguments (FaArgs; la_shape fills T and NB: its workgroup head is smaller than the field audit's) and writes one word
// per live record slot of `mask` [n] (zeroed); the records are grouped by the bus audit's launchers above; join, tally, select and report run
// over its sorted ids / gid / head_pos / nrec.  tmask: [groups] u32, pre-set to all ones.  lt: [0] fields of the whole machine (NS), [4 + c]
// where in lt chip c's interactions have their first field slots.  tally: la_tally_words u64, zeroed: [s] floating rows and [NS + s] open rows
// of field slot s, then per bus slot 66 words: tuples, open tuples, [2 + j] tuples in which position j is open, [34 + j] the records of those.
void la_shape(FaArgs& a);
size_t la_lds_bytes(const FaArgs& a, uint32_t T);
inline uint64_t la_tally_words(uint32_t n_fields, uint32_t n_buses) { return 2ull * n_fields + 66ull * n_buses; }
void launch_la_masks(hipStream_t st, const FaArgs& a, uint32_t first_id, uint32_t* mask);
void launch_la_join(hipStream_t st, const uint32_t* ids, const uint32_t* mask, const uint32_t* gid, uint32_t n_live, uint32_t* tmask);
void launch_la_tally(hipStream_t st, const uint32_t* desc, const uint32_t* lt, const uint32_t* ids, const uint32_t* mask, const uint32_t* gid, const uint32_t* head_pos, const uint32_t* tmask,
                     uint32_t n_live, uint32_t n_fields, uint32_t n_buses, unsigned long long* tally);
// appends (first record id, group) of the open groups, at most cap; counters[4] is the cursor (zero before)
void launch_la_select(hipStream_t st, const uint32_t* ids, const uint32_t* head_pos, const uint32_t* tmask, uint32_t n_groups, uint32_t cap, unsigned long long* ukeys, uint32_t* uvals,
                      uint32_t* counters);
// out: n_rep rows of 8 + widest bus + 2 R words (k_la_report states the layout)
void launch_la_report(hipStream_t st, const uint32_t* desc, const uint32_t* ids, const uint32_t* mask, const uint32_t* head_pos, const uint32_t* nrec, const uint32_t* tmask,
                      const uint32_t* uvals, uint32_t n_rep, uint32_t R, uint32_t* out);
// coverage_audit.hip — the passes of the coverage audit (host/coverage_audit.hpp: contract; Prover::coverage_audit drives them), per chip.  The
// evaluations are the mutation audit's (MaArgs; mutation_eval.hpp).  A CELL of a chip is ((detector * width + column) * D + delta index),
// cells = (K + M) * width * D of them.  audit: wg_tables [GX][cells][4] u32 {kills, sole, ~first_row, ~first_sole_row} (zeroed), one table per
// workgroup along the rows; detected: [4] u64 per delta (zeroed).  merge (folds wg_tables in place): counts [cells][2] u64, rows [cells][2] u32,
// every cell written.  pack: packed[0] = cells with kills > 0, [1] = 0, then [(K + M) * D][2] u64 the sums over columns of kills /
// sole (4 words each), then per listed cell (the first `cap`, ascending) 8 words: cell index, kills lo / hi, sole lo / hi, first_row,
// first_sole_row, 0.
struct CovArgs {
    MaArgs m;     // T, NB, CY as cov_shape chose them
    uint32_t M;   // interactions of the chip
    uint32_t GX;  // workgroups along the rows: workgroup x walks the row tiles x, x + GX, .. below NB
};
// Rows per workgroup, column slices and workgroups along the rows (max_workgroups != 0: at most that many) of a chip's launch; throws
// std::invalid_argument when no tile of the chip fits the LDS
void cov_shape(CovArgs& v, uint32_t max_workgroups);
inline uint64_t cov_cells(const CovArgs& v) { return (uint64_t)(v.m.K + v.M) * v.m.width * v.m.D; }
inline uint64_t cov_packed_words(const CovArgs& v, uint64_t cap) { return 2 + 4ull * (v.m.K + v.M) * v.m.D + 8 * cap; }
void launch_cov_audit(hipStream_t st, const CovArgs& v, uint32_t* wg_tables, unsigned long long* detected);
void launch_cov_merge(hipStream_t st, const CovArgs& v, uint32_t* wg_tables, unsigned long long* counts, uint32_t* rows);
void launch_cov_pack(hipStream_t st, const CovArgs& v, const unsigned long long* counts, const uint32_t* rows, uint32_t cap, uint32_t* packed);
// open.hip
void launch_bary_weights(hipStream_t st, uint64_t n, const uint32_t* min_poly_dev, Fp shift, const DeviceTables& tb, uint32_t* w);
// the same for several (height, point) pairs in one launch: job = { first block (u32), pad, n (u64), min-poly pointer, weight buffer, digit-plane image (or null) }
void launch_bary_weights_batch(hipStream_t st, const uint32_t* jobs_dev, uint32_t n_jobs, uint32_t total_blocks, double total_rows, Fp shift, const DeviceTables& tb);
uint32_t bary_weights_blocks(uint64_t n);
bool bary_weights_has_image(uint64_t n);
uint64_t col_dot_slots(uint64_t n);
uint64_t bary_buffer_words(uint64_t n);  // words of a weight vector launch_bary_weights fills (launch_col_dot takes such buffers)
uint64_t col_dot_max_columns(int np);  // widest matrix (view) one k_col_dot launch takes for np points; wider ones are opened in column chunks
// finish = false: only the partial sums; the caller collects a job per launch (col_dot_finish_job: appends its 12-word image to `jobs`, returns the next first
// block) and finishes all of them with ONE launch_col_dot_finish_batch behind the launches (jobs_dev = the uploaded images)
void launch_col_dot(hipStream_t st, DMatView m, uint64_t n, int np, const uint32_t* w0, const uint32_t* w1, uint32_t* partial,
                    const uint32_t* scale5_dev, uint32_t* out_dev, bool finish = true);
uint32_t col_dot_finish_job(std::vector<uint32_t>& jobs, uint32_t first_block, uint64_t n, uint64_t width, int np, const uint32_t* partial, const uint32_t* scale5_dev, uint32_t* out_dev);
void launch_col_dot_finish_batch(hipStream_t st, const uint32_t* jobs_dev, uint32_t n_jobs, uint32_t total_blocks);
// accumulate: add to the vector already in `out` (a height with more than MAX_OPEN_POINTS_PER_LAUNCH distinct opening points is
// reduced in several launches)
constexpr int MAX_OPEN_POINTS_PER_LAUNCH = 4;
// Y of every (matrix, point) written into the reduce descriptors on the device (open.hip, k_open_y)
void launch_open_y(hipStream_t st, const uint32_t* vals_dev, const uint32_t* apow_dev, const uint32_t* desc_dev, const uint32_t* entry_off_dev, uint32_t n_entries, uint32_t* pool_dev);
// n_points: the descriptor's number of distinct points (1 .. MAX_OPEN_POINTS_PER_LAUNCH; sizes the 4-rows-per-thread kernel's arrays; anything else = the maximum)
// vec_ok: the caller's word that every matrix of the descriptor has a 16-byte-aligned base and a column stride that is a multiple of 4 words
// (reduce_vec_ok below, evaluated where the descriptor is built — the pointers live in device memory here).  The R-rows-per-thread kernel reads the
// columns with 8- / 16-byte loads and needs that, `out` 16-byte aligned and L a power of two >= 1024; anything else takes the thread-per-row kernel.
inline bool reduce_vec_ok(const void* col0, uint64_t stride_words) { return ((uintptr_t)col0 & 15) == 0 && (stride_words & 3) == 0; }
void launch_reduce_openings(hipStream_t st, const uint32_t* desc_dev, uint64_t L, Fp shift, const DeviceTables& tb, uint32_t* out, uint64_t total_width,
                            bool accumulate, int n_points, bool vec_ok);
// beta5_dev: the folding challenge as 5 Montgomery words in device memory (written by k_fri_challenge)
void launch_fri_fold(hipStream_t st, const uint32_t* in, uint64_t L, const uint32_t* beta5_dev, const uint32_t* add, const DeviceTables& tb, uint32_t* out);
// One DuplexChallenger step on the device: observe the 8-word root at digest8_dev, sample beta into beta5_dev; the root is
// also copied to commit8_dev.  pos_dev: [480 Poseidon round constants][16 circulant MDS coefficients]; ch_dev: 50-word state.
constexpr int DEV_CHALLENGER_WORDS = 50;
void launch_fri_challenge(hipStream_t st, const uint32_t* pos_dev, uint32_t* ch_dev, const uint32_t* digest8_dev, uint32_t* beta5_dev, uint32_t* commit8_dev);
void launch_pow_grind(hipStream_t st, const uint32_t* pos_dev, bool sparse, uint32_t k_pending, uint32_t first, uint32_t count, uint32_t bits, uint32_t* best_dev);
void launch_gather(hipStream_t st, const uint32_t* desc_dev, uint64_t n_desc, uint32_t* dst);
// the same from 8-word templates and the query indices (<= 256 queries: the query id is a byte) — open.hip, k_gather_q
void launch_gather_q(hipStream_t st, const uint32_t* templ_dev, uint64_t n_desc, const uint32_t* indices_dev, uint32_t* dst);

}  // namespace vk
