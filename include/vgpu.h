/*
 * vgpu.h — C ABI of the MI355X-native STARK prover backend for Valida (libvgpu.so).
 *
 * This is the drop-in boundary for ONE path of the reference: Machine::prove
 * (basic/src/lib.rs:147-675) and the traits it drives — StarkConfig (machine/src/config.rs:7-31),
 * Pcs: UnivariatePcsWithLde (call sites basic/src/lib.rs:199,201,223,225,258,261,594,599,619),
 * generate_permutation_trace (machine/src/chip.rs:121-130), quotient (machine/src/quotient.rs:18-37)
 * and the Fiat-Shamir challenger (basic/src/lib.rs:185-263,601-619).  The reference has no FFI of its
 * own (all Rust generics); every entry point below names the reference item it replaces.  A Rust host
 * binds it with #[repr(C)] structs — see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; all structs are POD.
 *   - field elements cross the ABI as canonical u32 < p = 2013265921 (BabyBear); extension elements
 *     (BinomialExtensionField<BabyBear,5>) as 5 consecutive u32; digests as 8 u32.
 *   - matrices cross as the reference's RowMajorMatrix<Val>: row-major u32[height * width].
 *   - every function returns VGPU_OK (0) or a negative status; vgpu_last_error() gives the message of
 *     the last failure on the calling thread.  Nothing unwinds across the ABI.
 *   - one vgpu_prover per device; a prover is not thread-safe; calls are host-synchronous.
 *   - the library never falls back to a CPU implementation: without a usable HIP device
 *     vgpu_prover_create fails with VGPU_ERR_HIP.
 */
#ifndef VGPU_H
#define VGPU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    VGPU_OK = 0,
    VGPU_ERR_INVALID_ARG = -1,
    VGPU_ERR_OOM = -2,
    VGPU_ERR_HIP = -3,
    VGPU_ERR_UNSUPPORTED = -4,
    VGPU_ERR_INTERNAL = -5,
    VGPU_ERR_FABRIC = -6   /* a sharded proof was given up because a peer rank failed, or the transport itself failed / ran into its deadline */
};
enum {
    VGPU_HASH_KECCAK256 = 0,  /* the reference's MMCS: SerializingHasher32<Keccak256Hash> + CompressionFunctionFromHasher (basic/tests/test_prover.rs:424-431) */
    VGPU_HASH_POSEIDON16 = 1  /* BASELINE.json north-star variant: PaddingFreeSponge<Perm16, 16, 8, 8> + TruncatedPermutation<Perm16, 2, 8, 16> over the
                                 challenger's Poseidon-16 (same round constants); the reference never instantiates it */
};

const char* vgpu_last_error(void);
const char* vgpu_version(void);

/* ---- StarkConfig (machine/src/config.rs:7-31; instantiated at basic/tests/test_prover.rs:413-455) ---- */
typedef struct vgpu_config {
    int32_t device;                /* HIP device ordinal */
    uint32_t log_blowup;           /* FriConfig.log_blowup      (test_prover.rs:443) */
    uint32_t num_queries;          /* FriConfig.num_queries     (:444) */
    uint32_t pow_bits;             /* FriConfig.proof_of_work_bits (:445) */
    uint32_t hash_kind;            /* VGPU_HASH_KECCAK256 | VGPU_HASH_POSEIDON16 */
    uint32_t observe_final_poly;   /* convention switch, default 0 */
    uint32_t poseidon_rc[480];     /* Poseidon<_,CosetMds<16>,16,5> round constants (test_prover.rs:418-422), canonical */
    uint32_t interpret_air;        /* 0: BasicMachine chips run their ahead-of-time compiled eval kernels; 1: every AIR, in-tree
                                      or captured through vgpu_air_*, runs as an interpreted register program (same values) */
} vgpu_config_t;

/* ---- AIR capture: the FFI image of SymbolicAirBuilder (machine/src/symbolic/symbolic_builder.rs:57-154).
 * A host runs its unchanged Chip::eval against a builder that forwards to these calls; node ids are
 * opaque u32 handles.  Interactions mirror Interaction/VirtualPairCol (machine/src/chip.rs:76-94). ---- */
typedef struct vgpu_air vgpu_air_t;
typedef struct vgpu_vcol_term { uint32_t is_preprocessed; uint32_t column; uint32_t weight; } vgpu_vcol_term_t;
typedef struct vgpu_vcol { const vgpu_vcol_term_t* terms; uint32_t n_terms; uint32_t constant; } vgpu_vcol_t;
typedef struct vgpu_interaction {
    const vgpu_vcol_t* fields; uint32_t n_fields;
    vgpu_vcol_t count;
    uint32_t is_global;   /* BusArgument::Global / Local */
    uint32_t bus_index;
    uint32_t is_send;     /* InteractionType::*Send / *Receive */
} vgpu_interaction_t;

/* The expression calls return a handle and no status.  A handle stands for the expression AS WRITTEN: the capture shares and folds equal
 * sub-expressions (x * 0 is the constant 0), but an expression's degree is the reference's (symbolic_expression.rs:36-62: a product adds its
 * operands' degrees whatever they are), so an AIR gets the log_quotient_degree it gets when captured by SymbolicAirBuilder.  Misuse -- a column
 * outside [0, width) or [0, preprocessed_width), a handle this AIR has not returned -- gives the handle 0xFFFFFFFF (which is never valid), and the
 * AIR is refused by vgpu_machine_push_air with VGPU_ERR_INVALID_ARG and a message naming the AIR and the first misuse. */
int32_t vgpu_air_new(const char* name, uint32_t width, uint32_t preprocessed_width, vgpu_air_t** out);
void vgpu_air_free(vgpu_air_t* air);
uint32_t vgpu_air_constant(vgpu_air_t* air, uint32_t canonical);                                  /* SymbolicExpression::Constant */
uint32_t vgpu_air_variable(vgpu_air_t* air, uint32_t is_preprocessed, uint32_t column, uint32_t is_next); /* ::Variable */
uint32_t vgpu_air_is_first_row(vgpu_air_t* air);
uint32_t vgpu_air_is_last_row(vgpu_air_t* air);
uint32_t vgpu_air_is_transition(vgpu_air_t* air);
uint32_t vgpu_air_add(vgpu_air_t* air, uint32_t a, uint32_t b);
uint32_t vgpu_air_sub(vgpu_air_t* air, uint32_t a, uint32_t b);
uint32_t vgpu_air_mul(vgpu_air_t* air, uint32_t a, uint32_t b);
uint32_t vgpu_air_neg(vgpu_air_t* air, uint32_t a);
void vgpu_air_assert_zero(vgpu_air_t* air, uint32_t node);                                       /* AirBuilder::assert_zero */
int32_t vgpu_air_add_interaction(vgpu_air_t* air, const vgpu_interaction_t* it);                 /* Chip::all_interactions order */

/* ---- Machine: ordered chips (basic/src/lib.rs:151-166) ---- */
typedef struct vgpu_machine vgpu_machine_t;
int32_t vgpu_machine_new(vgpu_machine_t** out);
/* compiles the constraint program.  log_quotient_degree 1 (every reference chip) .. 3 (constraint degree <= 9) is implemented;
 * beyond that VGPU_ERR_UNSUPPORTED with a message naming the AIR and its degree.  VGPU_ERR_INVALID_ARG: the capture was misused (above), or the
 * program needs more registers than the device interpreters hold in a workgroup's LDS (592 at log_quotient_degree 1, 640 above) */
int32_t vgpu_machine_push_air(vgpu_machine_t* m, const vgpu_air_t* air);
int32_t vgpu_machine_basic(vgpu_machine_t** out);                         /* the 14-chip BasicMachine from the in-tree chip definitions */
/* the same 14 chips, but captured the way a foreign host captures them: each chip's eval runs against a builder that only
 * calls vgpu_air_* / vgpu_air_add_interaction, then vgpu_machine_push_air (no native kernels: the interpreted path) */
int32_t vgpu_machine_basic_via_ffi(vgpu_machine_t** out);
void vgpu_machine_free(vgpu_machine_t* m);
uint32_t vgpu_machine_num_chips(const vgpu_machine_t* m);
/* per-chip facts: width, preprocessed width, #interactions, log_quotient_degree (get_log_quotient_degree,
 * symbolic_builder.rs:17-30), #constraints, program length, registers */
int32_t vgpu_machine_chip_info(const vgpu_machine_t* m, uint32_t chip, uint32_t out[8]);
/* Neutral word image of chip `chip`'s interactions in Chip::all_interactions order (machine/src/chip.rs:40-63; test hook):
 *   [n] then per interaction: [is_send] [is_global] [bus_index] [n_fields] count_vcol field_vcols..;
 *   vcol = [n_terms] [constant] n_terms x ([is_preprocessed] [column] [weight]).  Returns the word count (copies when out has room). */
int64_t vgpu_machine_interaction_words(const vgpu_machine_t* m, uint32_t chip, uint32_t* out, uint64_t cap);
/* Host interpretation of chip `chip`'s compiled program on one row pair (test hook; no GPU needed).
 * values out: the asserted constraint values in order; returns their count or a negative status. */
int32_t vgpu_machine_eval_constraints(const vgpu_machine_t* m, uint32_t chip, const uint32_t* main_local, const uint32_t* main_next,
                                      const uint32_t* prep_local, const uint32_t* prep_next, uint32_t is_first, uint32_t is_last,
                                      uint32_t is_transition, uint32_t* out, uint32_t cap);

/* ---- Challenger: DuplexChallenger<Val, Poseidon16, 16> (basic/src/lib.rs:185,200,224,229,...) ---- */
typedef struct vgpu_challenger vgpu_challenger_t;
int32_t vgpu_challenger_new(const uint32_t poseidon_rc[480], vgpu_challenger_t** out);
void vgpu_challenger_free(vgpu_challenger_t* ch);
void vgpu_challenger_observe(vgpu_challenger_t* ch, const uint32_t* values, uint64_t n);         /* CanObserve */
void vgpu_challenger_sample(vgpu_challenger_t* ch, uint32_t* out, uint64_t n);                    /* sample / sample_ext_element = 5 samples */
uint64_t vgpu_challenger_sample_bits(vgpu_challenger_t* ch, uint32_t bits);
uint32_t vgpu_challenger_grind(vgpu_challenger_t* ch, uint32_t bits);                             /* smallest witness */
void vgpu_poseidon16_permute(const uint32_t poseidon_rc[480], uint32_t state[16]);
/* the same permutation through the sparse-matrix form of the 22 partial rounds that the Poseidon-MMCS kernels use (test hook) */
int32_t vgpu_poseidon16_permute_sparse(const uint32_t poseidon_rc[480], uint32_t state[16]);

/* ---- Prover (one per device) ---- */
typedef struct vgpu_prover vgpu_prover_t;
typedef struct vgpu_trace vgpu_trace_t;   /* a RowMajorMatrix resident in HBM */
typedef struct vgpu_pdata vgpu_pdata_t;   /* Pcs::ProverData: committed LDEs + Merkle tree, in HBM */
typedef struct vgpu_proof vgpu_proof_t;

int32_t vgpu_prover_create(const vgpu_config_t* cfg, const vgpu_machine_t* machine, vgpu_prover_t** out);
void vgpu_prover_destroy(vgpu_prover_t* p);
/* bytes currently held / peak in the HBM pool */
void vgpu_prover_memory(const vgpu_prover_t* p, uint64_t* live_bytes, uint64_t* peak_bytes);
/* The prover caches device blocks by size and reuses them (no hipMalloc in the steady state).  Returns the cached-but-unused
 * blocks to the driver (bytes freed); also done automatically, once, when an allocation runs out of memory. */
uint64_t vgpu_prover_trim(vgpu_prover_t* p);
/* The pool's peak restarts from what is held now (a host that wants the high-water mark of ONE phase: bench.py reports the proving path's own). */
void vgpu_prover_memory_reset_peak(vgpu_prover_t* p);
/* The device's dense lane: the contexts of one device take turns in the big Merkle-tree launches of vgpu_prove / vgpu_prove_async (a thread per
 * node; they fill the chip's VALU issue slots on their own), so that one proof's tree phase runs beside the others' LDE, quotient and opening
 * phases instead of beside their tree phases.  Scheduling only: no proof word depends on it.  On by default for trees of at least 2^18 leaf
 * rows; `on` = 0 switches it off for this context, `min_nodes` > 0 sets the smallest tree that takes it (0 keeps the current value).  Takes
 * effect with the next proof.  (The Python binding calls this at context creation from VGPU_DENSE_LANE and VGPU_DENSE_LANE_MIN_NODES.) */
void vgpu_prover_set_dense_lane(vgpu_prover_t* p, uint32_t on, uint64_t min_nodes);
/* Constant columns: while vgpu_prove / vgpu_prove_async brings an uploaded main or preprocessed trace of more than 2^12 rows into the device layout it
 * compares every row of every column with row 0, on the device and inside the proof, and the low-degree extension fills the columns found constant
 * with that value instead of transforming them (the extension of a constant polynomial is the constant).  No proof word depends on it; proving TIME
 * depends on which columns of the traces are constant.  On by default; `on` = 0 transforms every column.  Takes effect with the next proof.
 * (The Python binding calls this at context creation from VGPU_CONST_COLS.) */
void vgpu_prover_set_const_columns(vgpu_prover_t* p, uint32_t on);
/* how many trees of this context entered the lane, and how many of those had to wait for ANOTHER context's event; both stay 0 with the lane off */
void vgpu_prover_lane_stats(const vgpu_prover_t* p, uint64_t* entered, uint64_t* waited);

/* per-kernel HIP-event timing (bench): switch on/off (resets the accumulators); the profile is text,
 * one line per kernel: "name launches total_ms total_algorithmic_bytes".  Returns the size needed. */
void vgpu_prover_set_profiling(vgpu_prover_t* p, uint32_t on);
/* Optional, off by default: keep the commitment to the PREPROCESSED traces (program ROM, range table: it depends on the machine and the program only,
 * not on the witness) across proofs while the SAME vgpu_trace_t handles are handed in again — working-layout copies, LDEs and tree stay on the
 * device; any other set (a re-upload of equal contents included) recomputes it; the root is observed into the transcript every time.  Saves one
 * synchronisation point and about 40 small launches per proof.  VGPU_PREP_CACHE=1 in the environment enables it for provers created afterwards. */
void vgpu_prover_set_prep_cache(vgpu_prover_t* p, uint32_t on);
/* restrict the timing to launches of ONE kernel name (NULL or "" = all): every timed launch carries a pair of events, which costs
 * the host and the command processor a little; a throughput measurement times only the kernel it reports a roofline for */
void vgpu_prover_set_profiling_filter(vgpu_prover_t* p, const char* kernel_name);
int64_t vgpu_prover_profile(vgpu_prover_t* p, char* out, uint64_t cap);
/* Measurement aid (bench.py's roofline): the shader clock the device sustains RIGHT NOW.  One wave on a stream of its own runs `iters` dependent
 * VALU additions and reads the shader-cycle counter and the 100 MHz wall clock before and after: out[0] = shader cycles, out[1] = wall ticks
 * (clock in Hz = out[0] / out[1] * 1e8).  Blocks the caller for the few tens of microseconds the wave runs; safe beside running proofs (no
 * allocation, no device-wide synchronisation after the first call).  Needs a HIP device. */
int32_t vgpu_shader_clock_probe(int32_t device, uint32_t iters, uint64_t out[2]);

/* Page-locked host memory for the matrices a host hands over: vgpu_trace_upload / vgpu_oplog_upload from such a buffer is one DMA at
 * PCIe rate; from ordinary (pageable) memory the runtime stages the copy through its own bounce buffers on the calling thread, which
 * at 516 MB of main traces per C2 proof is slower than the proof itself (bench.py: pcie_inclusive).  A Rust host would back its
 * RowMajorMatrix<Val> values with this allocator.  Needs a HIP device; free with vgpu_host_free. */
int32_t vgpu_host_alloc(uint64_t bytes, void** out);
void vgpu_host_free(void* ptr);

/* H2D of a host RowMajorMatrix (the reference passes these by value, basic/src/lib.rs:223) */
int32_t vgpu_trace_upload(vgpu_prover_t* p, const uint32_t* data, uint64_t height, uint64_t width, vgpu_trace_t** out);
void vgpu_trace_free(vgpu_trace_t* t);

/* pcs.commit_batches / commit_shifted_batches (basic/src/lib.rs:199,223,258,599): coset_shifts may be NULL */
int32_t vgpu_commit_batches(vgpu_prover_t* p, const vgpu_trace_t* const* mats, uint32_t n_mats, const uint32_t* coset_shifts,
                            uint32_t root[8], vgpu_pdata_t** out);
/* The main commitment round as vgpu_prove runs it, on its own (a test hook): uploaded row-major matrices only, no coset shifts; the ingest flags the
 * columns in which some row differs from row 0 and — with vgpu_prover_set_const_columns on — the LDE of a matrix of more than 2^12 rows fills the
 * unflagged columns instead of transforming them.  Root and LDEs are those of vgpu_commit_batches either way.  varies_out (may be NULL): the flags,
 * one word per column, matrix after matrix (0 = constant column). */
int32_t vgpu_commit_batches_flagged(vgpu_prover_t* p, const vgpu_trace_t* const* mats, uint32_t n_mats, uint32_t root[8], vgpu_pdata_t** out,
                                    uint32_t* varies_out);
/* pcs.get_ldes (basic/src/lib.rs:201,225,261): copy LDE `idx` back as row-major canonical, rows in
 * COMMITTED (bit-reversed) order; out must hold (height << log_blowup) * width words */
int32_t vgpu_pdata_lde(vgpu_prover_t* p, const vgpu_pdata_t* pd, uint32_t idx, uint32_t* out, uint64_t cap_words);
/* pcs.get_ldes without a copy: the committed LDE `idx` where it lives in HBM.  Column-major (column c at data + c * stride),
 * Montgomery form (x * 2^32 mod p), rows in COMMITTED order: storage row j holds the evaluation at coset_shift * w^bitrev(j),
 * i.e. the reference's natural-order view row i is storage row bitrev(i); `vertically_strided(stride, offset)`
 * (machine/src/quotient.rs:41-47) = the first height / stride storage rows.  Valid until vgpu_pdata_free. */
typedef struct vgpu_lde_view {
    const uint32_t* data;   /* device pointer */
    uint64_t height, width, stride;
    uint32_t log_blowup;
} vgpu_lde_view_t;
uint32_t vgpu_pdata_num_matrices(const vgpu_pdata_t* pd);
int32_t vgpu_pdata_lde_view(const vgpu_pdata_t* pd, uint32_t idx, vgpu_lde_view_t* out);
void vgpu_pdata_free(vgpu_pdata_t* pd);

/* generate_permutation_trace (machine/src/chip.rs:121-208) for chip `chip` of the prover's machine.
 * challenges: 3 extension elements (15 words).  out: height x 5(M+1) row-major (flatten_to_base),
 * cumulative_sum: 5 words. */
int32_t vgpu_perm_trace(vgpu_prover_t* p, uint32_t chip, const vgpu_trace_t* main, const vgpu_trace_t* preprocessed_or_null,
                        const uint32_t challenges[15], uint32_t* out, uint64_t cap_words, uint32_t cumulative_sum[5]);

/* The same, leaving the permutation trace in HBM as a trace handle (flatten_to_base layout: ready for vgpu_commit_batches) —
 * the call a host makes at basic/src/lib.rs:232-258 when it drives the phases itself. */
int32_t vgpu_perm_trace_device(vgpu_prover_t* p, uint32_t chip, const vgpu_trace_t* main, const vgpu_trace_t* preprocessed_or_null,
                               const uint32_t challenges[15], vgpu_trace_t** out, uint32_t cumulative_sum[5]);

/* quotient (machine/src/quotient.rs:18-37) of chip `chip`: evaluates Air::eval + eval_permutation_constraints on the quotient
 * domain from the chip's three committed LDEs (pcs.get_ldes of the preprocessed / main / permutation rounds: matrix indices
 * within each ProverData; prep_pd may be NULL for chips without preprocessed columns), divides by the zerofier, decomposes and
 * flattens (quotient.rs:63-67).  Result: the height x (5 << log_quotient_degree) chunk matrix as a trace handle, to be committed
 * with vgpu_commit_batches(.., coset_shifts = coset_shift^(2^log_quotient_degree)) (basic/src/lib.rs:593-599). */
int32_t vgpu_quotient(vgpu_prover_t* p, uint32_t chip, const vgpu_pdata_t* prep_pd, uint32_t prep_idx, const vgpu_pdata_t* main_pd, uint32_t main_idx,
                      const vgpu_pdata_t* perm_pd, uint32_t perm_idx, const uint32_t perm_challenges[15], const uint32_t alpha[5],
                      const uint32_t cumulative_sum[5], vgpu_trace_t** out);

/* pcs.open_multi_batches (basic/src/lib.rs:611-619).  rounds[r]: ProverData of round r; points: for every round, for every
 * committed matrix of that round (commit order), n_points[k] extension elements (5 words each), all concatenated; n_points has
 * one entry per (round, matrix).  The transcript `ch` is advanced as the reference's `&mut challenger` is (batch challenge, FRI
 * betas, proof-of-work witness, query indices).  Result handle:
 *   vgpu_opening_values: openings[round][matrix][point][column] flattened in that order, 5 words per value (lib.rs:622-645);
 *   vgpu_opening_proof:  the TwoAdicFriPcsProof as words — exactly the tail of vgpu_proof_words after the per-chip section. */
typedef struct vgpu_opening vgpu_opening_t;
int32_t vgpu_open_multi_batches(vgpu_prover_t* p, const vgpu_pdata_t* const* rounds, uint32_t n_rounds, const uint32_t* n_points,
                                const uint32_t* points, vgpu_challenger_t* ch, vgpu_opening_t** out);
uint64_t vgpu_opening_values_len(const vgpu_opening_t* o);
const uint32_t* vgpu_opening_values(const vgpu_opening_t* o);
uint64_t vgpu_opening_proof_len(const vgpu_opening_t* o);
const uint32_t* vgpu_opening_proof(const vgpu_opening_t* o);
void vgpu_opening_free(vgpu_opening_t* o);

/* pcs.verify_multi_batches (basic/src/lib.rs:825-837).  Host-only (no device is touched; only log_blowup, num_queries, pow_bits,
 * hash_kind, observe_final_poly and poseidon_rc of `cfg` are read).  commits: n_rounds x 8 words; n_mats[r] matrices per round;
 * heights / widths / n_points: one entry per (round, matrix), rounds concatenated, heights = TRACE heights (Dimensions);
 * points / values: as vgpu_open_multi_batches takes / returns them; proof: vgpu_opening_proof words.  The transcript `ch`
 * must be in the state the prover's was in when it called open_multi_batches.  Returns VGPU_OK if the opening is accepted,
 * VGPU_ERR_INVALID_ARG with the reason in vgpu_last_error() if it is rejected. */
int32_t vgpu_verify_multi_batches(const vgpu_config_t* cfg, const uint32_t* commits, uint32_t n_rounds, const uint32_t* n_mats, const uint64_t* heights,
                                  const uint32_t* widths, const uint32_t* n_points, const uint32_t* points, const uint32_t* values, uint64_t n_value_words,
                                  const uint32_t* proof, uint64_t n_proof_words, vgpu_challenger_t* ch);

/* Machine::verify (basic/src/lib.rs:677-1064; verify_constraints, machine/src/verify.rs:11-107): checks a proof produced by vgpu_prove
 * (flat "VPF1" words) against `machine` on the HOST — transcript, pcs.verify_multi_batches over the three rounds, every chip's AIR and
 * permutation constraints out of domain against Z_H(zeta) * quotient(zeta), and that the chips' cumulative sums cancel.  Needs no device.
 * preprocessed_commit: the commitment of the preprocessed traces (8 words; the reference's verifier recomputes it with
 * pcs.commit_batches(preprocessed_traces), lib.rs:791-804: vgpu_host_commit_root does that on the host), or NULL for a machine without
 * preprocessed traces.  Returns VGPU_OK when the proof is accepted, VGPU_ERR_INVALID_ARG with the reason in vgpu_last_error when not. */
int32_t vgpu_verify(const vgpu_config_t* cfg, const vgpu_machine_t* machine, const uint32_t* preprocessed_commit, const uint32_t* proof_words,
                    uint64_t n_words);
/* ---- Batched Machine::verify on the device (vgpu_verify's verdicts over many proofs; kernels/verify.hip).  A verifier handle is apart from
 * vgpu_prover_t: a verify-only host builds no prover tables.  cfg: device, log_blowup, num_queries, pow_bits, hash_kind, observe_final_poly,
 * poseidon_rc (what vgpu_verify reads, plus the device); the machine description is copied.  The parse, the transcript, the proof of work,
 * every shape check, the out-of-domain constraint check and the cumulative sums run on at most 16 host threads; every Merkle opening, the
 * reduced openings and the FRI fold of every query run on the device.  Proofs are checked in chunks of at most chunk_words proof words
 * (default 2^25, about 150 MiB of device buffer; a larger single proof is a chunk of its own), so a batch of any size runs in bounded HBM. */
typedef struct vgpu_verifier vgpu_verifier_t;
int32_t vgpu_verifier_create(const vgpu_config_t* cfg, const vgpu_machine_t* machine, vgpu_verifier_t** out);
void vgpu_verifier_destroy(vgpu_verifier_t* v);
int32_t vgpu_verifier_set_chunk_words(vgpu_verifier_t* v, uint64_t chunk_words);
/* Machine::verify of n_proofs proofs (flat VPF1 words each).  preprocessed_commits: n_proofs x 8 words (proof i's preprocessed commitment,
 * the same rule as vgpu_verify's argument), or NULL for a machine without preprocessed traces.  status[i] = VGPU_OK or VGPU_ERR_INVALID_ARG:
 * exactly vgpu_verify's verdict on proof i, and vgpu_verifier_message(v, i) its message.  The call itself fails only on a device or
 * allocation error. */
int32_t vgpu_verify_batch(vgpu_verifier_t* v, const uint32_t* const* proofs, const uint64_t* n_words, const uint32_t* preprocessed_commits,
                          uint32_t n_proofs, int32_t* status);
/* the rejection message of proof i of the last batch ("" when accepted): its byte length, copied (NUL-terminated) when out has room */
int64_t vgpu_verifier_message(const vgpu_verifier_t* v, uint32_t i, char* out, uint64_t cap);
/* wall time of the last batch: host stages (plans, packing, verdicts, constraints) and device stage (upload, kernels, flags back), ms */
void vgpu_verifier_timing(const vgpu_verifier_t* v, double* host_ms, double* device_ms);
/* pcs.commit_batches / commit_shifted_batches on the HOST (the same LDE and MMCS conventions as vgpu_commit_batches, plain O(n log n)
 * code): for the small matrices a verifier commits itself.  mats[i]: canonical row-major heights[i] x widths[i]. */
int32_t vgpu_host_commit_root(const vgpu_config_t* cfg, const uint32_t* const* mats, const uint64_t* heights, const uint64_t* widths, uint32_t n_mats,
                              const uint32_t* coset_shifts, uint32_t root[8]);

/* FRI fold_even_odd of an Ext5 vector (n x 5 words, bit-reversed domain order) — App. B10 */
int32_t vgpu_fri_fold(vgpu_prover_t* p, const uint32_t* f, uint64_t n, const uint32_t beta[5], uint32_t* out);

/* Test hook: primitive `op` of the device's field arithmetic (kernels/field_probe.hip: reduce_once, sub_mod, the Montgomery reductions, Ext5
 * products, the radix-16 butterfly network, the signed S-box, the Poseidon-16 permutation — the functions the proving kernels call) on n_items
 * operand tuples, one work item each.  Operands and results are RAW STORED (Montgomery) WORDS, nothing is converted: word k of item i is
 * operands[k * n_items + i] / results[k * n_items + i].  operand_words / result_words: the buffers' sizes, n_items times the op's words per item (else
 * VGPU_ERR_INVALID_ARG).  Ops and their shapes: valida_amd.FIELD_PROBE_OPS.  Arithmetic operands outside an op's documented domain give
 * unspecified words; a butterfly item whose low / lowbits would index past the twiddle tables is refused. */
int32_t vgpu_field_probe(vgpu_prover_t* p, uint32_t op, const uint32_t* operands, uint64_t operand_words, uint64_t n_items, uint32_t* results, uint64_t result_words);

/* Test hook: the lazily folded sums of the device's field arithmetic (kernels/lazy_probe.hip) on n_items operand tuples of RAW STORED WORDS, laid
 * out as vgpu_field_probe's.  op 0 fold_hi: (lo, hi), hi < 2p -> (lo, hi); op 1 ext_mul: a[5], b[5] -> a b; op 2 lin_dot: terms x { A[5], v } -> sum A v,
 * terms = 1 .. 17 or 34, unrolled; op 3 ext_dot: terms x { A[5], C[5] } -> sum A C, terms = 1 .. 8; op 4: op 2 as a rolled loop, terms = 1 .. 64.
 * terms = 0 for ops 0 and 1.  Any other op / length, or buffer sizes that do not match the shape: VGPU_ERR_INVALID_ARG. */
int32_t vgpu_lazy_probe(vgpu_prover_t* p, uint32_t op, uint32_t terms, const uint32_t* operands, uint64_t operand_words, uint64_t n_items, uint32_t* results, uint64_t result_words);

/* Test hook: poison the prover's HBM pool(vgpu_prover_trim's cache).  The pool clears nothing, so a recycled block holds the last contents of a
 * buffer of the same size — usually the previous identical call's correct answer, which hides a stage that reads what it has not written.
 * mode bit 0: every block the pool hands out, fresh or recycled, is filled with `word` first; bit 1: every block is filled at the moment it
 * returns to the cache (a block released inside a fork/join section: at the join); 0 switches the hook off (the default; the only cost is
 * then one branch per pool operation).  Each fill covers the whole rounded block and is synchronous: the device drains, hipMemsetD32, the device
 * drains again — for tests, not for timed runs.  Takes effect with the next pool operation; VGPU_ERR_INVALID_ARG while a proof or an audit
 * owns the context.  The library reads no environment variable for it (the Python binding reads VGPU_POOL_POISON when a Prover is created). */
int32_t vgpu_prover_set_pool_poison(vgpu_prover_t* p, uint32_t mode, uint32_t word);
/* Test hook: out = {blocks, bytes filled on allocation, blocks, bytes filled on release} since the context was created. */
void vgpu_prover_pool_poison_stats(const vgpu_prover_t* p, uint64_t out[4]);
/* Test hook, the positive control of the one above: takes a block of `bytes` bytes from the pool exactly as a stage would, downloads its first
 * n_words words to out[0 .. n_words) and the LAST word of the rounded block to out[n_words], and releases it — a "stage" that reads before it
 * writes, so under poison it must see the word.  out has room for n_words + 1 words; bytes >= 1 and 4 * n_words <= bytes (else
 * VGPU_ERR_INVALID_ARG). */
int32_t vgpu_prover_pool_peek(vgpu_prover_t* p, uint64_t bytes, uint32_t* out, uint64_t n_words);
/* Test hook: with on != 0 every chunk of vgpu_verify_batch first fills the verifier's whole device buffer (which it keeps and reuses across
 * chunks and batches) with `word`, by a memset on the verifier's stream in front of the chunk's copies. */
int32_t vgpu_verifier_set_poison(vgpu_verifier_t* v, uint32_t on, uint32_t word);

/* Machine::prove (basic/src/lib.rs:147-675).  main[i] = trace of chip i; preprocessed traces are given
 * with their chip indices in chip order (BasicMachine: program, range).
 * debug_flags: 1 = keep the per-chip intermediate matrices (vgpu_proof_debug_*); 2 = run check_constraints and
 * check_cumulative_sums on the device before committing, as debug builds of the reference do (basic/src/lib.rs:270-375):
 * a violated constraint fails the call with VGPU_ERR_INVALID_ARG and a message naming chip, constraint and row.
 * The traces may belong to ANOTHER prover context of the same device (a host that uploads or generates segment i+1 on a context of its
 * own while this one proves segment i): the call first waits for that context's queued work and keeps it alive until the proof is done.
 * A context runs one proof at a time; calls from several threads (and the workers of several vgpu_prove_async tickets) QUEUE on it and are
 * served one after the other, as several threads may call prove on the reference's `Machine: Sync` (machine/src/machine.rs:13).
 * The commitment to the preprocessed traces (basic/src/lib.rs:189-201) is recomputed in every call, as in the reference; see
 * vgpu_prover_set_prep_cache for hosts that prove many segments of one program. */
int32_t vgpu_prove(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips,
                   const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t debug_flags, vgpu_proof_t** out);
/* The same, asynchronously: returns at once, a host thread of its own drives this prover's streams.  Two provers on one
 * GPU, each with one ticket outstanding, keep two proofs in flight from a single caller thread (independent segments:
 * one proof's latency-bound Merkle-top / FRI chain overlaps the other's commits).  The traces must outlive the wait. */
typedef struct vgpu_ticket vgpu_ticket_t;
int32_t vgpu_prove_async(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips,
                         const vgpu_trace_t* const* prep, uint32_t n_prep, vgpu_ticket_t** out);
int32_t vgpu_ticket_wait(vgpu_ticket_t* t, vgpu_proof_t** out);   /* consumes the ticket */
/* CBOR image of the proof (ciborium over the serde-derived MachineProof, basic/src/bin/valida.rs:425-427; field names of
 * machine/src/proof.rs:13-44 and, for the PCS proof, SURVEY.md Appendix B12 — unpinned).  flags: VGPU_CBOR_*.  Returns the
 * length in bytes (copying when out has room) or a negative status. */
#define VGPU_CBOR_CANONICAL_FIELDS 1u  /* BabyBear as canonical u32 instead of the derived {"value": <Montgomery word>} */
#define VGPU_CBOR_PLAIN_DIGESTS 2u     /* commitments as [Val; 8] instead of Hash { value, _marker } */
int64_t vgpu_proof_cbor(const uint32_t* proof_words, uint64_t n_words, uint32_t flags, uint8_t* out, uint64_t cap_bytes);
/* The way back (ciborium::from_reader on the verifier's side; the reference's tests verify a proof after exactly this round trip,
 * basic/tests/test_prover.rs:456-469): CBOR image -> proof words.  Accepts either setting of the two switches per value.  Returns the word
 * count (copies when out has room), or a negative status with the reason in vgpu_last_error. */
int64_t vgpu_proof_from_cbor(const uint8_t* bytes, uint64_t n_bytes, uint32_t* out, uint64_t cap_words);
/* The same for a first contact with a proof file of the real `valida prove` (every encoding convention of the absent crates is recall):
 * flags & VGPU_CBOR_IN_BARE_IS_MONTGOMERY reads a BARE integer field element as the raw Montgomery word instead of the canonical value;
 * *forms_seen (may be null) reports what the image contained: VGPU_CBOR_SAW_* bits. */
#define VGPU_CBOR_IN_BARE_IS_MONTGOMERY 1u
#define VGPU_CBOR_SAW_FIELD_STRUCT 1u    /* {"value": m} */
#define VGPU_CBOR_SAW_FIELD_BARE 2u
#define VGPU_CBOR_SAW_DIGEST_STRUCT 4u   /* Hash { value, _marker } */
#define VGPU_CBOR_SAW_DIGEST_PLAIN 8u
int64_t vgpu_proof_from_cbor_ex(const uint8_t* bytes, uint64_t n_bytes, uint32_t flags, uint32_t* out, uint64_t cap_words, uint32_t* forms_seen);
uint64_t vgpu_proof_len(const vgpu_proof_t* pr);            /* u32 words of the flat "VPF1" encoding */
const uint32_t* vgpu_proof_words(const vgpu_proof_t* pr);
/* 11 doubles, ms: ingest, commit_main, perm, commit_perm, quotient, commit_quotient, open_values, open_reduce, fri, queries, total */
void vgpu_proof_phase_ms(const vgpu_proof_t* pr, double out[11]);
/* transcript probe: 8 (preprocessed root) + 15 (perm challenges) + 5 (alpha) + 5 (zeta) words */
void vgpu_proof_transcript(const vgpu_proof_t* pr, uint32_t out[33]);
/* with debug_flags & 1: per-chip intermediate matrices, row-major canonical, natural row order */
int64_t vgpu_proof_debug_perm_trace(const vgpu_proof_t* pr, uint32_t chip, uint32_t* out, uint64_t cap_words);
int64_t vgpu_proof_debug_quotient(const vgpu_proof_t* pr, uint32_t chip, uint32_t* out, uint64_t cap_words);
void vgpu_proof_free(vgpu_proof_t* pr);

/* ---- Bus audit: WHICH LogUp tuples of a witness are unbalanced — the exact, challenge-free statement of which check_cumulative_sums
 * (basic/src/lib.rs:373-375, the debug_flags & 2 path of vgpu_prove) is the randomised form.  Inputs: exactly what vgpu_prove takes.
 *   record    one (chip, row, interaction) of Chip::all_interactions order (machine/src/chip.rs:40-63) whose count column is non-zero on that row;
 *             its tuple = the interaction's fields on the row (canonical), its bus = (is_global, bus_index).
 *   same tuple  two records of one bus whose field lists are equal after ZERO-PADDING to the widest interaction of that bus: the permutation
 *             argument reduces a tuple as sum_j f_j beta^j (machine/src/chip.rs:121-208), so a trailing zero field is invisible to it
 *             (BasicMachine: the cpu chip sends 14 fields on the general bus, every ALU chip receives 13).
 *   net       sum of the counts of a tuple's send records minus that of its receive records, in F_p; unbalanced: net != 0.
 *   order     records ascend by (chip, row, interaction); the report lists the tuples by their first record and, under each, its first
 *             max_records_per_tuple records.  The report is exact (no hash decides it) and the same words run after run.
 * Options: a zero field selects its default — max_tuples 64, max_records_per_tuple 4, hash_bits 64; opts may be NULL.  hash_bits is a test
 * hook: the device's grouping key is cut to that many bits (1..64; more is refused), collisions become common, the report must not change.
 * vgpu_bus_audit runs on the device (kernels/bus_audit.hip), queued on the prover context like a proof; scratch comes from the prover's pool:
 * 60 bytes per (row, interaction) pair of the machine (live or not), 24 more per unbalanced tuple, plus the working-layout copy of every
 * uploaded (not device-generated) trace; VGPU_ERR_OOM with a message when the pool cannot give them, VGPU_ERR_INVALID_ARG for more than
 * 2^32 - 2 pairs.  vgpu_bus_audit_host is the same contract on the host over canonical row-major matrices (one thread, no device): for small
 * programs on a box without a GPU.  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_bus_report_words, u32 words; u64 values as lo, hi):
 *   [0] 0x31524256 "VBR1" [1] word count [2] balanced [3] truncated [4,5] total_unbalanced (exact even when the list is cut) [6] reported [7] n_buses
 *   per bus, ascending (is_global, bus_index), 12 words: is_global, bus_index, width, 0, live records, send records, receive records, unbalanced tuples (u64 each)
 *   per reported tuple: is_global, bus_index, width, net, send sum, receive sum (canonical), send records, receive records (u64 each), n_listed,
 *                       width fields (padded), n_listed x (chip, row, interaction, is_send, count). */
typedef struct vgpu_bus_audit_opts { uint64_t max_tuples; uint32_t max_records_per_tuple; uint32_t hash_bits; } vgpu_bus_audit_opts_t;
typedef struct vgpu_bus_report vgpu_bus_report_t;
int32_t vgpu_bus_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                       uint32_t n_prep, const vgpu_bus_audit_opts_t* opts, vgpu_bus_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_bus_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                            const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                            const vgpu_bus_audit_opts_t* opts, vgpu_bus_report_t** out);
uint64_t vgpu_bus_report_len(const vgpu_bus_report_t* r);
const uint32_t* vgpu_bus_report_words(const vgpu_bus_report_t* r);
/* out[0]: the device pass (events around it on the prover's stream; 0 for the host audit), out[1]: wall time of the whole call; milliseconds */
void vgpu_bus_report_timing(const vgpu_bus_report_t* r, double out[2]);
void vgpu_bus_report_free(vgpu_bus_report_t* r);

/* ---- Constraint audit: WHICH AIR constraints of a witness fail, on which rows, with which value — check_constraints
 * (machine/src/check_constraints.rs:14-84, called per chip from basic/src/lib.rs:270-277; the debug_flags & 2 path of vgpu_prove reports one
 * (row, constraint) of the first failing chip) made exact and complete.  Inputs: exactly what vgpu_prove and vgpu_bus_audit take.
 *   domain      the trace itself: row r of chip c of height n has next = (r + 1) mod n; is_first_row = [r == 0], is_last_row = [r == n - 1],
 *               is_transition = [r != n - 1], as 0/1 field values (check_constraints.rs:37, :69-79).
 *   constraint  k of a chip = the k-th assert_zero of its Air::eval, in call order (for a vgpu_air_* captured AIR: the k-th vgpu_air_assert_zero);
 *               it fails on row r when its value there is non-zero.  Only Air::eval is audited: the three permutation / running-sum constraints
 *               depend on sampled challenges, and their exact statement is the bus audit above.
 *   order       entries ascend by (chip, constraint); under each, its first max_rows_per_constraint failing rows in ascending row order, each
 *               with the canonical value of the constraint polynomial on that row.  Only the first max_constraints failing (chip, constraint)
 *               pairs are listed; the totals stay exact and `truncated` says the list was cut.  No challenge enters: the report is exact and the
 *               same words run after run, for Machine.basic (compiled chip templates) and for captured AIRs (the interpreted program) alike.
 * Options: a zero field selects its default — max_constraints 64, max_rows_per_constraint 4 (at most 2^24 and 4096); opts may be NULL;
 * reserved != 0 is refused.
 * vgpu_constraint_audit runs on the device (kernels/constraint_audit.hip), queued on the prover context like a proof or a bus audit; it accepts
 * device-generated and uploaded traces, and traces of another context of the same device.  Chips without constraints are not read.  Scratch
 * comes from the prover's pool: 8 bytes per (constraint, workgroup of T rows) of every chip with constraints, i.e. at most 8 K / T bytes per
 * row (K <= 96 constraints, T = 256 rows, down to 64 for a captured AIR with a large register file: 3 to 12 bytes per row), 8 (K + 1) per chip,
 * 8 bytes per (constraint, listed row slot) of a failing chip, plus the working-layout copy of every uploaded (not device-generated) trace;
 * VGPU_ERR_OOM with a message when the pool cannot give them; VGPU_ERR_INVALID_ARG for bad shapes and for a chip of more than 96 constraints.
 * vgpu_constraint_audit_host is the same contract on the host over canonical row-major matrices (one thread, no device, any number of
 * constraints).  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_constraint_report_words, u32 words; u64 values as lo, hi):
 *   [0] 0x31524356 "VCR1" [1] word count [2] satisfied [3] truncated [4,5] total_failing = failing (chip, constraint) pairs (exact even when
 *   the list is cut) [6] reported [7] n_chips
 *   per chip, in machine order, 6 words: constraints, failing constraints, height (u64), rows failing at least one constraint (u64)
 *   per reported constraint: chip, constraint, failing rows (u64), n_listed, then n_listed x (row, value). */
typedef struct vgpu_constraint_audit_opts { uint64_t max_constraints; uint32_t max_rows_per_constraint; uint32_t reserved; } vgpu_constraint_audit_opts_t;
typedef struct vgpu_constraint_report vgpu_constraint_report_t;
int32_t vgpu_constraint_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                              uint32_t n_prep, const vgpu_constraint_audit_opts_t* opts, vgpu_constraint_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_constraint_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                   const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                   const vgpu_constraint_audit_opts_t* opts, vgpu_constraint_report_t** out);
uint64_t vgpu_constraint_report_len(const vgpu_constraint_report_t* r);
const uint32_t* vgpu_constraint_report_words(const vgpu_constraint_report_t* r);
/* out[0]: the device pass (events around it on the prover's stream, after the working-layout copies of uploaded traces; 0 for the host audit),
 * out[1]: wall time of the whole call; milliseconds */
void vgpu_constraint_report_timing(const vgpu_constraint_report_t* r, double out[2]);
void vgpu_constraint_report_free(vgpu_constraint_report_t* r);

/* ---- Mutation audit: WHICH cells of a witness could be changed without any AIR constraint or bus noticing — mutation testing of the AIRs, the
 * converse of the two audits above (they are only as strong as the AIRs they evaluate).  Inputs: exactly what vgpu_prove and the audits take.
 *   mutation      chip h with main matrix M (height n, width w), a row r, a main column c and a delta d: M' = M except M'[r][c] = M[r][c] + d
 *                 mod p.  Preprocessed columns are never mutated.
 *   AIR-detected  Air::eval of the chip on M' at rows r and (r - 1) mod n, over the constraint audit's domain (next = (row + 1) mod n,
 *                 is_first_row / is_last_row / is_transition as 0/1 values): some constraint is non-zero there that was zero at the same row
 *                 on M (a NEWLY failing constraint, so a witness that already fails can be audited).  For n = 1 the two rows are one row and
 *                 the mutated cell is seen as `local` and as `next` in one evaluation.  The permutation constraints are not evaluated: the bus
 *                 rule is their exact statement.
 *   bus-detected  every interaction of the chip on row r, in Chip::all_interactions order, for M and for M': an interaction with count 0 is no
 *                 record, otherwise the record is (count, fields), all canonical; detected when the record of some interaction differs.
 *   counts        per (chip, column, delta index), exact over all n rows: `air` rows that are AIR-detected, `bus` rows that are bus-detected,
 *                 `free` rows that are neither.  A column is UNBOUND when free = n for every delta.
 *   order         an entry is a (chip, column, delta index) with free > 0; entries ascend by (chip, column, delta index), each with its first
 *                 max_rows_per_entry free rows in ascending order.  Only the first max_entries entries are listed; the totals stay exact and
 *                 `truncated` says the list was cut.  No challenge, no hash and no floating point enter: the same words run after run, for
 *                 Machine.basic (compiled chip templates) and for captured AIRs (the interpreted program) alike.
 * The report is a statement about single-cell slack on THIS witness; it is not a soundness proof (a bound cell may be bound only on the rows
 * this witness has; slack of two cells of one row changed together is the pair audit's subject, below).
 * Options: a zero field selects its default — max_entries 1024, max_rows_per_entry 4 (at most 2^24 and 4096), n_deltas 0 = the pair {1, p - 1};
 * otherwise deltas[0 .. n_deltas) are 1 to 4 distinct canonical values in 1..p-1; opts may be NULL; reserved != 0 is refused.
 * vgpu_mutation_audit runs on the device (kernels/mutation_audit.hip), queued on the prover context like a proof or the other audits; it accepts
 * device-generated and uploaded traces.  Scratch comes from the prover's pool: 4 bytes per (column, delta, workgroup of T rows) twice (table and
 * prefix), i.e. at most 8 w D / T bytes per row (T = 256 rows, less for a captured AIR with a large register file), 24 w D bytes of totals and
 * 12 w of column flags per chip, 4 w D max_rows_per_entry bytes of listed rows for the widest chip, plus the working-layout copy of every
 * uploaded (not device-generated) trace; VGPU_ERR_OOM with a message when the pool cannot give them; VGPU_ERR_INVALID_ARG for bad shapes, for
 * a chip of more than 96 constraints and for one whose row tile (its columns and program registers) does not fit 160 KB of LDS at 64 rows.
 * vgpu_mutation_audit_host is the same contract on the host over canonical row-major matrices (one thread, no device, any number of
 * constraints).  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_mutation_report_words, u32 words; u64 values as lo, hi):
 *   [0] 0x31524d56 "VMR1" [1] word count [2] n_deltas D [3] truncated [4,5] total_entries = (chip, column, delta) with free > 0 (exact even when
 *   the list is cut) [6] reported [7] n_chips [8..11] the deltas (canonical; unused slots 0)
 *   per chip, in machine order, 6 + 6 D words: width, constraints, height (u64), unbound columns, 0, then per delta the sums over the chip's
 *   columns of free, air, bus (u64 each)
 *   per reported entry: chip, column, delta index, n_listed, free, air, bus (u64 each), then n_listed rows. */
typedef struct vgpu_mutation_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t n_deltas;
    uint32_t deltas[4];
    uint32_t reserved[2];
} vgpu_mutation_audit_opts_t;
typedef struct vgpu_mutation_report vgpu_mutation_report_t;
int32_t vgpu_mutation_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                            uint32_t n_prep, const vgpu_mutation_audit_opts_t* opts, vgpu_mutation_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_mutation_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                 const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                 const vgpu_mutation_audit_opts_t* opts, vgpu_mutation_report_t** out);
uint64_t vgpu_mutation_report_len(const vgpu_mutation_report_t* r);
const uint32_t* vgpu_mutation_report_words(const vgpu_mutation_report_t* r);
/* out[0]: the device pass (events around it on the prover's stream, after the working-layout copies of uploaded traces; 0 for the host audit),
 * out[1]: wall time of the whole call; milliseconds.  out[2]: the Air::eval row evaluations the audit performed (baselines included) */
void vgpu_mutation_report_timing(const vgpu_mutation_report_t* r, double out[3]);
void vgpu_mutation_report_free(vgpu_mutation_report_t* r);

/* ---- Pair audit: WHICH TWO cells of one row could be changed together without any AIR constraint or bus noticing although changing one of them
 * alone is noticed — the next order of slack after the mutation audit (a column that `a + b - c = 0` or a bus field `a + b` mentions looks bound
 * to single mutations; a prover can still move a by +1 and b by -1).  Inputs: exactly what vgpu_prove and the audits take.
 *   pair mutation  chip h with main matrix M (height n, width w), a row r, two main columns c1 < c2 and a delta pair q = i D + j over the
 *                  option's deltas: M'' = M except M''[r][c1] = M[r][c1] + d_i and M''[r][c2] = M[r][c2] + d_j mod p.  Both cells are on the
 *                  same row.  Preprocessed columns are never mutated.
 *   detected       exactly the mutation audit's two rules applied to M'': AIR-detected when a constraint is non-zero at row r or (r - 1) mod n
 *                  that was zero at that same row on M (for n = 1 one evaluation, both cells seen as local and as next); bus-detected when the
 *                  record of some interaction of row r differs (count 0 is no record).
 *   counts         per (chip, c1, c2, q), exact over all n rows: `free` rows where the pair mutation is neither AIR- nor bus-detected;
 *                  `compensated` rows that are free although at least one of the single mutations (r, c1, d_i), (r, c2, d_j) is detected by
 *                  the mutation audit's rules.  Compensated rows are the finding; the other free rows are already in the mutation report.
 *   coupled        a pair is coupled when some constraint of the chip's Program reads both columns in any role, or some single interaction's
 *                  virtual columns (count or fields) reference both, or n = 1.  For an uncoupled pair the detectors of the pair mutation are
 *                  the union of the two singles' detectors, so compensated = 0 and free = the rows where both singles are free: both passes
 *                  skip uncoupled pairs.  The report never depends on a shortcut or on a tuning knob.
 *   order          an entry is a (chip, c1, c2, q) with compensated > 0; entries ascend by (chip, c1, c2, q), each with its first
 *                  max_rows_per_entry compensated rows in ascending order.  Only the first max_entries entries are listed; the totals stay
 *                  exact and `truncated` says the list was cut.  No challenge, no hash and no floating point enter: the same words run after
 *                  run, from device and host, for Machine.basic and for captured AIRs.
 * What it is not: it covers same-row pairs only; cross-row pairs and triples are not looked for; it is a statement about THIS witness, not a
 * soundness proof; `check`'s exit status never depends on it.
 * Options: a zero field selects its default — max_entries 1024, max_rows_per_entry 4 (at most 2^24 and 4096), n_deltas 0 = the pair {1, p - 1},
 * otherwise deltas[0 .. n_deltas) are 1 to 4 distinct canonical values in 1..p-1 (the mutation audit's limits); chip_mask bit h = audit chip h,
 * 0 = all chips (a bit beyond the machine's chips is refused); unselected chips keep their block with audited = 0 and zero counts; opts may
 * be NULL; reserved != 0 is refused.
 * vgpu_pair_audit runs on the device (kernels/pair_audit.hip), queued on the prover context like a proof or the other audits; it accepts
 * device-generated and uploaded traces.  Scratch comes from the prover's pool, with E = coupled pairs x D^2 entries per chip: 16 E + 256 bytes
 * of totals, 8 E bytes of bus masks and 4 bytes per pair, 8 E bytes per workgroup of T rows (table and prefix; T = 256 rows, less for a chip
 * whose tile is large), 4 max_rows_per_entry bytes per entry up to the last listed one of the chip with the most, plus the working-layout copy
 * of every uploaded trace; VGPU_ERR_OOM with a message when the pool cannot give them (chip_mask audits fewer chips at a time);
 * VGPU_ERR_INVALID_ARG for bad shapes, for a chip of more than 96 constraints, of more than 4096 columns, and for one whose row tile does not
 * fit 160 KB of LDS at 64 rows (about 620 columns).
 * vgpu_pair_audit_host is the same contract on the host over canonical row-major matrices (one thread, no device, no limits).  Both validate
 * shapes as vgpu_prove does.
 * Report image (vgpu_pair_report_words, u32 words; u64 values as lo, hi):
 *   [0] 0x31525056 "VPR1" [1] word count [2] n_deltas D [3] truncated [4,5] total_entries = (chip, c1, c2, q) with compensated > 0 (exact even
 *   when the list is cut) [6] reported [7] n_chips [8..11] the deltas (canonical; unused slots 0)
 *   per chip, in machine order, 8 + 4 D^2 words: width, constraints, interactions, audited (0 / 1), height (u64), coupled pairs, slack pairs
 *   (pairs with compensated > 0 for some q), then per q the sums over ALL the chip's pairs of free and compensated (u64 each; an uncoupled
 *   pair contributes its exact free and 0)
 *   per reported entry: chip, c1, c2, q, n_listed, 0, free, compensated (u64 each), then n_listed rows. */
typedef struct vgpu_pair_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t n_deltas;
    uint32_t deltas[4];
    uint32_t chip_mask;
    uint32_t reserved;
} vgpu_pair_audit_opts_t;
typedef struct vgpu_pair_report vgpu_pair_report_t;
int32_t vgpu_pair_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                        uint32_t n_prep, const vgpu_pair_audit_opts_t* opts, vgpu_pair_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_pair_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                             const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                             const vgpu_pair_audit_opts_t* opts, vgpu_pair_report_t** out);
uint64_t vgpu_pair_report_len(const vgpu_pair_report_t* r);
const uint32_t* vgpu_pair_report_words(const vgpu_pair_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: the Air::eval row evaluations the
 * audit performed (baselines and single mutations included) */
void vgpu_pair_report_timing(const vgpu_pair_report_t* r, double out[3]);
void vgpu_pair_report_free(vgpu_pair_report_t* r);

/* ---- Rank audit: every first-order degree of freedom of one trace row.  At row r of chip h, which directions in the space of the row's w main
 * cells leave every constraint and every bus record unchanged to first order?  That is the null space of the Jacobian of everything that reads
 * the row: its dimension counts the degrees of freedom, its zero columns are the cells free on their own, the rest is every compensated
 * combination of any arity and with any coefficients (pairs, triples, a + 256 b limb trades) — what a sweep over +-1 deltas never tries.  All bus
 * records are affine, and so are most constraints, so for them the answer is exact.  Inputs: exactly what vgpu_prove and the audits take.
 *   Jacobian       chip h with main matrix M (height n, width w) and a row r: J_r has w columns, one per main cell M[r][c] (preprocessed columns
 *                  are never varied).  Its rows: for every constraint k the partial derivatives dC_k / dM[r][c] of Air::eval at evaluation q = r,
 *                  where the cell is read as `local`, and the same at q = (r - 1) mod n, where it is read as `next`, on the constraint audit's
 *                  domain (next = (q + 1) mod n; is_first_row = [q = 0], is_last_row = [q = n - 1], is_transition = [q != n - 1] as 0 / 1).  For
 *                  n = 1 there is one evaluation, the cell local and next at once, the derivative the sum over both roles.  Derivatives are
 *                  taken at the witness as it is, whether or not the constraint holds there.  Permutation constraints are not evaluated; the
 *                  bus rows are their exact statement: for every interaction m (Chip::all_interactions order) one row holds the main-column
 *                  weights of its count and, when that count is non-zero at row r on M, one further row per field holds that field's
 *                  main-column weights.  A direction v in F_p^w is TANGENT-FREE iff J_r v = 0; for the bus part that is exact: the record of m
 *                  is unchanged along M[r] + t v for every t iff v is orthogonal to those rows.
 *   per row        from the reduced row echelon form R of J_r (unique, so no elimination order can change a word): rank rho, nullity
 *                  nu = w - rho, z = the zero columns of J_r.  The row is COUPLED when nu > z (a compensated direction that is not made of
 *                  single free cells).  Column c is PINNED iff e_c lies in the row space (c is a pivot column whose row of R has no other
 *                  non-zero entry), otherwise LOOSE (some tangent-free direction moves it); ZERO when column c of J_r is zero (a zero column is
 *                  loose); COUPLED at r when loose and not zero — the finding: the cell is bound alone and slack together.
 *   null vector    the canonical null vector of a loose column c: if c is a non-pivot column, the basis vector of c (v_c = 1, v_p = -R[row of
 *                  p][c] for every pivot column p, 0 on the other non-pivot columns); if c is a pivot column with row i, the basis vector of the
 *                  smallest non-pivot column f with R[i][f] != 0.
 *   order          an entry is a (chip, column) with a coupled row; entries ascend, each with its first max_rows_per_entry coupled rows in
 *                  ascending order.  Only the first max_entries entries are listed; the totals stay exact and `truncated` says the list was
 *                  cut.  No challenge, no hash and no floating point enter: the same words run after run, from device and host, for
 *                  Machine.basic and for captured AIRs.
 * What it is not: it is FIRST ORDER — for a constraint of degree >= 2 in the row's cells a tangent-free direction is necessary for a CURVE of
 * unnoticed changes and says nothing about a finite jump: b (b - 1) = 0 pins b here although b -> 1 - b passes it; x^2 = 0 at x = 0 reports x as
 * zero / loose although it is bound.  Finite flips stay the subject of the mutation and pair audits.  It covers the cells of one row only;
 * cross-row combinations are not looked for.  It is a statement about THIS witness, not a soundness proof; `check`'s exit status never depends on it.
 * Options: a zero field selects its default — max_entries 1024 (at most 2^24), max_rows_per_entry 4 (at most 4096); chip_mask bit h = audit chip
 * h, 0 = all chips (a bit beyond the machine's chips is refused); unselected chips keep their block with audited = 0 and zero counts; opts may be
 * NULL; reserved != 0 is refused.
 * vgpu_rank_audit runs on the device (kernels/rank_audit.hip: one wave per trace row, one lane per column, the elimination in LDS), queued on the
 * prover context like a proof or the other audits; it accepts device-generated and uploaded traces.  Scratch comes from the prover's pool: per
 * chip 32 + 16 w bytes of totals, 8 w bytes per workgroup of T rows (table and prefix; T = 1 to 64 rows), the interaction weight rows (4 w bytes
 * per count and field), 72 max_rows_per_entry bytes per column up to the last listed one of the chip with the most, plus the working-layout copy
 * of every uploaded trace; VGPU_ERR_OOM with the arithmetic in the message when the pool cannot give them (chip_mask audits fewer chips at a
 * time).  VGPU_ERR_INVALID_ARG for bad shapes, for a chip of more than 192 columns, and for a chip that does not fit 160 KB of LDS with one wave
 * per workgroup: 4 x (w (w | 1) [basis] + K w [the K constraints' raw Jacobian rows of one evaluation] + 128 registers [captured AIR under the
 * interpreting prover: (value, derivative) x 64 lanes per program register] + 10 w + 12 + 3 (w + preprocessed w) [tile of one row, halo, flags])
 * bytes <= 163840.  There is no fixed limit on the number of constraints: no fail mask is kept, K enters through that sum alone.
 * vgpu_rank_audit_host is the same contract on the host over canonical row-major matrices (a dual-number evaluation of the chip's Program, RREF
 * by row insertion; one thread, no device, no limits).  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_rank_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31525256 "VRR1" [1] word count [2] terms per listed row, always 8 [3] truncated [4,5] total_entries = (chip, column) with a coupled row
 *   (exact even when the list is cut) [6] reported [7] n_chips
 *   per chip, in machine order, 16 + 4 w words: width, constraints, interactions, audited (0 / 1), height (u64), sum over rows of nu (u64), sum
 *   over rows of z (u64), coupled rows (u64), max nullity, columns loose on some row, columns pinned on every row, columns coupled on some row,
 *   then per column c: loose rows (u64), zero rows (u64)
 *   per reported entry: chip, column, n_listed, 0, coupled rows (u64), then n_listed rows of 18 words: row, n_support (exact), then the first 8
 *   (column, coefficient) terms of the canonical null vector in ascending column order, unused slots 0. */
typedef struct vgpu_rank_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t reserved[2];
} vgpu_rank_audit_opts_t;
typedef struct vgpu_rank_report vgpu_rank_report_t;
int32_t vgpu_rank_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                        uint32_t n_prep, const vgpu_rank_audit_opts_t* opts, vgpu_rank_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_rank_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                             const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                             const vgpu_rank_audit_opts_t* opts, vgpu_rank_report_t** out);
uint64_t vgpu_rank_report_len(const vgpu_rank_report_t* r);
const uint32_t* vgpu_rank_report_words(const vgpu_rank_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: the dual row evaluations of the
 * contract, 2 w per row of a chip with constraints (w for n = 1); the device pass ends a row early once its rank is w */
void vgpu_rank_report_timing(const vgpu_rank_report_t* r, double out[3]);
void vgpu_rank_report_free(vgpu_rank_report_t* r);

/* ---- Field audit: which FIELDS of a chip's bus records its constraints leave undetermined.  The row audits above share one rule: a changed bus
 * record detects, so a cell that feeds a record counts as bound in every one of them.  That leaves them blind to a chip that receives
 * (opcode, a, b, c) and never ties c to a and b.  The field audit asks the rank audit's Jacobian per record field instead of per cell.  Inputs:
 * exactly what vgpu_prove and the audits take.  Chip h, main matrix M (height n, width w), row r; the rows are those of the rank audit's
 * Jacobian J_r (the same domain, the same n = 1 rule, derivatives at the witness as it is):
 *   C              the constraint rows dC_k / dM[r][c] at q = r and at q = (r - 1) mod n.
 *   psi_m          the main-column weights of the count of every interaction m, live or not.
 *   phi_{m,j}      the main-column weights of field j of interaction m; they exist only when m is LIVE at r: its count is non-zero on M.
 *   per field      of a live interaction m: the field is CONSTANT when phi_{m,j} = 0 (it reads only constants or preprocessed columns); a
 *                  constant field is never audited and never floats.  Otherwise S_{m,j} = C + {psi_*} + {phi_{m,i} : i != j}; the field is
 *                  DETERMINED at r iff phi_{m,j} lies in the row space of S_{m,j}, otherwise it FLOATS: there is a direction v in the row's
 *                  cells that leaves every constraint, every count and every other field of that record unchanged to first order and moves this
 *                  field.
 *   not held fixed the records of the chip's OTHER interactions, deliberately.  The same cell often also goes to the range bus (the output
 *                  bytes of add and sub) or to a sister record (cpu's channel values, shift's two records); holding that copy fixed would hide
 *                  exactly the holes this audit is for.
 *   direction      of a floating field: R = the reduced row echelon form of S_{m,j}, b_f = the null-space basis vector of non-pivot column f
 *                  (the rank audit's definition: 1 at f, -R[row of p][f] at every pivot column p), f the smallest with phi_{m,j} . b_f != 0,
 *                  v = b_f / (phi_{m,j} . b_f): S v = 0 and phi v = 1.  R is unique, so no elimination order changes a word.
 *   order          an entry is a (chip, interaction, field) with a floating row; entries ascend, each with its first max_rows_per_entry
 *                  floating rows in ascending order.  Only the first max_entries entries are listed; the totals stay exact and `truncated` says
 *                  the list was cut.  The same words run after run, from device and host, for Machine.basic and for captured AIRs.
 * What it is not: it is FIRST ORDER, on THIS witness, with the other rows' cells held fixed.  b (b - 1) = 0 pins b here (this is why add's
 * carries count as bound); x^2 = 0 at x = 0 makes x look free; a field determined only for y != 0 (z = x y, field x) floats on the rows where
 * y = 0.  A floating field on a SEND usually means "this chip delegates" (cpu's read values, shift's output): the finding is a field that also
 * floats on the receiving chip.  Inputs are not functions of outputs, so lt's operands are expected to float.  `check`'s exit status never
 * depends on this audit.
 * Options are exactly the rank audit's (vgpu_rank_audit_opts_t: max_entries, max_rows_per_entry, chip_mask, reserved), with the same defaults
 * and refusals; unselected chips keep their block with audited = 0 and zero counts.
 * vgpu_field_audit runs on the device (kernels/field_audit.hip: one wave per trace row, one lane per column, the base elimination of C and the
 * counts once per row in LDS, each live record's fields in a small quotient), queued on the prover context like a proof or the other audits; it
 * accepts device-generated and uploaded traces.  Scratch comes from the prover's pool: per chip 24 bytes + 8 per interaction and per field of
 * totals, 8 bytes per (field, workgroup of T rows; T = 1 to 64), the interaction weight rows (4 w bytes per count and field),
 * 72 max_rows_per_entry bytes per field up to the last listed one of the chip with the most, plus the working-layout copy of every uploaded
 * trace; VGPU_ERR_OOM with the arithmetic in the message when the pool cannot give them.  VGPU_ERR_INVALID_ARG for bad shapes, for a chip of
 * more than 192 columns, for an interaction of more than 32 fields, and for a chip that does not fit 160 KB of LDS with one wave per workgroup:
 * with F = the most fields of one interaction, 4 x (w (w | 1) [basis] + K w [raw Jacobian rows] + F ((w + F) | 1) [quotient] + 128 registers
 * [captured AIR under the interpreting prover] + 4 w + 3 F + 12 + 3 fields + 5 interactions + 3 (w + preprocessed w)) bytes <= 163840.
 * vgpu_field_audit_host is the same contract on the host over canonical row-major matrices (dual-number evaluation of the chip's Program, RREF
 * by row insertion, one elimination per field; one thread, no device, no limits).  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_field_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31414656 "VFA1" [1] word count [2] terms per listed row, always 8 [3] truncated [4,5] total_entries = (chip, interaction, field) with
 *   a floating row (exact even when the list is cut) [6] reported [7] n_chips
 *   per chip, in machine order: width, constraints, interactions, audited (0 / 1), height (u64), live records = sum over rows of live
 *   interactions (u64), floating fields = sum over rows and fields (u64), rows with at least one floating field (u64); then per interaction:
 *   is_send, bus kind (0 local, 1 global), bus index, n_fields, live rows (u64), then per field: constant (0 / 1), floating rows (u64)
 *   per reported entry: chip, interaction, field, n_listed, floating rows (u64), then n_listed rows of 18 words: row, n_support (exact), then
 *   the first 8 (column, coefficient) terms of the direction v in ascending column order, unused slots 0. */
typedef struct vgpu_field_report vgpu_field_report_t;
int32_t vgpu_field_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                         uint32_t n_prep, const vgpu_rank_audit_opts_t* opts, vgpu_field_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_field_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                              const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                              const vgpu_rank_audit_opts_t* opts, vgpu_field_report_t** out);
uint64_t vgpu_field_report_len(const vgpu_field_report_t* r);
const uint32_t* vgpu_field_report_words(const vgpu_field_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: the dual row evaluations: 2 w per
 * row of a chip with constraints and interactions (w for n = 1); the listing pass evaluates its listed rows again, uncounted */
void vgpu_field_report_timing(const vgpu_field_report_t* r, double out[3]);
void vgpu_field_report_free(vgpu_field_report_t* r);

/* ---- Link audit: the bus tuple fields that NO chip on the bus pins — the join the field audit leaves to the reader.  A floating field on a send
 * usually means that the chip delegates; the finding is a field that floats at every record carrying the tuple.  Inputs: exactly what vgpu_prove
 * and the other audits take.
 *   definitions    records, buses, "same tuple" (after zero-padding to the bus's widest interaction) and record order are the bus audit's, word
 *                  for word; float masks are the field audit's, word for word (the same Jacobian rows, the same n = 1 rule, the same constant
 *                  rule).  All chips are audited: there is no chip mask, because a join needs every end.
 *   record mask    of a live record of interaction m with nf fields on a bus of width W <= 32: bit j < nf is set iff field j floats at that row.
 *                  Bits nf .. W - 1 are clear: a padded position is the constant 0 and so is pinned.  Constant and determined fields are clear.
 *   tuple mask     the AND of the record masks of all the tuple's records, sends and receives alike.  Position j is OPEN in the tuple iff its
 *                  bit is set, otherwise it is ANCHORED; a tuple with a non-zero mask is an open tuple.  The audit ignores `net`: it runs on
 *                  balanced and unbalanced witnesses alike.
 *   per record     a field that floats at a record is OPEN there if its position is open in the record's tuple, otherwise it is ANSWERED: it
 *                  floats locally, and another record of the tuple pins it.
 *   order          open tuples ascend by their first record; each lists its first max_records_per_tuple records in record order.  Only the first
 *                  max_tuples open tuples are listed; the totals stay exact and `truncated` says the list was cut.  The same words run after run,
 *                  from device and host, for Machine.basic and for captured AIRs.
 * What it is not: it is FIRST ORDER, on THIS witness.  Each record is judged alone: the field audit deliberately does not hold sister records of
 * the same row fixed, so "open" means that no single record's own chip pins the position; a joint move may still be blocked by a sister
 * record.  "Anchored" is per tuple as it stands: a lookup bus whose receiver can move multiplicities between tuples is not modelled.  `check`'s
 * exit status never depends on this audit.
 * Options: max_tuples, max_records_per_tuple and hash_bits are the bus audit's (zeros select its defaults 64, 4 and 64; hash_bits is its test
 * hook with the same meaning and refusals: the report must not change under it); reserved must be zero.
 * VGPU_ERR_INVALID_ARG, host and device alike, for bad shapes and for a bus wider than 32 fields (the tuple mask is one word; the message
 * carries the arithmetic).  vgpu_link_audit runs on the device (kernels/link_audit.hip: the field audit's wave-per-row elimination writes one
 * mask word per record slot, the bus audit's records / sort / groups / reduce group the records, two streaming passes over the sorted records
 * AND the masks per tuple and tally them), queued on the prover context like a proof or the other audits; it accepts device-generated and
 * uploaded traces.  There the field audit's limits apply as well (192 columns, 32 fields per interaction, 160 KB of LDS with one wave per
 * workgroup: 4 x (w (w | 1) + K w + F ((w + F) | 1) + 128 registers + 4 w + 3 F + 12 + 4 interactions + 3 (w + preprocessed w)) bytes) and
 * the bus audit's of 2^32 - 2 (row, interaction) pairs.  Scratch comes from the prover's pool: 68 bytes per (row, interaction) pair (the bus
 * audit's 60, 4 for the record mask, 4 for the tuple mask), 16 per field and 528 per bus of tallies, the interaction weight rows, 24 bytes per
 * open tuple and the working-layout copy of every uploaded trace; VGPU_ERR_OOM with the arithmetic in the message when the pool cannot give them.
 * vgpu_link_audit_host is the same contract on the host over canonical row-major matrices (the host field audit's masks, the host bus audit's
 * records sorted by full padded tuple; one thread, no device, no limit beyond the 32-field bus).
 * Report image "VLA1" (vgpu_link_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31414C56 "VLA1" [1] word count [2] truncated [3,4] total open tuples (exact even when the list is cut) [5] reported [6] n_buses
 *   [7] n_chips
 *   per bus, ascending (is_global, bus_index): is_global, bus_index, width, live records (u64), tuples (u64), open tuples (u64), then per
 *   position j < width: tuples in which j is open (u64), records of those tuples (u64)
 *   per chip, in machine order: interactions, then per interaction: is_send, bus kind (0 local, 1 global), bus index, n_fields, live rows
 *   (u64), then per field: constant (0 / 1), floating rows (u64; the field audit's count for the same witness), open rows (u64)
 *   per reported open tuple: is_global, bus_index, width, tuple mask, send records (u64), receive records (u64), n_listed, the width padded
 *   fields, then n_listed x (chip, row, interaction, is_send, record mask). */
typedef struct vgpu_link_audit_opts { uint64_t max_tuples; uint32_t max_records_per_tuple; uint32_t hash_bits; uint32_t reserved; } vgpu_link_audit_opts_t;
typedef struct vgpu_link_report vgpu_link_report_t;
int32_t vgpu_link_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                        uint32_t n_prep, const vgpu_link_audit_opts_t* opts, vgpu_link_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_link_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                             const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                             const vgpu_link_audit_opts_t* opts, vgpu_link_report_t** out);
uint64_t vgpu_link_report_len(const vgpu_link_report_t* r);
const uint32_t* vgpu_link_report_words(const vgpu_link_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: the dual row evaluations of the
 * masks, counted as the field audit counts them */
void vgpu_link_report_timing(const vgpu_link_report_t* r, double out[3]);
void vgpu_link_report_free(vgpu_link_report_t* r);

/* ---- Step audit: finite steps along each row's null directions.  The rank audit ends at first order: a null vector of a row's Jacobian may be a
 * real trade (a + b - c, limb trades) or the artefact of a quadratic constraint at a degenerate point (x^2 = 0 at x = 0).  The step audit takes
 * the rank audit's canonical null vector v of every (row, loose column) and judges the finite moves M[r] + t v by the mutation audit's rule.
 * Inputs: exactly what vgpu_rank_audit takes.  Chip h, main matrix M (height n, width w), row r:
 *   directions   exactly the rank audit's: J_r, its RREF, loose / pinned / zero / coupled, the canonical null vector of each loose column; the
 *                vector of a ZERO loose column is e_c.  Several columns may share a vector; results are per column.
 *   move         loose column c with vector v, step index s, t = steps[s]: M' = M except M'[r][j] = M[r][j] + t v_j mod p for every j.
 *                Preprocessed columns never move.
 *   detected     the mutation audit's two rules on M'.  AIR: Air::eval at q = r and q = (r - 1) mod n on the constraint audit's domain; a
 *                constraint that is non-zero there and was zero on M detects; n = 1 is one evaluation with the row as local and next at once;
 *                permutation constraints are not evaluated.  Bus: a changed record detects — v annihilates the count row and, on live rows,
 *                every field row, so it never does; the host audit evaluates it all the same and counts it, the device pass writes 0.
 *   per cell     (row, loose column): pass mask, bit s = step s goes undetected.  EXACT: every step passes; CURVED: otherwise.
 *   per chip     max_degree (the machine's max constraint degree) and line_exact = [n_steps >= max_degree]: along the line every constraint is
 *                a polynomial in t of degree <= max_degree that is zero at t = 0 if it held; n_steps further zeros make it vanish
 *                identically, so no constraint that holds now fails anywhere on the line of an exact cell.
 * A listed exact row is a certificate: made on the trace, the move leaves vgpu_constraint_audit's and vgpu_bus_audit's reports as they were.
 * What it is not: one row, THIS witness, moves along the canonical vectors only (not the whole null space); line_exact is about constraints that
 * held; cross-row combinations are not looked for; `check`'s exit status never depends on it.
 * Options: max_entries, max_rows_per_entry, chip_mask as vgpu_rank_audit_opts_t, same defaults and refusals; n_steps and steps: 1 to 4 distinct
 * canonical values in 1..p-1, n_steps = 0 the default {1, p - 1, 2}; opts may be NULL; reserved != 0 is refused.
 * vgpu_step_audit runs on the device (kernels/step_audit.hip: one wave per trace row, the rank audit's dual evaluation and LDS elimination, then
 * ceil(nu S / 64) passes of plain evaluations, lane <-> (non-pivot column, step)), queued on the prover context; scratch from the pool: per chip
 * 48 + 32 w bytes of totals, 8 w bytes per workgroup of rows, the interaction weight rows, 80 max_rows_per_entry bytes per column up to the last
 * listed one; VGPU_ERR_OOM with the arithmetic when the pool cannot give them.  VGPU_ERR_INVALID_ARG for bad shapes, more than 192 columns, and a
 * chip that does not fit 160 KB of LDS with one wave per workgroup: the rank audit's sum plus 4 x (2 w + 24 + ceil(2 K / 32)) bytes (two more
 * per-column counters, the pass bits, the baseline bits).  vgpu_step_audit_host: the same contract on the host, one thread, no limits.
 * Report image (vgpu_step_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31525356 "VSR1" [1] word count [2] terms per listed row, always 8 [3] truncated [4,5] total_entries = (chip, column) with a
 *   coupled-and-exact or a curved row (exact even when the list is cut) [6] reported [7] n_chips [8] n_steps [9] 0 [10..13] steps, unused 0
 *   per chip, in machine order, 30 + 8 w words: width, constraints, interactions, audited (0 / 1), height (u64), max_degree, line_exact, then u64
 *   each: loose cells, zero cells, exact cells, coupled-and-exact cells (sums over rows and columns), confirmed rows (a coupled-and-exact
 *   column), refuted rows (a curved column), passes of step 0..3 ((row, loose column) cells), bus-detected (0); then per column c, u64 each:
 *   loose rows, zero rows, exact rows, coupled-and-exact rows
 *   per reported entry (ascending (chip, column)): chip, column, n_listed, 0, coupled-and-exact rows (u64), curved rows (u64), then n_listed rows
 *   of 20 words — the first max_rows_per_entry rows, ascending, where the column is loose and (not zero, or curved); zero-and-exact rows (the
 *   mutation audit's free cells) are counted and never listed: row, pass mask, zero (0 / 1), n_support (exact), then the first 8 (column,
 *   coefficient) terms of the vector in ascending column order, unused slots 0. */
typedef struct vgpu_step_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t n_steps;
    uint32_t steps[4];
    uint32_t reserved[3];
} vgpu_step_audit_opts_t;
typedef struct vgpu_step_report vgpu_step_report_t;
int32_t vgpu_step_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                        uint32_t n_prep, const vgpu_step_audit_opts_t* opts, vgpu_step_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_step_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                             const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                             const vgpu_step_audit_opts_t* opts, vgpu_step_report_t** out);
uint64_t vgpu_step_report_len(const vgpu_step_report_t* r);
const uint32_t* vgpu_step_report_words(const vgpu_step_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: row evaluations (the rank
 * audit's dual ones plus the plain ones of the moves) */
void vgpu_step_report_timing(const vgpu_step_report_t* r, double out[3]);
void vgpu_step_report_free(vgpu_step_report_t* r);

/* ---- Invariant audit: the affine-linear relations every row of a chip keeps.  The other audits ask what the constraints and bus records bind;
 * this one asks which relations the WITNESS keeps that nothing may be asking for, and on how many rows the chip's own constraints and records
 * enforce each of them to first order.  Inputs: exactly what vgpu_prove and the audits take.
 *   invariants   chip h, main matrix M (n x w): the augmented row a_r = (1, M[r][0], .., M[r][w - 1]); the invariants are the l in F_p^(w + 1)
 *                with l . a_r = 0 for every r.  R = the reduced row echelon form of the n x (w + 1) matrix of the a_r, columns in that order
 *                (unique: no elimination order, grid or row order changes a word; column 0 is always a pivot); rho_A = rank, d = w + 1 - rho_A.
 *   basis        one invariant per non-pivot main column f: l_f = 1, l_p = -R[row of p][f] for every pivot column p (only pivots left of f
 *                occur), 0 elsewhere: "column f is this affine function of earlier columns".  CONSTANT (kind 0) when no main column other
 *                than f has a non-zero coefficient (M[r][f] = -l_0 on every row), otherwise a RELATION (kind 1).
 *   enforcement  c = (l_1 .. l_w) against the rank audit's Jacobian J_r (the same matrix, word for word; n = 1 by its rule): l is ENFORCED at
 *                row r iff c lies in the row space of J_r, otherwise FREE at r: some first-order-unnoticed move of the row's cells breaks the
 *                relation.  Each invariant is judged against J_r alone, never against J_r plus other invariants.
 * What it is not: affine-linear relations only (b (b - 1) = 0 is not found); one row (relations between a row and its successor are not looked
 * for); THIS witness (a short program has accidental relations); the verdict is per basis vector (a sum of two free invariants can be
 * enforced); enforcement is first order, with the rank audit's caveats; `check`'s exit status never depends on it.
 * Options: max_entries, max_rows_per_entry, chip_mask as vgpu_rank_audit_opts_t, same defaults and refusals; max_terms: (column, coefficient)
 * terms listed per invariant, 0 the default 8, at most 4096; opts may be NULL; reserved != 0 is refused.
 * vgpu_invariant_audit runs on the device (kernels/invariant_audit.hip), queued on the prover context.  Phase 1: a streaming exact elimination of
 * the augmented rows, one wave per slice of rows with its reduced basis in LDS, at most 2048 workgroups per chip, then a tree of fan 16 that
 * eliminates the workgroups' bases into the one RREF and writes the d canonical vectors.  Phase 2 (skipped when d = 0): one wave per trace row, the rank
 * audit's dual evaluation and LDS elimination, then one reduce-only sweep per invariant; free rows are counted per workgroup and listed by
 * count -> scan -> list, no atomic admits a row.  Scratch from the pool: per chip (w + 1) (w + 2) words per phase-1 workgroup and a sixteenth of that again for the tree (64 MB at
 * most), (w + 1)^2 + 2 words of merged basis, 8 d bytes of totals, 8 d bytes per workgroup of rows, the interaction weight rows, 4 max_rows_per_entry bytes per listed
 * invariant; VGPU_ERR_OOM with a message when the pool cannot give them.  VGPU_ERR_INVALID_ARG with the chip's name and the arithmetic for a chip
 * whose phase 1 (4 x ((w + 1) ((w + 1) | 1) + 3 (w + 1) + 32 ((w + 1) | 1) + 8) bytes: w <= 184) or phase 2 (the rank audit's sum with its
 * 4 x 6 w bytes of counters replaced by 4 x (w^2 + 4 w) bytes for the invariants and theirs when that is more, d = w counted) does not fit 160 KB
 * of LDS with one wave per workgroup; one lane per augmented column, three words per lane, would allow 191 columns.
 * vgpu_invariant_audit_host: the same contract on the host, one thread, no limits.
 * Report image (vgpu_invariant_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31524956 "VIR1" [1] word count [2] max_terms [3] truncated [4,5] total_entries = the sum of d over the audited chips (exact even when
 *   the list is cut) [6] reported [7] n_chips
 *   per chip, in machine order, 14 words: width, constraints, interactions, audited (0 / 1), height (u64), rho_A, d, constant columns, relations,
 *   invariants enforced on every row, on some rows, on no row, 0.  A chip that is not audited keeps its first six words, the rest 0.
 *   per entry, ascending (chip, column f), 12 + 2 T + L words: chip, column f, kind, l_0, support (main columns with a non-zero coefficient, f
 *   included; exact), T = listed terms = min(support, max_terms), L = listed free rows = min(free_rows, max_rows_per_entry), 0, enforced_rows
 *   (u64), free_rows (u64), then T (column, coefficient) terms ascending by column, then the first L free rows, ascending. */
typedef struct vgpu_invariant_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t max_terms;
    uint32_t reserved[3];
} vgpu_invariant_audit_opts_t;
typedef struct vgpu_invariant_report vgpu_invariant_report_t;
int32_t vgpu_invariant_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                             uint32_t n_prep, const vgpu_invariant_audit_opts_t* opts, vgpu_invariant_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_invariant_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                  const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                  const vgpu_invariant_audit_opts_t* opts, vgpu_invariant_report_t** out);
uint64_t vgpu_invariant_report_len(const vgpu_invariant_report_t* r);
const uint32_t* vgpu_invariant_report_words(const vgpu_invariant_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: dual row evaluations of phase 2 */
void vgpu_invariant_report_timing(const vgpu_invariant_report_t* r, double out[3]);
void vgpu_invariant_report_free(vgpu_invariant_report_t* r);

/* ---- Transition audit: the invariant audit over a two-row window and under a gate: the affine-linear relations between a row and its successor
 * that the WITNESS keeps on every window, or on every window where a boolean column holds one value, and the windows at which the chip's own
 * constraints and records hold each of them to first order.  Inputs: exactly what vgpu_prove and the audits take.
 *   windows      chip h, main matrix M (n x w): window r = 0 .. n - 2 (no wrap: the AIR's when_transition domain) is the row
 *                a_r = (1, M[r][0..w), M[r + 1][0..w)) of AW = 2 w + 1 WINDOW COLUMNS: 0 the constant, 1 + c `local` c, 1 + w + c `next` c.
 *                n = 1: no windows; the chip's block keeps its first six words, the rest 0.
 *   gates        window column j >= 1 is BOOLEAN when its values over all windows lie in {0, 1} and both occur.  Gate 0: every window; then for
 *                every boolean j ascending (j = 1), (j = 0).  max_gates cuts this list (gate 0 included); n_bool and n_gates stay exact.  A gate
 *                of fewer than min_gate_windows windows is listed but not audited; gate 0 always is.
 *   space        R_g = the reduced row echelon form of the a_r of the windows where g holds, columns in that order (unique: no grid, tree or
 *                row order changes a word); rho_g, d_g = AW - rho_g; pivots(g) is a subset of pivots(0).
 *   entries      the canonical vector of a non-pivot column f: l_f = 1, l_p = -R_g[row of p][f] for the pivots p (left of f), 0 elsewhere.  Gate 0
 *                lists every non-pivot f of the `next` block whose vector has a non-zero `local` coefficient (kind 2) and counts the others
 *                (local_only: the invariant audit's subject; next_only: the same relations shifted).  Gate g >= 1 lists every f in
 *                pivots(0) \ pivots(g) but the gate's own column.  kind 0: a constant (only l_0 and l_f), 1: one block, 2: both blocks.
 *   verdict      per window r of the entry's gate, J the rank audit's Jacobian (the same matrix, word for word): FREE at r iff l's `local` part
 *                is outside the row space of J_r or its `next` part outside that of J_{r + 1}, otherwise HELD at r.  One-sided: free is a
 *                certificate; held is exact for a chip none of whose constraints reads `next`, otherwise "no one-row move breaks it".
 * What it is not: affine-linear only; single gates (no conjunction of two gates); no joint 2 w-column Jacobian; THIS witness; per basis vector;
 * first order, with the rank audit's caveats; `check`'s exit status never depends on it.
 * Options: max_entries, max_rows_per_entry, chip_mask as vgpu_rank_audit_opts_t, same defaults and refusals (entries cut from the list are not
 * judged); max_terms: (window column, coefficient) terms listed per entry, 0 the default 8, at most 4096; min_gate_windows: 0 the default 64;
 * max_gates: 0 the default 256, at most 4096; opts may be NULL; reserved != 0 is refused.
 * vgpu_transition_audit runs on the device (kernels/transition_audit.hip), queued on the prover context: the column flags (ballots per wave, one
 * OR per workgroup), a streaming exact elimination of the gated windows (one wave per slice, gates over the grid's y, a tree of fan 16 to the one
 * RREF per gate), then per trace row the rank audit's dual evaluation and LDS elimination and up to two reduce-only sweeps per listed entry, one
 * bit per (entry, half, row); free windows are counted and listed by count -> scan -> list, no atomic admits a row.  VGPU_ERR_INVALID_ARG with
 * the chip's name and the arithmetic for a chip with 2 w + 1 > 184 or whose phase 2 does not fit 160 KB of LDS with one wave and one entry
 * staged; VGPU_ERR_OOM with the arithmetic when the pool cannot give the scratch.
 * vgpu_transition_audit_host: the same contract on the host, one thread, no limits.
 * Report image (vgpu_transition_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31525456 "VTR1" [1] word count [2] max_terms [3] truncated [4,5] total_entries (exact even when the list is cut) [6] reported
 *   [7] n_chips [8] gate blocks [9] min_gate_windows [10] max_gates [11] 0
 *   per chip, in machine order, 16 words: width, constraints, interactions, audited (0 / 1), height (u64), n_bool, n_gates = 1 + 2 n_bool, gates
 *   listed, gates audited, rho_0, d_0, local_only, next_only, transitions (the three split d_0), gated (entries of the gates >= 1).
 *   per listed gate, ascending (chip, position), 10 words: chip, window column (0: gate 0), value, audited, windows (u64), rho_g, d_g, entries
 *   of the gate (exact), 0.
 *   per entry, ascending (chip, gate, column f), 14 + 2 T + L words: chip, gate column, gate value, window column f, kind, l_0, support (window
 *   columns >= 1 with a non-zero coefficient, f included; exact), T = min(support, max_terms), L = min(free_windows, max_rows_per_entry), 0,
 *   free_windows (u64), held_windows (u64), then T (window column, coefficient) terms ascending, then the first L free windows, ascending. */
typedef struct vgpu_transition_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t max_terms;
    uint32_t min_gate_windows;
    uint32_t max_gates;
    uint32_t reserved[3];
} vgpu_transition_audit_opts_t;
typedef struct vgpu_transition_report vgpu_transition_report_t;
int32_t vgpu_transition_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                              uint32_t n_prep, const vgpu_transition_audit_opts_t* opts, vgpu_transition_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_transition_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                   const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                   const vgpu_transition_audit_opts_t* opts, vgpu_transition_report_t** out);
uint64_t vgpu_transition_report_len(const vgpu_transition_report_t* r);
const uint32_t* vgpu_transition_report_words(const vgpu_transition_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: dual row evaluations of phase 2 */
void vgpu_transition_report_timing(const vgpu_transition_report_t* r, double out[3]);
void vgpu_transition_report_free(vgpu_transition_report_t* r);

/* ---- Product audit: the products of two columns the witness keeps affine.  The invariant audit finds affine-linear relations only; the
 * constraints a chip consists of are mostly of degree two (b^2 = b, s t = 0, s t = s, s x = y, a b = c).  This audit lists, per chip, every
 * product of two independent columns that is an affine function of the row on every row of the WITNESS, and on how many rows the chip's own
 * constraints and records enforce it to first order.  Inputs: exactly what vgpu_prove and the audits take.
 *   space        chip h, main matrix M (n x w): a_r = (1, M[r][0], .., M[r][w - 1]); R = the reduced row echelon form of the a_r (the invariant
 *                audit's R, word for word), Pi its pivot columns (column 0 always), rho = |Pi|.  The q = rho - 1 pivot main columns are the
 *                INDEPENDENT columns.  A non-pivot column is an affine function of earlier ones (the invariant audit reports that) and takes
 *                no part.
 *   pairs        all (i, j), i <= j, both independent columns, in lexicographic order: m = q (q + 1) / 2.
 *   relation     pair (i, j) is a relation iff some beta in F_p^(w + 1), supported on Pi, has M[r][i] M[r][j] = beta . a_r on every row r.  The
 *                columns of Pi are linearly independent over the rows, so beta is unique: no grid, order or seed changes a word.
 *   kinds        0 BOOLEAN: i = j and beta = e_i.  1 ZERO: beta = 0.  2 SELECT: i != j and beta = e_i or beta = e_j (one column is 1 wherever
 *                the other is non-zero).  3 OTHER.
 *   verdict      the gradient of x_i x_j - beta . (1, x) at row r is g_r in F_p^w, g_r[k] = [k = i] M[r][j] + [k = j] M[r][i] - beta_(k + 1) (for
 *                i = j the first two terms add up to 2 M[r][i]).  ENFORCED at r iff g_r lies in the row space of the rank audit's Jacobian J_r
 *                (the same matrix, word for word; n = 1 by its rule).  FLAT iff g_r = 0: counted among the enforced rows and also on its own;
 *                first order says nothing there (x y = 0 at x = y = 0).  FREE otherwise: some first-order-unnoticed move of the row's cells
 *                breaks the relation.
 * What it is not: single products only (s a - s b = 0 is not found unless s a and s b are each affine); one row; THIS witness (a short program
 * has accidental relations); first order, with the rank audit's caveats; `check`'s exit status never depends on it.
 * Options: max_entries, max_rows_per_entry, chip_mask, max_terms, reserved as vgpu_invariant_audit_opts_t, same defaults and refusals.
 * vgpu_product_audit runs on the device (kernels/product_audit.hip), queued on the prover context.  (1) Pivots: the invariant audit's phase 1 and
 * merge.  (2) Basis rows: the rho rows that are not in the span of the rows before them, one wave per slice of rows eliminating over the rho
 * compacted columns and remembering the rows that raised the rank, then an ordered merge tree of fan 16 (the first-independent rows of L ++ R are
 * those of first-independent(L) ++ first-independent(R)): the same rows whatever the grid.  (3) Solve: the rho x rho matrix of the basis rows over
 * Pi inverted by Gauss-Jordan in one workgroup (in LDS when 8 rho^2 + 16 bytes fit, else in pool scratch), beta of every pair = inverse x
 * products at the basis rows.  (4) Sweep: per row and live pair M[r][i] M[r][j] == beta . a_r[Pi], a tile of 64 rows as [rho][64] and the beta of 32
 * pairs as [32][rho] in LDS, one thread per (row, pair), a mismatch stores 0 into the pair's flag; a first launch over the first 256 rows with all m
 * pairs, the survivors compacted, a second launch over all rows with the survivors.  (5) Enforce: one wave per trace row, the rank audit's dual
 * evaluation and LDS elimination once per row, then per relation g_r built from its sparse (column, coefficient) list (staged through LDS in
 * groups) and the row's two cells, one reduce-only sweep and the flat bit; free rows are counted per workgroup and listed by count -> scan ->
 * list, no atomic admits a row.  Scratch from the pool; VGPU_ERR_OOM with the arithmetic when the pool cannot give it.  VGPU_ERR_INVALID_ARG
 * with the chip's name and the arithmetic wherever the invariant audit would refuse the chip, and for a chip whose enforcement phase (the rank
 * audit's sum plus 4 x ((2 NW + 2) E + the entry group) bytes for E relations) does not fit 160 KB of LDS with one wave per workgroup.
 * vgpu_product_audit_host: the same contract on the host, one thread, no limits.
 * Report image (vgpu_product_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31525156 "VQR1" [1] word count [2] max_terms [3] truncated [4,5] total_entries = the relations of the audited chips (exact even when
 *   the list is cut) [6] reported [7] n_chips
 *   per chip, in machine order, 16 words: [0] width [1] constraints [2] interactions [3] audited (0 / 1) [4,5] height (u64) [6] rho [7] m (pairs)
 *   [8] relations [9] boolean [10] zero [11] select [12] other [13] relations enforced on every row [14] on some rows [15] on no row.  q is not
 *   stored: q = rho - 1 (0 for rho = 0), and the block has no padding.  A chip that is not audited keeps its first six words, the rest 0.
 *   per entry, ascending (chip, i, j), 16 + 2 T + L words: chip, i, j, kind, beta_0, support (main columns with a non-zero coefficient in beta;
 *   exact), T = listed terms = min(support, max_terms), L = listed free rows = min(free_rows, max_rows_per_entry), enforced_rows (u64), free_rows
 *   (u64), flat_rows (u64), 0, 0, then T (column, coefficient) terms ascending by column, then the first L free rows, ascending:
 *   M[r][i] M[r][j] = beta_0 + sum(coefficient * M[r][column]). */
typedef struct vgpu_product_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t max_terms;
    uint32_t reserved[3];
} vgpu_product_audit_opts_t;
typedef struct vgpu_product_report vgpu_product_report_t;
int32_t vgpu_product_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                           uint32_t n_prep, const vgpu_product_audit_opts_t* opts, vgpu_product_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_product_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                const vgpu_product_audit_opts_t* opts, vgpu_product_report_t** out);
uint64_t vgpu_product_report_len(const vgpu_product_report_t* r);
const uint32_t* vgpu_product_report_words(const vgpu_product_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: dual row evaluations of the
 * enforcement phase */
void vgpu_product_report_timing(const vgpu_product_report_t* r, double out[3]);
void vgpu_product_report_free(vgpu_product_report_t* r);

/* ---- Domain audit: the audits above judge a witness by local algebra.  A LOOKUP MEMBERSHIP ties a cell to a set ("this cell is a byte because
 * it is sent to the range bus"), and none of them sees a missing one.  Per chip and main column: which set of values does this witness put
 * there, and on which rows is a narrow column not a field of a live send to a lookup table.  Inputs: exactly what vgpu_prove and the audits take.
 *   vcol           (vgpu_vcol_t) constant + sum weight * cell (mod p) at row r, over main or preprocessed cells of row r.  A field or count is
 *                  BARE(c) iff it has one term, main, column c, weight 1, constant 0.  A record (chip, interaction, row) is LIVE iff its count
 *                  vcol != 0 at that row.
 *   column domain  per main column of every audited chip, over all n rows, canonical values: min, max, nonzero_rows, wide_rows (value >= 2^16),
 *                  distinct_narrow (the exact number of distinct values < 2^16), dense (1 iff wide_rows = 0 and distinct_narrow = max - min +
 *                  1), bits (the bit length of max), class 0 CONSTANT (min = max), 1 BOOLEAN (max <= 1, not constant), 2 BYTE (max < 2^8), 3
 *                  HALF (max < 2^16), 4 WIDE.  NARROW iff the class is BYTE or HALF and max < 2^max_bits.
 *   lookup buses   a TABLE CHIP has zero constraints, zero sends and at least one receive.  Bus (is_global, bus_index) is a LOOKUP BUS iff it
 *                  has a receive and every receive on it, machine-wide, belongs to a table chip: structural, independent of the witness
 *                  (lookup_auto = 1).  With lookup_auto = 0 bit bus_index of lookup_global_mask / lookup_local_mask decides; a machine with
 *                  a bus index >= 64 is refused then.  Buses are numbered in ascending (is_global, bus_index).
 *   appearances    an (interaction, field position) at which column c is bare; per appearance is_send, the bus, the position, live_rows.
 *                  Per column: guarded_rows (rows with at least one live bare SEND on a lookup bus), sent_rows (a live bare send on any other
 *                  bus), received_rows (a live bare receive), unguarded_rows = n - guarded_rows, unguarded_nonzero_rows (unguarded and the cell
 *                  != 0), mixed_rows (rows with a live send one of whose fields reads c without being bare(c)).
 *   entries        the narrow columns with unguarded_nonzero_rows > 0, ascending (chip, column), each with its appearances and its first
 *                  max_rows_per_entry unguarded non-zero rows, ascending, with their values; total_entries stays exact when the list is cut.
 *   bus positions  per bus, field position and direction, over the live records of the WHOLE machine (chip_mask does not narrow them): min,
 *                  max, distinct_narrow, wide_records, records and the bus's lookup flag: what a table actually offers.
 * What it is not: THIS witness only (a short program leaves columns accidentally narrow); only bare fields count as guards (a send of 256 a + b
 * guards neither column: see mixed_rows); values near p (small negatives) are WIDE; a guard says the cell is looked up, not that the table is
 * sound (the range chip's counter is an unconstrained main column, which the mutation audit reports); `check`'s exit status never depends on it.
 * Options: max_entries (default 1024, at most 2^24), max_rows_per_entry (default 4, at most 4096), chip_mask (0: all), max_bits (0: 16; above 16
 * refused), lookup_auto, the two masks, reserved (must be zero).  A null pointer gives the defaults.  In a struct max_entries, max_rows_per_entry
 * and lookup_auto are taken AS GIVEN (0 entries / 0 rows list nothing and keep every count exact; lookup_auto = 0 with zero masks names no lookup
 * bus): start from the defaults, not from a zeroed struct.
 * vgpu_domain_audit runs on the device (kernels/domain_audit.hip), queued on the prover context, wave64.  (1) k_da_scan: gridDim.y = the chip's
 * virtual columns (its main columns, then every (interaction, field) gated by its count), gridDim.x = at most 2048 slices of whole 256-row
 * tiles; a workgroup of 256 threads streams its slice (main columns are column-major: coalesced), reduces min / max / counts by wave shuffles
 * and LDS to one integer atomic of each kind, and sets values < 2^16 in an 8 KB LDS bitmap (a wave whose live lanes hold one value sets the
 * bit once), which it ORs into the column's 2048-word bitmap in device memory.  (2) k_da_classify: per bitmap the popcount, dense, bits, class,
 * narrow.  (3) k_da_guard: one thread per row walks the chip's appearance table (staged in LDS), counts per wave by ballots, per workgroup in
 * LDS, one add per workgroup; the unguarded non-zero rows of narrow columns are listed by count -> scan -> list, no atomic admits a row.  The
 * only atomics are integer OR, min, max and add: every word is the same run after run.  Scratch from the pool, zeroed by one memset;
 * VGPU_ERR_OOM with the arithmetic when the pool cannot give it.  vgpu_domain_audit_host: the same contract on the host, one thread, no limits.
 * Report image (vgpu_domain_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x314d4456 "VDM1" [1] word count [2] max_bits [3] truncated [4,5] total_entries (exact even when the list is cut) [6] reported
 *   [7] n_chips [8] lookup_auto [9] n_buses [10] n_positions [11] 0
 *   per chip, in machine order, 10 words: [0] width [1] constraints [2] interactions [3] audited (0 / 1) [4,5] height (u64) [6] is_table
 *   [7] narrow columns [8] entries [9] appearances; then `width` column records of 24 words: [0] min [1] max [2] distinct_narrow [3] class
 *   [4] dense [5] bits [6] narrow [7] appearances [8,9] nonzero_rows [10,11] wide_rows [12,13] guarded_rows [14,15] sent_rows [16,17]
 *   received_rows [18,19] unguarded_rows [20,21] unguarded_nonzero_rows [22,23] mixed_rows.  A chip that is not audited keeps words 0 .. 6 of
 *   its block; the rest and its column records are 0.
 *   per bus, ascending (is_global, bus_index), 4 words: is_global, bus_index, lookup, width (the most fields of an interaction on it)
 *   per bus, position and direction (sends, then receives), 12 words: [0] bus (its number in the list above) [1] position [2] is_send
 *   [3] lookup [4] min [5] max [6] distinct_narrow [7] 0 [8,9] wide_records [10,11] records; without a live record [4 .. 11] are 0.
 *   per entry, 8 + 8 A + 2 L words: chip, column, class, max, A = appearances, L = listed rows = min(unguarded_nonzero_rows,
 *   max_rows_per_entry), unguarded_nonzero_rows (u64); then per appearance 8 words: interaction, position, is_send, is_global, bus_index, lookup
 *   (a send on a lookup bus), live_rows (u64); then L (row, value) pairs. */
typedef struct vgpu_domain_audit_opts {
    uint64_t max_entries;
    uint32_t max_rows_per_entry;
    uint32_t chip_mask;
    uint32_t max_bits;
    uint32_t lookup_auto;
    uint64_t lookup_global_mask;
    uint64_t lookup_local_mask;
    uint32_t reserved[2];
} vgpu_domain_audit_opts_t;
typedef struct vgpu_domain_report vgpu_domain_report_t;
int32_t vgpu_domain_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                          uint32_t n_prep, const vgpu_domain_audit_opts_t* opts, vgpu_domain_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_domain_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                               const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                               const vgpu_domain_audit_opts_t* opts, vgpu_domain_report_t** out);
uint64_t vgpu_domain_report_len(const vgpu_domain_report_t* r);
const uint32_t* vgpu_domain_report_words(const vgpu_domain_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: cells scanned (main cells of the
 * audited chips plus one per evaluated count or field vcol and row) */
void vgpu_domain_report_timing(const vgpu_domain_report_t* r, double out[3]);
void vgpu_domain_report_free(vgpu_domain_report_t* r);

/* ---- Memory audit: the audits above judge a witness by bus balance and by local algebra.  None asks whether the memory table IS a memory: the
 * reference's memory AIR is commented out (memory/src/stark.rs:22-78), so nothing requires a read to return the last value written to its
 * address, and a wrong value planted consistently in the sender's channel and the table's row passes every one of them.  This audit replays
 * the receives of one bus as a memory and names the records that break it.  Inputs: exactly what vgpu_prove and the audits take.
 *   bus       global bus 2 (the BasicMachine's memory bus) by default; bus_is_global / bus_index name another.  Every RECEIVE on it is read
 *             through its vcols and must have exactly 8 fields (is_read, clk, addr, is_static_initial, v0, v1, v2, v3), the shape of
 *             memory/src/lib.rs:216-233.  Another field count, a bus without a receive, more than 2^32 - 2 slots: VGPU_ERR_INVALID_ARG, the
 *             message names the reason.
 *   records   a SLOT is (chip, receive, row), LIVE iff its count vcol != 0 at the row; values canonical.  A live record is a READ iff
 *             is_read == 1, otherwise a WRITE; STATIC iff is_static_initial == 1.
 *   order     live records by (addr, clk, static before non-static, seq), seq = lexicographic (chip, row, interaction): the key
 *             addr << 32 | clk << 1 | !static and a stable sort of the slots enumerated in seq order.  Inside one (addr, clk) the bus record
 *             carries no ordinal: the trace's own order decides, as the reference's stable sort of the clk-ordered log leaves it;
 *             same_cycle_pairs counts the verdicts that rest on that.
 *   state     per address the last WRITE before a record in that order, or none; a read leaves it unchanged; an address nobody has written
 *             reads as 0 (read_or_init, memory/src/lib.rs:107-120).
 *   findings  at most one kind per live record, the lowest applicable: 1 MALFORMED with a reason mask (bit 0 count != 1, bit 1 is_read not in
 *             {0, 1}, bit 2 is_static not in {0, 1}, bit 3 static with is_read == 1 or clk != 0, bit 4 a value field >= 256; the record still
 *             takes its place in the order and acts as a write or read by the rule above), 2 DUPLICATE_STATIC (a static record whose
 *             predecessor in the order is a static record of the same address), 3 STALE_READ (a read with a last write whose four value
 *             fields differ from the read's, compared as field elements), 4 UNINIT_READ (a read with no write before it and a non-zero
 *             value).  A tampered read is one finding; a tampered write one per read that follows it before the next write.
 *   counters  exact: live, reads, writes, statics, addresses (distinct), min_addr, max_addr, max_clk, uninit_zero_reads (a read with no write
 *             before it and value 0: counted, never a finding), same_cycle_pairs (positions whose predecessor has the same (addr, clk), both
 *             non-static, at least one a write), max_clk_gap (between successive records of one address), dummy_reads_clk (over successive
 *             same-address pairs with gap > L the sum of gap / L), dummy_reads_addr (over successive different addresses with difference > L
 *             the sum of diff / L), L = live: what insert_dummy_reads (memory/src/lib.rs:286-362) would add, static records counted as
 *             operations at clk 0; layout_descents (rows r with rows r and r + 1 of one chip and receive both live and key(r) > key(r + 1))
 *             and the first such (chip, row): whether an adjacent-row AIR could hold on the trace as laid out; one count per kind.
 *   list      the first max_findings findings in ascending order position (default 64, at most 2^20; in a struct taken as given: 0 lists
 *             nothing and every count stays exact).  reserved must be zero.  A null options pointer gives the defaults.
 * What it is not: it judges the table's receives only (whether the senders agree is the bus audit's question) and THIS witness only; same-cycle
 * order is the trace's, not proven; addresses are field elements, so two u32 addresses p apart are one address here, as in the proof; it says
 * nothing about a continuation's initial memory.
 * vgpu_memory_audit runs on the device (kernels/memory_audit.hip), queued on the prover context, wave64, workgroups of 256: k_mm_keys (a
 * thread per row, one descriptor walk per receive; key and id per slot, per workgroup the live count, the OR of the live keys and of their
 * complements and the layout descents from an LDS tile with one halo row), the bus audit's radix sort over the key bytes in which some live
 * key differs, k_mm_gather (order position -> packed record and a mark: position + 1 for a write or the first record of an address), an
 * exclusive max-scan of the marks (the last write), k_mm_judge (kind, reason, counters by ballots, LDS, one atomic per counter and workgroup;
 * findings by count -> scan -> list).  The only atomics are integer add, or and max: every word is the same run after run.  Scratch from the
 * pool, its totals zeroed by one memset; VGPU_ERR_OOM with the arithmetic when the pool cannot give it.  vgpu_memory_audit_host: the same
 * contract on the host, one thread, std::stable_sort, no limits.
 * Report image (vgpu_memory_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x314d4d56 "VMM1" [1] word count [2] bus_is_global [3] bus_index [4] receives [5] truncated [6] listed [7] max_findings [8,9] slots
 *   [10,11] live [12,13] reads [14,15] writes [16,17] statics [18,19] addresses [20] min_addr [21] max_addr [22] max_clk [23] max_clk_gap
 *   [24,25] uninit_zero_reads [26,27] same_cycle_pairs [28,29] dummy_reads_clk [30,31] dummy_reads_addr [32,33] layout_descents [34] chip and
 *   [35] row of the first descent (all ones: none) [36,37] findings [38,39] malformed [40,41] duplicate_static [42,43] stale_read [44,45]
 *   uninit_read [46,47] 0; without a live record [20 .. 23] are 0
 *   per receive, seq order, 2 words: chip, interaction
 *   per listed finding 20 words: [0] kind [1] reason [2] chip [3] interaction [4] row [5] addr [6] clk [7..10] value [11..14] expected (the
 *   last write's value, 0 when there is none) [15] chip [16] interaction [17] row of the last write (all ones: none) [18] order position [19] 0 */
typedef struct vgpu_memory_audit_opts {
    uint32_t max_findings;
    uint32_t bus_is_global;
    uint32_t bus_index;
    uint32_t reserved;
} vgpu_memory_audit_opts_t;
typedef struct vgpu_memory_report vgpu_memory_report_t;
int32_t vgpu_memory_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                          uint32_t n_prep, const vgpu_memory_audit_opts_t* opts, vgpu_memory_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_memory_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                               const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                               const vgpu_memory_audit_opts_t* opts, vgpu_memory_report_t** out);
uint64_t vgpu_memory_report_len(const vgpu_memory_report_t* r);
const uint32_t* vgpu_memory_report_words(const vgpu_memory_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: slots evaluated */
void vgpu_memory_report_timing(const vgpu_memory_report_t* r, double out[3]);
void vgpu_memory_report_free(vgpu_memory_report_t* r);

/* ---- Program audit: the memory audit asks whether the memory table is a memory; the same hole exists for instruction fetch.  The reference comments
 * out both halves of the program bus (the cpu's send of (pc, opcode, a..e) with count one, cpu/src/lib.rs:138-157; the program chip's receive of
 * the preprocessed ROM row with count `multiplicity`, program/src/lib.rs:50-68) and the program chip's AIR is empty: nothing ties a cpu row's
 * instruction to ROM[pc] or the multiplicity column to how often a word ran.  This audit replays the would-be bus exactly.  Inputs: exactly what
 * vgpu_prove and the audits take.
 *   options   fetch_chip (default 0, the cpu), pc_col (1), n_fields (6; 1 to 8), field_cols (3..8: opcode, a..e; main columns of the fetching
 *             chip), table_chip (1, program), key_col (0) and table_cols (1..6), preprocessed columns of the table chip, mult_col (0), a main
 *             column of the table chip, rom_len (0: the table's height; the table's rows from rom_len on are padding and not fetchable),
 *             max_findings and max_ranges (64, at most 2^20; in a struct taken as given: 0 lists nothing and every count stays exact), reserved
 *             (0).  A null pointer gives these defaults, the BasicMachine's.  VGPU_ERR_INVALID_ARG before anything is queued, the message naming
 *             the reason: a column outside its trace, a table chip without a preprocessed trace, a table whose main and preprocessed heights
 *             differ, rom_len above the table's height, a fetch or table height above 2^30, n_fields outside 1..8, a non-zero reserved.
 *   records   a FETCH is every row r of the fetching chip, padding rows included, count one: pc(r) = the cell at pc_col, f(r)[j] = the cell at
 *             field_cols[j].  A table row i has key K[i], word W[i][j], multiplicity m[i].  c[i] = the fetches with pc(r) == i, for i below the
 *             table's height.  Lookups are by row index; values canonical.
 *   findings  1 TABLE_KEY (a table row with K[i] != i), 2 PC_OUT_OF_ROM (a fetch with pc >= rom_len), 3 WRONG_INSTRUCTION (pc < rom_len and some
 *             field differs from W[pc] by something other than 2^32 mod p = 268435454), 4 WRAPPED_OPERAND (pc < rom_len, at least one field
 *             differs and every differing field has f - W = 2^32 mod p: the reference's set_imm_value / set_left_imm_value, cpu/src/lib.rs:
 *             356-372, put the u32 value of a negative immediate mod p into the cpu row where the ROM holds from_i32 of it; counted and listed
 *             apart, never a fault), 5 MULTIPLICITY (m[i] != c[i] mod p).  mask: bit j for every differing field, wrapped or not.  A fetch gets at
 *             most one of 2, 3, 4; a table row may get 1 and 5.  Kinds 1, 2, 3, 5 are the HARD findings.  With rom_len = the table's height
 *             there is no hard and no wrapped finding exactly when the reference's program bus, uncommented, balances on this witness.
 *   counters  exact: fetches, table rows, rom_len, fetched_words (i < rom_len with c[i] > 0), unfetched_words, unfetched_ranges (maximal runs of
 *             unfetched words below rom_len), hottest_pc and hottest_count (the largest c[i] over the table's rows, the lowest i on a tie; 0 and 0
 *             when no fetch hits the table), first_pc, last_pc, over the windows (r, r + 1) sequential (pc' = pc + 1 in the field), stay
 *             (pc' = pc) and jumps (the rest); one count per kind.
 *   lists     findings: the first max_findings hard findings, TABLE_KEY by i, then the fetch findings by row, then MULTIPLICITY by i; wrapped:
 *             the first max_findings WRAPPED_OPERAND rows in row order; unfetched: the first max_ranges ranges [lo, hi), ascending.
 * What it is not: it judges the fetches against the table of THIS witness only.  It does not ask whether the opcode flags fit the opcode,
 * whether the step did what the opcode says (for the ALU results that is the arithmetic audit's question, below), or whether the preprocessed
 * commitment is the verifier's.
 * vgpu_program_audit runs on the device (kernels/program_audit.hip), queued on the prover context, wave64, workgroups of 256: k_pg_hist (the
 * fetch counts in an LDS histogram of min(table height, 32768) bins per workgroup, taller tables in slices; a wave whose live lanes hold one pc
 * adds once), k_pg_judge (a thread per fetch: kind, mask, the window to the next row through an LDS tile with one halo row; counters by ballots,
 * LDS, one atomic per counter and workgroup), k_pg_table (a thread per table row: key, multiplicity, fetched flag, range starts and ends through
 * a halo, the hottest word as a maximum of count << 32 | ~pc); every list by count -> scan -> list.  The only atomics are integer add and max:
 * every word is the same run after run.  Scratch from the pool, its totals and counts zeroed by one memset; VGPU_ERR_OOM with the arithmetic when
 * the pool cannot give it.  vgpu_program_audit_host: the same contract on the host, one thread, no limits beyond the refusals.
 * Report image (vgpu_program_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31475056 "VPG1" [1] word count [2] fetch_chip [3] table_chip [4] n_fields [5] truncated (bit 0 findings, bit 1 wrapped, bit 2
 *   unfetched) [6] listed findings [7] listed wrapped [8] listed ranges [9] max_findings [10] max_ranges [11] rom_len [12,13] fetches [14,15]
 *   table rows [16,17] fetched_words [18,19] unfetched_words [20,21] unfetched_ranges [22] hottest_pc [23] 0 [24,25] hottest_count [26]
 *   first_pc [27] last_pc [28,29] sequential [30,31] stay [32,33] jumps [34,35] hard findings [36,37] table_key [38,39] pc_out_of_rom [40,41]
 *   wrong_instruction [42,43] wrapped_operand [44,45] multiplicity [46,47] 0
 *   per listed finding, then per listed wrapped row, 24 words: [0] kind [1] mask [2] the fetch row (kinds 2, 3, 4) or the table row (1, 5)
 *   [3] pc (the table row for kinds 1, 5) [4..11] found: f(r)[j] (kinds 2, 3, 4), K[i] in [4] (kind 1), m[i] in [4] (kind 5) [12..19]
 *   expected: W[pc][j] (kinds 3, 4), 0 (kind 2), i in [12] (kind 1), c[i] mod p in [12] and c[i] in [13] (kind 5) [20..23] 0
 *   per listed range 2 words: lo, hi */
typedef struct vgpu_program_audit_opts {
    uint32_t fetch_chip;
    uint32_t pc_col;
    uint32_t n_fields;
    uint32_t field_cols[8];
    uint32_t table_chip;
    uint32_t key_col;
    uint32_t table_cols[8];
    uint32_t mult_col;
    uint32_t rom_len;
    uint32_t max_findings;
    uint32_t max_ranges;
    uint32_t reserved;
} vgpu_program_audit_opts_t;
typedef struct vgpu_program_report vgpu_program_report_t;
int32_t vgpu_program_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                           uint32_t n_prep, const vgpu_program_audit_opts_t* opts, vgpu_program_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_program_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                const vgpu_program_audit_opts_t* opts, vgpu_program_report_t** out);
uint64_t vgpu_program_report_len(const vgpu_program_report_t* r);
const uint32_t* vgpu_program_report_words(const vgpu_program_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: fetches + table rows */
void vgpu_program_report_timing(const vgpu_program_report_t* r, double out[3]);
void vgpu_program_report_free(vgpu_program_report_t* r);

/* ---- Arithmetic audit: the memory audit asks whether the memory table is a memory and the program audit whether the fetches match the ROM; this
 * one asks whether the ALU records compute their opcode.  `div`'s eval is a TODO in the reference, the field audit reports all 13 fields of its
 * receive as floating, `shift` delegates to `mul` and `div` on the general bus with a power of two as operand, and `lt`, `com`, `mul` and
 * `bitwise` are only as tight as their transcribed constraints: a result planted consistently in the ALU chip's row, the cpu's write channel and
 * the memory table passes every other audit.  This audit replays the general bus as arithmetic.  Inputs: exactly what vgpu_prove and the audits
 * take.
 *   options   max_findings (64, at most 2^20; in a struct taken as given: 0 lists nothing and every count stays exact), bus_is_global (1) and
 *             bus_index (0: the BasicMachine's general bus), sides (1; bit 0 the receives, bit 1 the sends: with bit 1 the cpu's own send
 *             (opcode, read 1, read 2, write, clk) is judged by the same rule), reserved (0).  A null pointer gives these defaults.
 *             VGPU_ERR_INVALID_ARG before anything is queued, the message naming the reason: an entry with fewer than 13 fields, a bus with no
 *             entry on the selected sides, sides outside 1..3, max_findings above 2^20, a non-zero reserved, more than 2^32 - 2 slots.
 *   entries   an ENTRY is a (chip, interaction) on that bus and a selected side, in ascending (chip, interaction) order, read through its vcols
 *             by the descriptor walk of the bus audit: the compiled and the interpreting machine give the same words.  Fields 0..12 are opcode,
 *             x[0..3], y[0..3], z[0..3], word bytes most significant first; fields beyond 12 (the clk of output and cpu) are ignored.
 *   records   a SLOT is (entry, row), LIVE iff its count vcol is non-zero at that row (lt's count is a multiplicity: any non-zero value is
 *             live); values canonical.  A live record is JUDGED iff its opcode is in 100..118, the nineteen ALU opcodes (index opcode - 100: ADD
 *             SUB MUL DIV LT SHL SHR AND OR XOR SDIV NE MULHU SRA MULHS LTE EQ SLT SLE), otherwise OTHER (WRITE 300 at output): counted, never
 *             judged.
 *   expected  the arithmetic the reference runs: ADD, SUB, MUL the low word; MULHU AND MULHS the unsigned high word of the 64-bit product (the
 *             reference zero-extends, machine/src/core.rs:146-158); DIV the unsigned quotient; SDIV the signed quotient truncated toward zero;
 *             SHL, SHR shift by y; SRA shifts by y and replicates the sign; AND, OR, XOR bitwise; LT, LTE unsigned, SLT, SLE signed, NE, EQ;
 *             a boolean result is the word (0, 0, 0, r).
 *   findings  per judged record at most one kind, the first that applies: 1 MALFORMED (some field among 1..12 is >= 256; mask: bit j - 1 for
 *             field j); 2 UNDEFINED (reason 1: DIV or SDIV with y = 0, 2: SDIV of 0x80000000 by 0xFFFFFFFF, 3: SHL, SHR or SRA with y >= 32;
 *             the VM refuses these, so no honest witness holds one); no finding if z is the expected word; 4 SHIFT_QUOTIENT (an SDIV record
 *             with y = 2^k, k <= 31, and z = sra(x, k), which differs from the truncated quotient: the shift chip's delegation of SRA to div,
 *             alu_u32/src/shift/mod.rs); 5 ARITHMETIC_SHR (an SHR record with z = sra(x, y), which differs from x >> y: the reference logs SRA
 *             rows as Shr32, shift/mod.rs:325-328); 3 WRONG_RESULT otherwise.  mask of kinds 3, 4, 5: the differing bytes of z, bit j for z[j].
 *             Kinds 1, 2, 3 are HARD, 4 and 5 SOFT: counted and listed apart, never a fault.
 *   counters  exact: slots, live, judged, other, one count per opcode, per kind and per UNDEFINED reason, mulhs_sign_matters (the well-formed
 *             MULHS records whose signed high word differs from the unsigned one: the rows on which the reference's MULHS is not the ISA's;
 *             counted, never a finding), per entry live and hard.
 *   lists     the first max_findings hard findings, then the first max_findings soft findings, each in slot order: entry-major, rows ascending.
 * What it is not: it judges each record alone, and this witness only.  Whether senders and receivers agree is the bus audit's question.  It does
 * not read the chips' auxiliary columns (carries, bit decompositions, power_of_two) and says nothing about the cpu's flags, pc or fp.
 * vgpu_arithmetic_audit runs on the device (kernels/arithmetic_audit.hip), queued on the prover context, wave64, workgroups of 256: k_ar_judge (a
 * launch per entry, a thread per row: one descriptor walk, the rule in plain u32 / u64 integer code, one packed verdict word per slot; counters by
 * ballots, LDS, one integer atomicAdd per counter and workgroup), the memory audit's scan over the two workgroup tables, k_ar_list (a thread per
 * row reads its verdict; a listed finding walks the descriptor again).  The only atomics are integer add: every word is the same run after run.
 * Scratch from the pool, its totals zeroed by one memset; VGPU_ERR_OOM with the arithmetic when the pool cannot give it.
 * vgpu_arithmetic_audit_host: the same contract on the host, one thread.
 * Report image (vgpu_arithmetic_report_words, u32 words; u64 values as lo, hi; field values canonical):
 *   [0] 0x31524156 "VAR1" [1] word count [2] bus_is_global [3] bus_index [4] sides [5] truncated (bit 0 hard list, bit 1 soft list) [6] listed
 *   hard [7] listed soft [8] max_findings [9] entries [10,11] slots [12,13] live [14,15] judged [16,17] other [18,19] hard [20,21] malformed
 *   [22,23] undefined [24,25] wrong_result [26,27] soft [28,29] shift_quotient [30,31] arithmetic_shr [32,33] mulhs_sign_matters [34,35]
 *   division by zero [36,37] signed overflow [38,39] shift range [40..77] the nineteen opcode counts [78,79] 0
 *   per entry 8 words: chip, interaction, is_send, n_fields, live (lo, hi), hard (lo, hi)
 *   per listed hard finding, then per listed soft finding, 24 words: [0] kind [1] mask or reason [2] chip [3] interaction [4] row [5] opcode
 *   [6..9] x [10..13] y [14..17] z [18] expected word (0 for kinds 1 and 2) [19] count [20] is_send [21..23] 0 */
typedef struct vgpu_arithmetic_audit_opts {
    uint32_t max_findings;
    uint32_t bus_is_global;
    uint32_t bus_index;
    uint32_t sides;
    uint32_t reserved;
} vgpu_arithmetic_audit_opts_t;
typedef struct vgpu_arithmetic_report vgpu_arithmetic_report_t;
int32_t vgpu_arithmetic_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                              uint32_t n_prep, const vgpu_arithmetic_audit_opts_t* opts, vgpu_arithmetic_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_arithmetic_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                   const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                   const vgpu_arithmetic_audit_opts_t* opts, vgpu_arithmetic_report_t** out);
uint64_t vgpu_arithmetic_report_len(const vgpu_arithmetic_report_t* r);
const uint32_t* vgpu_arithmetic_report_words(const vgpu_arithmetic_report_t* r);
/* out[0]: the device pass (0 for the host audit), out[1]: wall time of the whole call; milliseconds.  out[2]: the live records */
void vgpu_arithmetic_report_timing(const vgpu_arithmetic_report_t* r, double out[3]);
void vgpu_arithmetic_report_free(vgpu_arithmetic_report_t* r);

/* ---- Coverage audit: WHICH constraint or bus interaction detects each mutation of the mutation audit — per detector: does this witness exercise
 * it at all, and is it ever the only thing that catches a change.  Inputs: exactly what vgpu_prove and the audits take.
 *   mutations     exactly those of the mutation audit above: (chip, row r, main column c, delta index j), the same trace domain, 1 to 4 distinct
 *                 deltas (default {1, p - 1}); preprocessed columns are never mutated.
 *   detectors     of a chip with K constraints and M interactions: 0 .. K - 1 the constraints in assert_zero call order (the constraint audit's
 *                 numbering), K .. K + M - 1 the interactions in Chip::all_interactions order.
 *   kills         constraint k KILLS (r, c, j) when on the mutated trace it is non-zero at row r or at row (r - 1) mod n and was zero at that same
 *                 row on the unmutated trace (newly failing, as in the mutation audit; for n = 1 one evaluation, the cell local and next).
 *                 Interaction m kills it when its record on row r differs before and after (count 0: no record; otherwise (count, fields),
 *                 canonical).
 *   counts        S(r, c, j) = the set of detectors that kill the mutation.  Per cell (chip, detector t, column c, delta j), exact over all n
 *                 rows: kills = #{r : t in S}, sole = #{r : S = {t}}, first_row = min{r : t in S}, first_sole_row = min{r : S = {t}} or
 *                 0xFFFFFFFF when there is none.
 *   classes       per detector, over all columns and deltas: DEAD every kills is 0; SHADOWED some kills > 0 and every sole is 0; ESSENTIAL
 *                 anything else.
 *   per chip and delta   detected = #{(r, c) : S not empty}, free = n w - detected: the mutation audit's free for the same witness and deltas.
 *   order         cells with kills > 0 ascend by (chip, detector, column, delta index); only the first max_cells are listed, the chip blocks and
 *                 total_cells stay exact and `truncated` says the list was cut.  No challenge, no hash and no floating point enter: the same
 *                 words run after run, from the device and from the host, for Machine.basic and for captured AIRs alike.
 * What it is not: "dead" is a statement about THIS witness and single-cell mutations by these deltas — it measures what the test program
 * reaches, and is not a fault of the witness or of the AIR.  "Shadowed" does not mean removable: a constraint that is never alone against
 * one-cell changes may be the only guard against a two-cell change.
 * Options: a zero field selects its default — max_cells 8192 (at most 2^24), n_deltas 0 = the pair {1, p - 1}; otherwise deltas[0 .. n_deltas)
 * are 1 to 4 distinct canonical values in 1..p-1; max_workgroups 0 = the device's default number of workgroups along a chip's rows (a tuning
 * knob: the report never depends on it; the host audit ignores it); opts may be NULL; reserved != 0 is refused.
 * vgpu_coverage_audit runs on the device (kernels/coverage_audit.hip), queued on the prover context like a proof or the other audits; it accepts
 * device-generated and uploaded traces.  Scratch comes from the prover's pool: per chip 16 bytes per cell (detector, column, delta) and workgroup
 * along its rows (at most 1024 workgroups per chip by default, fewer for a chip of fewer than 1024 row tiles of 256; cpu at 2^20 rows: 95 MB),
 * 24 bytes per cell, 16 per (detector, delta), 32 per listed cell (at most max_cells per chip), 12 w of column flags, plus the working-layout
 * copy of every uploaded trace; VGPU_ERR_OOM with a message when the pool cannot give them; VGPU_ERR_INVALID_ARG for bad shapes, for a chip of more than 96
 * constraints and for one whose row tile with one column's cells does not fit 160 KB of LDS at 64 rows.  Only the chip blocks and the listed
 * cells are copied to the host.  vgpu_coverage_audit_host is the same contract on the host over canonical row-major matrices (one thread, no
 * device, no limits).  Both validate shapes as vgpu_prove does.
 * Report image (vgpu_coverage_report_words, u32 words; u64 values as lo, hi):
 *   [0] 0x31524b56 "VKR1" [1] word count [2] n_deltas D [3] truncated [4,5] total_cells = cells with kills > 0 (exact even when the list is cut)
 *   [6] reported [7] n_chips [8..11] the deltas (canonical; unused slots 0)
 *   per chip, in machine order, 10 + 4 D + 4 D (K + M) words: width, K, M, 0, height (u64); the numbers of dead constraints, shadowed
 *   constraints, dead interactions, shadowed interactions; per delta detected, free (u64 each); per detector, per delta, kills and sole summed
 *   over the chip's columns (u64 each)
 *   per reported cell, 10 words: chip, detector, column, delta index, kills, sole (u64 each), first_row, first_sole_row. */
typedef struct vgpu_coverage_audit_opts {
    uint64_t max_cells;
    uint32_t n_deltas;
    uint32_t deltas[4];
    uint32_t max_workgroups;
    uint32_t reserved[2];
} vgpu_coverage_audit_opts_t;
typedef struct vgpu_coverage_report vgpu_coverage_report_t;
int32_t vgpu_coverage_audit(vgpu_prover_t* p, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips, const vgpu_trace_t* const* prep,
                            uint32_t n_prep, const vgpu_coverage_audit_opts_t* opts, vgpu_coverage_report_t** out);
/* main[i]: canonical row-major heights[i] x widths[i]; prep[k] (prep_heights[k] x prep_widths[k]) belongs to chip prep_chips[k] */
int32_t vgpu_coverage_audit_host(const vgpu_machine_t* machine, const uint32_t* const* main, const uint64_t* heights, const uint64_t* widths, uint32_t n_main,
                                 const uint32_t* prep_chips, const uint32_t* const* prep, const uint64_t* prep_heights, const uint64_t* prep_widths, uint32_t n_prep,
                                 const vgpu_coverage_audit_opts_t* opts, vgpu_coverage_report_t** out);
uint64_t vgpu_coverage_report_len(const vgpu_coverage_report_t* r);
const uint32_t* vgpu_coverage_report_words(const vgpu_coverage_report_t* r);
/* out[0]: the device pass (events around it on the prover's stream, after the working-layout copies of uploaded traces; 0 for the host audit),
 * out[1]: wall time of the whole call; milliseconds.  out[2]: the Air::eval row evaluations the audit performed (baselines included) */
void vgpu_coverage_report_timing(const vgpu_coverage_report_t* r, double out[3]);
void vgpu_coverage_report_free(vgpu_coverage_report_t* r);

/* ---- RCCL inside the library: one process per GPU; the host's launcher distributes the 128-byte id that rank 0
 * obtains from vgpu_comm_unique_id (any out-of-band channel: MPI, a file, the Rust host's own RPC), every rank then calls
 * vgpu_comm_init with its prover.  vgpu_comm_allgather_roots is the path's one collective: each segment's commitment roots
 * (3 x 8 words after vgpu_prove) to every rank over xGMI; out holds world * n_words words, rank-major. ---- */
typedef struct vgpu_comm vgpu_comm_t;
#define VGPU_COMM_ID_BYTES 128
int32_t vgpu_comm_unique_id(uint8_t id[VGPU_COMM_ID_BYTES]);
int32_t vgpu_comm_init(vgpu_prover_t* p, const uint8_t id[VGPU_COMM_ID_BYTES], uint32_t rank, uint32_t world, vgpu_comm_t** out);
int32_t vgpu_comm_allgather_roots(vgpu_comm_t* c, const uint32_t* words, uint32_t n_words, uint32_t* out);
void vgpu_comm_destroy(vgpu_comm_t* c);
/* Deadline of every collective issued through `c` (the roots all-gather, the exchanges of vgpu_prove_sharded): one that has not completed
 * within timeout_ms — a peer died or never entered it — is aborted (ncclCommAbort), the call fails (VGPU_ERR_HIP / VGPU_ERR_FABRIC) and the
 * communicator is dead: every later call on it is refused, create a new one.  0 (the default, or the environment's VGPU_COMM_TIMEOUT_MS) = wait for ever. */
int32_t vgpu_comm_set_timeout_ms(vgpu_comm_t* c, uint32_t timeout_ms);

/* ---- ONE proof sharded over several GPUs.  Its commitment round alone: pcs.commit_batches of one round sharded over the
 * ranks of `comm` — column-sharded LDEs, an all-to-all into row-range shards, a subtree per rank, an all-gather of the subtree
 * roots.  Every rank passes the SAME matrices (only its own columns are extended) and receives the SAME root that
 * vgpu_commit_batches gives on one GPU.  world must be a power of two. */
int32_t vgpu_commit_batches_sharded(vgpu_prover_t* p, vgpu_comm_t* comm, const vgpu_trace_t* const* mats, uint32_t n_mats, const uint32_t* coset_shifts,
                                    uint32_t root[8]);
/* The same phases with `world` prover contexts of THIS process standing in for the ranks (a box with one GPU): the exchanges
 * are device-to-device copies.  mats[r * n_mats + i] = matrix i as uploaded through provers[r]. */
int32_t vgpu_commit_batches_sharded_local(vgpu_prover_t* const* provers, uint32_t world, const vgpu_trace_t* const* mats, uint32_t n_mats,
                                          const uint32_t* coset_shifts, uint32_t root[8]);
/* The WHOLE of Machine::prove (basic/src/lib.rs:147-675) for one proof over the ranks of `comm`: every committed LDE, every Merkle
 * tree, the quotient evaluation, the opened values, the reduced openings and the FRI layers live and are computed in row-range shards
 * (a rank's row range of a bit-reversed LDE on s H_L is the sub-coset s w_L^e H_{L/W}, again bit-reversed: the single-GPU kernels run on
 * it with a shifted coset); the transcript is replicated.  Exchanges per proof: an all-to-all (columns -> row ranges) and a roots
 * all-gather per commitment round, one halo exchange (the successor shard) and one all-to-all (rows -> columns) around the quotient,
 * an all-gather of partial opened values, a roots all-gather per sharded FRI layer, an all-gather of the proof tail.  Every rank
 * passes the SAME traces (they are replicated; what a proof's memory goes into — LDEs, trees, FRI layers — is sharded) and
 * receives the SAME proof words vgpu_prove gives on one GPU.  Matrices whose LDE has fewer than max(4 world, 2^log_min_sharded) rows
 * are computed whole by every rank.  Any log_blowup (the quotient domain, machine/src/quotient.rs:41-47, is the first world >> (log_blowup - 1)
 * ranks' row ranges: those ranks evaluate the quotient); chips of log_quotient_degree 1; world must be a power of two.  The call
 * owns the prover context and the communicator until it returns: no other proof on `p`, no vgpu_comm_* call on `comm` from another thread
 * meanwhile (RCCL serialises the operations of one communicator), and every rank must make the same call with traces of the same shapes. */
int32_t vgpu_prove_sharded(vgpu_prover_t* p, vgpu_comm_t* comm, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips,
                           const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);
/* The same with `world` prover contexts of THIS process standing in for the ranks (device-to-device copies for the exchanges):
 * main[r * n_main + i] / prep[r * n_prep + k] = the traces as uploaded through provers[r]. */
int32_t vgpu_prove_sharded_local(vgpu_prover_t* const* provers, uint32_t world, const vgpu_trace_t* const* main, uint32_t n_main,
                                 const uint32_t* prep_chips, const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);

/* The same over the HOST'S OWN transport: one rank per process (or per thread with its own prover), the exchanges carried by two
 * callbacks over host buffers — what a Rust host plugs its MPI / TCP / shared-memory layer into, and how the sharded prover runs one rank
 * per process where no RCCL communicator exists.  Both callbacks are collective (every rank calls them in the same order with matching
 * sizes), block until this rank's data has arrived, and return 0 on success (anything else aborts the proof on every rank).
 *   all_gather : every rank contributes n_words words; out receives world * n_words words, rank-major.
 *   all_to_all : send[s] (send_words[s] words) goes to rank s, recv[s] (recv_words[s] words) arrives from rank s; the entries of s == rank
 *                are null / 0 (the library keeps its own block on the device).  Device blocks are staged through page-locked host memory.
 * Failure protocol: every exchange is staged first (everything that can fail on this rank alone: staging buffers, device-to-host copies),
 * then the ranks all_gather one status word, then the exchange runs.  A rank whose proof fails (bad shapes, out of memory, a HIP error)
 * reports it in the status word instead of going on, and EVERY rank returns VGPU_ERR_FABRIC (vgpu_last_error names the failing rank) instead
 * of blocking in an exchange its peer never enters.  A callback that itself returns non-zero is fatal for the transport: that rank returns
 * at once, issues no further callback, and its peers leave through their own callback's error or through the deadline.
 * Deadline: timeout_ms > 0 bounds every single callback.  The library then runs the callbacks on a helper thread of its own (they must be
 * callable from another thread than the caller's); one that has not returned in time is ABANDONED there — the library never touches its
 * buffers again, the helper thread ends if the callback ever returns — and the call fails with VGPU_ERR_FABRIC.  A peer that died costs the
 * survivors at most timeout_ms, never a hang.  timeout_ms == 0: callbacks run on the calling thread and must bound themselves.
 * struct_size must be sizeof(vgpu_fabric_t): a host compiled against another layout of this struct is refused, not misread. */
typedef struct vgpu_fabric {
    uint32_t struct_size;   /* = sizeof(vgpu_fabric_t) */
    uint32_t timeout_ms;    /* deadline of one callback; 0 = none */
    void* user;
    uint32_t rank, world;   /* world: a power of two */
    int32_t (*all_gather)(void* user, const uint32_t* words, uint64_t n_words, uint32_t* out);
    int32_t (*all_to_all)(void* user, const uint32_t* const* send, const uint64_t* send_words, uint32_t* const* recv, const uint64_t* recv_words);
} vgpu_fabric_t;
int32_t vgpu_prove_sharded_fabric(vgpu_prover_t* p, const vgpu_fabric_t* fabric, const vgpu_trace_t* const* main, uint32_t n_main, const uint32_t* prep_chips,
                                  const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);
/* The same three entry points with ROW-RANGE inputs: the traces themselves are sharded.  A chip whose LDE is sharded — at least
 * max(4 world, 2^log_min_sharded, 2 * 2^log_blowup) LDE rows: vgpu_sharded_trace_is_split says so for a trace height — hands in ONLY its rows
 * [rank n / world, (rank + 1) n / world) (a trace of n / world rows, natural order); every other chip its whole trace.  full_heights[i] = chip i's
 * whole trace height n on every rank.  Per-rank trace memory and the permutation-trace work are then 1 / world too: generate_permutation_trace's
 * running sum (machine/src/chip.rs:176-205) becomes a local scan plus ONE all-gather of the ranks' totals (5 words per chip), and every
 * commitment round deals the row ranges into whole columns with one more all-to-all.  The preprocessed traces (constants of the program) are
 * handed in whole on every rank.  The proof words are those of vgpu_prove on one GPU. */
uint32_t vgpu_sharded_trace_is_split(uint32_t world, uint32_t log_blowup, uint32_t log_min_sharded, uint64_t height);
int32_t vgpu_prove_sharded_rows(vgpu_prover_t* p, vgpu_comm_t* comm, const vgpu_trace_t* const* main, uint32_t n_main, const uint64_t* full_heights, const uint32_t* prep_chips,
                                const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);
int32_t vgpu_prove_sharded_rows_fabric(vgpu_prover_t* p, const vgpu_fabric_t* fabric, const vgpu_trace_t* const* main, uint32_t n_main, const uint64_t* full_heights,
                                       const uint32_t* prep_chips, const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);
/* main[r * n_main + i] = rank r's rows (or whole trace) of chip i as uploaded through provers[r] */
int32_t vgpu_prove_sharded_rows_local(vgpu_prover_t* const* provers, uint32_t world, const vgpu_trace_t* const* main, uint32_t n_main, const uint64_t* full_heights,
                                      const uint32_t* prep_chips, const vgpu_trace_t* const* prep, uint32_t n_prep, uint32_t log_min_sharded, vgpu_proof_t** out);
/* Host-only check of a transport before proofs depend on it (no device needed): a status round, an all_gather of n_words rank-dependent
 * words and an all_to_all of rank-pair-dependent blocks of different sizes, every received word verified.  fail_rank < world makes that
 * rank fail between two exchanges the way a failing proof would: every rank must then return a non-zero status — none may hang. */
int32_t vgpu_fabric_selftest(const vgpu_fabric_t* fabric, uint32_t n_words, uint32_t fail_rank);

/* ---- trace generation on the device: Chip::generate_trace (machine/src/chip.rs:22) of the big
 * BasicMachine chips as kernels, fed by the VM's operation logs instead of host-built RowMajorMatrix traces.
 * The logs are what the reference's chips hold after Machine::run: Cpu::operations + pc/fp/instruction per cycle
 * (cpu/src/lib.rs:56-77), MemoryChip::operations: BTreeMap<clk, Vec<Operation>> flattened in (clk, issue) order
 * (memory/src/lib.rs:25-60), and each ALU chip's Vec<Operation> (alu_u32/src/add/mod.rs:26-36).  Words cross the
 * ABI as the u32 value of the big-endian Word (machine/src/core.rs:9). ---- */
/* cpu Operation (cpu/src/lib.rs:40-54).  The last four are appended (their order is not the reference's enum order): LOADU8 / LOADS8
 * (cpu/src/lib.rs:493-601: a read of the pointer, a read of its word, the write), STOREU8 (:646-697: three reads — the third read_or_init,
 * memory/src/lib.rs:107-120, which logs a Read of 0 for a never-written cell — then the write; channel 1 keeps the last of the later reads,
 * :253-296, so the second read reaches no channel), READ_ADVICE (:398-436: one write, the advice byte or u32::MAX at the end of the tape). */
enum { VGPU_CPU_STORE32 = 0, VGPU_CPU_LOAD32, VGPU_CPU_JAL, VGPU_CPU_JALV, VGPU_CPU_BEQ, VGPU_CPU_BNE, VGPU_CPU_IMM32, VGPU_CPU_BUS,
       VGPU_CPU_BUS_LEFT_IMM, VGPU_CPU_STOP, VGPU_CPU_LOADFP, VGPU_CPU_LOAD_U8, VGPU_CPU_LOAD_S8, VGPU_CPU_STORE_U8, VGPU_CPU_READ_ADVICE };
typedef struct vgpu_cpu_op {
    uint32_t pc, fp, opcode;
    int32_t operands[5];
    uint32_t kind;        /* VGPU_CPU_* */
    uint32_t has_imm;     /* Operation::*(Some(imm)) */
    uint32_t imm;
    uint32_t mem_first;   /* index of this cycle's first entry in the memory log */
} vgpu_cpu_op_t;
typedef struct vgpu_mem_op { uint32_t clk, addr, value, is_write; } vgpu_mem_op_t;   /* memory Operation::{Read,Write}(addr, value) at clk */
typedef struct vgpu_alu_op { uint32_t opcode, a, b, c; } vgpu_alu_op_t;              /* e.g. Operation::Add32(a, b, c): a = result */
typedef struct vgpu_out_op { uint32_t clk, byte; } vgpu_out_op_t;                    /* OutputChip::values entry (clk, byte) (output/src/lib.rs:21-23) */
typedef struct vgpu_oplog_desc {
    uint64_t struct_size;   /* = sizeof(vgpu_oplog_desc_t): vgpu_oplog_upload refuses a host compiled against another layout of this struct */
    const vgpu_cpu_op_t* cpu; uint64_t n_cpu;
    const vgpu_mem_op_t* mem; uint64_t n_mem;
    const vgpu_alu_op_t* alu[4]; uint64_t n_alu[4];   /* add, sub, lt, bitwise */
    const uint32_t* static_cells; uint64_t n_static;  /* MemoryChip::static_data as (addr, value) pairs, ascending address (may be null / 0) */
    uint32_t rom_len;                                 /* ProgramROM length (program chip rows before padding) */
    /* the five remaining chips, each as the reference's chip holds it after Machine::run: Mul32Chip / Div32Chip / Shift32Chip / Com32Chip
     * ::operations (opcode = the Operation variant: MUL32 | MULHS32 | MULHU32, DIV32 | SDIV32, SHL32 | SHR32 | SRA32, NE32 | EQ32 — a shift
     * instruction also leaves a Mul32 / Div32 / SDiv32 with the power of two in the mul / div log, alu_u32/src/shift/mod.rs:207-212) and
     * OutputChip::values.  All may be null / 0. */
    const vgpu_alu_op_t* alu2[4]; uint64_t n_alu2[4];  /* mul, div, shift, com */
    const vgpu_out_op_t* output; uint64_t n_output;
} vgpu_oplog_desc_t;
typedef struct vgpu_oplog vgpu_oplog_t;
int32_t vgpu_oplog_upload(vgpu_prover_t* p, const vgpu_oplog_desc_t* log, vgpu_oplog_t** out);
/* the checks vgpu_oplog_upload makes, without a device: VGPU_OK, or VGPU_ERR_INVALID_ARG with the reason in vgpu_last_error() */
int32_t vgpu_oplog_validate(const vgpu_oplog_desc_t* log);
void vgpu_oplog_free(vgpu_oplog_t* log);
/* Any chip of the BasicMachine — all fourteen Chip::generate_trace as kernels: cpu, program, mem, add, sub, lt, bitwise, mul, div, shift,
 * com, output from their logs (the last five exactly as incomplete as the reference fills them: div / com rows carry only the opcode
 * flag, mul leaves r / s zero, output never writes counter / counter_mult / opcode), range from the result words of the instructions
 * that range-check them (add, sub, mul*, div*: the cpu log's bus operations and the cycle's memory write), static_data from the
 * initialised cells.  The returned trace is already in the prover's working layout (no ingest pass). */
int32_t vgpu_generate_trace(vgpu_prover_t* p, const vgpu_oplog_t* log, uint32_t chip, vgpu_trace_t** out);
void vgpu_trace_shape(const vgpu_trace_t* t, uint64_t* height, uint64_t* width);
/* canonical row-major copy of a device trace (what the reference's generate_trace would have returned) */
int32_t vgpu_trace_download(vgpu_prover_t* p, const vgpu_trace_t* t, uint32_t* out, uint64_t cap_words);

/* ---- synthetic workloads (bench inputs; upstream of the hot path) ---- */
typedef struct vgpu_workload vgpu_workload_t;
/* fib_program (basic/tests/test_prover.rs:35-188) with loop bound n, fp = 0x1000, run to STOP, traces generated */
int32_t vgpu_workload_fib(uint32_t n, vgpu_workload_t** out);
/* ALU-heavy loop (SURVEY.md §8 workload C4): add, sub, xor, and, or, lt, addi, addi, bne per iteration */
int32_t vgpu_workload_alu(uint32_t iters, vgpu_workload_t** out);
/* the reference's other pinned prover programs (basic/tests/test_prover.rs:190-402): "left_imm_ops", "signed_inequality", "loadfp",
 * and "static_data" (basic/tests/test_static_data.rs:31-59, cells 0x10 / 0x14 initialised through the static-data chip) */
int32_t vgpu_workload_named(const char* name, vgpu_workload_t** out);
/* final value of the 32-bit memory cell at `addr` (machine.mem().cells, test_prover.rs:483-486,494-640) */
int32_t vgpu_workload_cell(const vgpu_workload_t* w, uint32_t addr, uint32_t* value);
void vgpu_workload_free(vgpu_workload_t* w);
/* stats: [cycles, cpu ops, memory ops, add ops, result word (u32 at fp+4), program length, padded cpu height] */
void vgpu_workload_stats(const vgpu_workload_t* w, uint64_t out[8]);
int32_t vgpu_workload_main_trace(const vgpu_workload_t* w, uint32_t chip, const uint32_t** data, uint64_t* height, uint64_t* width);
/* the VM's operation logs (pointers stay valid until vgpu_workload_free) */
void vgpu_workload_oplog(const vgpu_workload_t* w, vgpu_oplog_desc_t* out);
/* k = 0: program ROM (chip 1), k = 1: range table (chip 12) */
int32_t vgpu_workload_preprocessed(const vgpu_workload_t* w, uint32_t k, uint32_t* chip, const uint32_t** data, uint64_t* height, uint64_t* width);
/* A Valida executable (basic/src/bin/valida.rs:340-354): load_executable_file (elf/src/lib.rs:19-120) — raw machine code, 24-byte little-endian
 * records (ProgramROM::from_machine_code, machine/src/program.rs:181-196), or a little-endian ELF32 / ELF64 (code, static data, initial pc) —
 * then Machine::run (basic/src/lib.rs:127-145) with fp = stack_height and the FixedAdviceProvider tape `advice` (machine/src/advice.rs:30-56),
 * all traces generated.  The VM executes every BasicMachine opcode Machine::step dispatches (basic/src/lib.rs:1066-1188).  Refused with a
 * message, never a crash: a malformed or truncated file, big-endian ELF, ELFCLASS other than 32 / 64, extended section numbering, no text
 * section, a data address beyond 32 bits, more than 2^22 instructions or 2^22 static cells; at run time an unrecognized opcode, a pc beyond
 * the ROM, a read before write, and a run that has not stopped after max_cycles cycles (the messages carry pc and opcode).
 * max_cycles = 0: load only (ROM, static data, preprocessed traces; no run, empty logs, no main traces). */
int32_t vgpu_workload_from_executable(const uint8_t* exe, uint64_t n_bytes, uint32_t stack_height,
                                      const uint8_t* advice, uint64_t n_advice, uint64_t max_cycles, vgpu_workload_t** out);
/* OutputChip::bytes (output/src/lib.rs:27-29): the bytes WRITE put on the output tape.  Returns their number (copies min(number, cap) to
 * out, which may be null when cap = 0), or a negative error code. */
int64_t vgpu_workload_output(const vgpu_workload_t* w, uint8_t* out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* VGPU_H */
