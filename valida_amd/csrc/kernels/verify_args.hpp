// The flat form of a chunk of Machine::verify plans (host/verify_batch.hpp builds it, kernels/verify.hip checks it): one u32 buffer whose
// sections are the arena and the job tables below.  Every offset is a WORD offset into the arena, every count and offset was bounded by
// the plan builder (the proof's words were parsed with their length fields checked, every path length equals its tree's log height), so
// the kernels index within the buffer without checking proof content again.
#pragma once
#include <cstdint>

namespace vk {

// per proof of the chunk
struct VfProof {
    uint32_t log_max, log_blowup, n_layers;
    uint32_t alpha, betas, final_poly;  // canonical Ext5 (betas: n_layers of them)
    uint32_t term0, n_terms;            // its reduced-opening terms: terms[term0 .. term0 + n_terms)
};
// one reduced-opening term: (proof, opened matrix, point), query-independent
struct VfTerm {
    uint32_t lh, width;  // log LDE height of the matrix, its width
    uint32_t z, ys;      // the point, the opened values (width canonical Ext5)
    uint32_t apow;       // alpha^k of the term's first column (canonical Ext5)
};
// one query whose reduced openings and fold chain are defined
struct VfQuery {
    uint32_t proof, index;
    uint32_t rows;   // n_terms arena offsets in the index table: the opened row of each term's matrix
    uint32_t ro;     // n_terms Ext5 accumulators (arena, written by k_verify_open)
    uint32_t sibs;   // n_layers arena offsets in the index table: each commit-phase step's sibling value
    uint32_t leaf;   // n_layers x 10 words (arena, written by k_verify_fold): each layer's opened row
    uint32_t flag;   // flag slot: the folded value differs from the final polynomial
};
// one Merkle opening: an input round or a commit-phase layer of one query
struct VfTree {
    uint32_t grp, n_grp;  // index table: n_grp x (log height, segment count), tallest first
    uint32_t seg;         // index table: segment pairs (arena offset, words), in height-sorted commit order, grouped as above
    uint32_t path, path_len, index, root;
    uint32_t flag;        // flag slot: the opening does not match its root
};

struct VerifyChunkArgs {
    uint32_t* arena;            // proof words, plan constants, accumulators, leaf rows
    uint32_t* flags;            // one word per check: 0 passed, 1 failed
    const uint32_t* idx;        // index table
    const VfProof* proofs;
    const VfTerm* terms;
    const VfQuery* queries;
    const VfTree* trees;
    const uint32_t* open_jobs;  // (query, term) pairs
    uint32_t n_open, n_queries, n_trees;
    int hash_kind;              // 0 Keccak-256, 1 Poseidon-16
    const uint32_t* pos;        // Poseidon tables (host/poseidon_opt.hpp poseidon_device_image), hash_kind 1
    bool pos_sparse;
};

}  // namespace vk
