// Batched Machine::verify on the device: the per-query checks of pcs.verify_multi_batches (host/verifier.hpp check_fri_plan) over a chunk
// of plans (kernels/verify_args.hpp, built by host/verify_batch.hpp), for every (proof, query) of the chunk at once.
//   k_verify_open  one thread per (query, reduced-opening term): alpha^k (row_j - y_j) / (x - z) summed over the term's columns, x = g w^rev(index)
//   k_verify_fold  one thread per query: the FRI fold through every commit-phase layer, each layer's opened row (folded value and sibling, in
//                  sibling order) written for the tree kernel, the final-polynomial comparison as a flag
//   k_verify_tree  one thread per Merkle opening (input rounds and commit-phase layers): hash the opened rows (height-sorted commit order),
//                  walk the sibling path with the injections, compare with the root
// Field sums are exact, so the terms' partial sums may be added in any order: the fold adds them per LDE height as the host does.  Every
// kernel is thread-per-chain plain C++ (no wave intrinsics, no inline assembly beyond keccak.hpp's), so tools/hipemu runs this very source
// (tests/emu/verify_emu.cpp).  Proof content never decides an index: the plan builder bounded every offset and length.
#include "launch.hpp"
#include "keccak.hpp"
#include "poseidon_perm.hpp"
#include "verify_args.hpp"

namespace vk {

namespace {

__device__ __forceinline__ Ext5 ext_canonical(const uint32_t* w) {
    Ext5 e;
#pragma unroll
    for (int k = 0; k < 5; k++) e.c[k] = Fp::from_canonical(w[k]);
    return e;
}
__device__ __forceinline__ Ext5 ext_raw(const uint32_t* w) {
    Ext5 e;
#pragma unroll
    for (int k = 0; k < 5; k++) e.c[k] = Fp::raw(w[k]);
    return e;
}

// SerializingHasher32<Keccak256> over a stream of canonical words, 34 words per block
struct KeccakSponge {
    KState a;
    uint32_t blk[34];
    int pos;
    __device__ __forceinline__ void init() { kstate_zero(a); pos = 0; }
    __device__ __forceinline__ void absorb_block() {
#pragma unroll
        for (int k = 0; k < 34; k++) absorb_word(a, k, blk[k]);
    }
    __device__ __forceinline__ void push(uint32_t w) {
        blk[pos++] = w;
        if (pos == 34) { absorb_block(); keccak_f1600<false>(a); pos = 0; }
    }
    __device__ __forceinline__ void finish(uint32_t (&out)[8]) {
        for (int k = pos; k < 34; k++) blk[k] = 0;
        blk[pos] ^= 0x01u;
        blk[33] ^= 0x80000000u;
        absorb_block();
        keccak_f1600<true>(a);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = ((i & 1) ? a.hi[i >> 1] : a.lo[i >> 1]) % vg::P;  // from_wrapped_u32
    }
};
// PaddingFreeSponge<Perm16, 16, 8, 8>: each chunk of 8 elements OVERWRITES state[0..len), then the permutation
struct PoseidonSponge {
    Fp st[16];
    Fp buf[8];
    int pos;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 16; i++) st[i] = Fp::zero();
        pos = 0;
    }
    __device__ __forceinline__ void flush(const PoseidonTab& tab) {
#pragma unroll
        for (int i = 0; i < 8; i++) if (i < pos) st[i] = buf[i];
        poseidon16_permute(st, tab);
        pos = 0;
    }
    __device__ __forceinline__ void push(uint32_t w, const PoseidonTab& tab) {
        buf[pos++] = Fp::from_canonical(w);
        if (pos == 8) flush(tab);
    }
    __device__ __forceinline__ void finish(uint32_t (&out)[8], const PoseidonTab& tab) {
        if (pos) flush(tab);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = st[i].canonical();
    }
};

__device__ __forceinline__ void compress(int hash_kind, const PoseidonTab& tab, const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
    if (hash_kind == 1) {  // TruncatedPermutation<Perm16, 2, 8, 16>
        Fp st[16];
#pragma unroll
        for (int i = 0; i < 8; i++) { st[i] = Fp::from_canonical(l[i]); st[8 + i] = Fp::from_canonical(r[i]); }
        poseidon16_permute(st, tab);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = st[i].canonical();
        return;
    }
    KState a;  // CompressionFunctionFromHasher: H(l || r), 16 words in one block
    kstate_zero(a);
#pragma unroll
    for (int i = 0; i < 8; i++) { absorb_word(a, i, l[i]); absorb_word(a, 8 + i, r[i]); }
    absorb_word(a, 16, 0x01u);
    absorb_word(a, 33, 0x80000000u);
    keccak_f1600<true>(a);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = ((i & 1) ? a.hi[i >> 1] : a.lo[i >> 1]) % vg::P;
}

// H(concatenation of n_seg segments): pairs (arena offset, words) at seg
__device__ __forceinline__ void hash_segments(const VerifyChunkArgs& a, const PoseidonTab& tab, const uint32_t* seg, uint32_t n_seg, uint32_t (&out)[8]) {
    if (a.hash_kind == 1) {
        PoseidonSponge s;
        s.init();
        for (uint32_t k = 0; k < n_seg; k++) {
            const uint32_t* w = a.arena + seg[2 * k];
            for (uint32_t j = 0; j < seg[2 * k + 1]; j++) s.push(w[j], tab);
        }
        s.finish(out, tab);
        return;
    }
    KeccakSponge s;
    s.init();
    for (uint32_t k = 0; k < n_seg; k++) {
        const uint32_t* w = a.arena + seg[2 * k];
        for (uint32_t j = 0; j < seg[2 * k + 1]; j++) s.push(w[j]);
    }
    s.finish(out);
}

}  // namespace

__global__ void __launch_bounds__(256) k_verify_open(VerifyChunkArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n_open) return;
    const uint32_t qi = a.open_jobs[2 * j], ti = a.open_jobs[2 * j + 1];
    const VfQuery Q = a.queries[qi];
    const VfProof P = a.proofs[Q.proof];
    const VfTerm T = a.terms[P.term0 + ti];
    const uint32_t* row = a.arena + a.idx[Q.rows + ti];
    const uint32_t rev = vg::reverse_bits_len(Q.index >> (P.log_max - T.lh), T.lh);
    const Fp x = Fp::from_canonical(vg::GENERATOR) * vg::two_adic_generator(T.lh).pow(rev);
    const Ext5 dinv = (Ext5::from_base(x) - ext_canonical(a.arena + T.z)).inv();
    const Ext5 alpha = ext_canonical(a.arena + P.alpha);
    Ext5 ap = ext_canonical(a.arena + T.apow), acc = Ext5::zero();
    for (uint32_t c = 0; c < T.width; c++) {
        acc += ap * ((Ext5::from_base(Fp::from_canonical(row[c])) - ext_canonical(a.arena + T.ys + 5 * c)) * dinv);
        ap *= alpha;
    }
    uint32_t* out = a.arena + Q.ro + 5 * ti;
#pragma unroll
    for (int k = 0; k < 5; k++) out[k] = acc.c[k].v;
}

__global__ void __launch_bounds__(256) k_verify_fold(VerifyChunkArgs a) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= a.n_queries) return;
    const VfQuery Q = a.queries[qi];
    const VfProof P = a.proofs[Q.proof];
    Ext5 folded = Ext5::zero();
    Fp x = vg::two_adic_generator(P.log_max).pow(vg::reverse_bits_len(Q.index, P.log_max));
    uint32_t idx = Q.index;
    const Fp minus_one = vg::two_adic_generator(1);
    for (uint32_t i = 0; i < P.n_layers; i++) {
        const uint32_t lf = P.log_max - 1 - i;
        for (uint32_t t = 0; t < P.n_terms; t++)
            if (a.terms[P.term0 + t].lh == lf + 1) folded += ext_raw(a.arena + Q.ro + 5 * t);
        const uint32_t sib = idx ^ 1u, pair = idx >> 1;
        Ext5 e0 = folded, e1 = folded;
        const Ext5 s = ext_canonical(a.arena + a.idx[Q.sibs + i]);
        if (sib & 1) e1 = s; else e0 = s;
        uint32_t* leaf = a.arena + Q.leaf + 10 * i;
#pragma unroll
        for (int c = 0; c < 5; c++) { leaf[c] = e0.c[c].canonical(); leaf[5 + c] = e1.c[c].canonical(); }
        Fp x0 = x, x1 = x;
        if (sib & 1) x1 *= minus_one; else x0 *= minus_one;
        const Ext5 beta = ext_canonical(a.arena + P.betas + 5 * i);
        folded = e0 + (beta - x0) * ((e1 - e0) * (x1 - x0).inv());
        idx = pair;
        x = x * x;
    }
    for (uint32_t t = 0; t < P.n_terms; t++)
        if (a.terms[P.term0 + t].lh == P.log_blowup) folded += ext_raw(a.arena + Q.ro + 5 * t);
    a.flags[Q.flag] = folded != ext_canonical(a.arena + P.final_poly) ? 1u : 0u;
}

__global__ void __launch_bounds__(128) k_verify_tree(VerifyChunkArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_trees) return;
    const VfTree T = a.trees[t];
    const PoseidonTab tab = tab_of(a.pos, a.pos_sparse);
    const uint32_t* grp = a.idx + T.grp;
    const uint32_t* seg = a.idx + T.seg;
    uint32_t node[8], tmp[8], h[8];
    hash_segments(a, tab, seg, grp[1], node);
    seg += 2 * grp[1];
    uint32_t g = 1, lh = grp[0], index = T.index;
    for (uint32_t k = 0; k < T.path_len; k++) {
        uint32_t sib[8];
        const uint32_t* sp = a.arena + T.path + 8 * k;
#pragma unroll
        for (int i = 0; i < 8; i++) sib[i] = sp[i];
        if (index & 1) compress(a.hash_kind, tab, sib, node, tmp);
        else compress(a.hash_kind, tab, node, sib, tmp);
        index >>= 1;
        lh--;
        if (g < T.n_grp && grp[2 * g] == lh) {
            hash_segments(a, tab, seg, grp[2 * g + 1], h);
            seg += 2 * grp[2 * g + 1];
            g++;
            compress(a.hash_kind, tab, tmp, h, node);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) node[i] = tmp[i];
        }
    }
    uint32_t bad = g != T.n_grp ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) bad |= node[i] != a.arena[T.root + i] ? 1u : 0u;
    a.flags[T.flag] = bad;
}

void launch_verify_chunk(hipStream_t st, const VerifyChunkArgs& a) {
    if (a.n_open) VK_LAUNCH(k_verify_open, dim3((a.n_open + 255) / 256), dim3(256), 0, st, a);
    if (a.n_queries) VK_LAUNCH(k_verify_fold, dim3((a.n_queries + 255) / 256), dim3(256), 0, st, a);
    if (a.n_trees) VK_LAUNCH(k_verify_tree, dim3((a.n_trees + 127) / 128), dim3(128), 0, st, a);
}

}  // namespace vk
