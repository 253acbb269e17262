// Batched Machine::verify (vgpu_verify_batch): the host half.  Per chunk of proofs:
//   1. plan_machine_proof of every proof on at most 16 host threads (parse, transcript, PoW, shapes: machine_verifier.hpp);
//   2. the plans packed into one flat buffer (kernels/verify_args.hpp) and their per-query checks run by a VerifyStage — the device
//      (kernels/verify.hip through capi.cpp), or the same kernels under tools/hipemu in the CPU tests;
//   3. per proof the first failure in the host verifier's order (a plan's slots: queries in order, each query's checks in order, a shape
//      failure ending the list), then finish_machine_proof (out-of-domain constraints, cumulative sums) on the host threads again.
// Verdicts and messages are vgpu_verify's: the host path is the same plan checked by check_fri_plan.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <functional>
#include <thread>
#include "machine_verifier.hpp"
#include "../kernels/verify_args.hpp"

namespace vhost {

// One chunk in flat form.  The arena is [the proofs' words, back to back (`spans`: where each comes from) | buf's arena part]; buf holds
// [arena part | idx | proofs | terms | queries | trees | open jobs], every table offset relative to buf.  flags: a separate array of n_flags
// words.  The proofs' words are never copied on the host: a stage puts each span where it belongs (the device stage uploads it directly).
struct VerifyChunk {
    struct Span { uint64_t at; const uint32_t* words; uint64_t n; };
    std::vector<Span> spans;
    uint64_t proof_words = 0;  // arena words the spans fill; buf's first word is arena word proof_words
    std::vector<uint32_t> buf;
    uint64_t idx_off = 0, proofs_off = 0, terms_off = 0, queries_off = 0, trees_off = 0, jobs_off = 0;
    uint32_t n_open = 0, n_queries = 0, n_trees = 0, n_flags = 0;
    uint64_t total_words() const { return proof_words + buf.size(); }
    // VerifyChunkArgs over an arena of total_words() words at `base` (device or host memory) and flags at `flags`
    vk::VerifyChunkArgs args(uint32_t* base, uint32_t* flags, int hash_kind, const uint32_t* pos, bool sparse) const {
        vk::VerifyChunkArgs a{};
        uint32_t* b = base + proof_words;
        a.arena = base;
        a.flags = flags;
        a.idx = b + idx_off;
        a.proofs = reinterpret_cast<const vk::VfProof*>(b + proofs_off);
        a.terms = reinterpret_cast<const vk::VfTerm*>(b + terms_off);
        a.queries = reinterpret_cast<const vk::VfQuery*>(b + queries_off);
        a.trees = reinterpret_cast<const vk::VfTree*>(b + trees_off);
        a.open_jobs = b + jobs_off;
        a.n_open = n_open; a.n_queries = n_queries; a.n_trees = n_trees;
        a.hash_kind = hash_kind; a.pos = pos; a.pos_sparse = sparse;
        return a;
    }
};
// runs a chunk's checks and returns its n_flags flag words
using VerifyStage = std::function<std::vector<uint32_t>(const VerifyChunk&)>;

// proofs of one call are cut into chunks of at most this many proof words (a single larger proof is a chunk of its own); a chunk's buffer
// is about 1.15 x its proof words (the plan's tables, accumulators and leaf rows beside them)
constexpr uint64_t VERIFY_CHUNK_WORDS_DEFAULT = 1ull << 25;  // 128 MiB of proof words, ~150 MiB of device buffer
constexpr unsigned VERIFY_HOST_THREADS = 16;                 // what a GPU job may use; never sized from the machine's core count

inline void parallel_for(size_t n, unsigned threads, const std::function<void(size_t)>& f) {
    const unsigned t = (unsigned)std::min<size_t>(n, std::max(1u, threads));
    if (t <= 1) { for (size_t i = 0; i < n; i++) f(i); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    std::exception_ptr err;
    std::mutex mu;
    for (unsigned k = 0; k < t; k++)
        pool.emplace_back([&] {
            for (size_t i; (i = next++) < n;) {
                try { f(i); } catch (...) { std::lock_guard<std::mutex> g(mu); if (!err) err = std::current_exception(); }
            }
        });
    for (auto& th : pool) th.join();
    if (err) std::rethrow_exception(err);
}

struct BatchVerifyResult { bool ok = true; std::string msg; };

namespace detail {

struct PlannedProof {
    bool rejected = false;
    std::string msg;
    MachinePlan mp;
    // per plan query, per slot: the flag slot of the device check (unused for REJECT)
    std::vector<std::vector<uint32_t>> slot_flag;
};

struct ChunkBuilder {
    VerifyChunk c;
    std::vector<uint32_t> arena, idx, jobs;
    std::vector<vk::VfProof> proofs;
    std::vector<vk::VfTerm> terms;
    std::vector<vk::VfQuery> queries;
    std::vector<vk::VfTree> trees;

    uint64_t next_proof = 0;  // where the next proof's words go (the proofs' region comes first: c.proof_words words, set before add())

    uint32_t off() const { return (uint32_t)(c.proof_words + arena.size()); }
    uint32_t put_ext(const Ext5& e) { const uint32_t o = off(); for (auto& k : e.c) arena.push_back(k.canonical()); return o; }
    uint32_t put_digest(const Digest8& d) { const uint32_t o = off(); arena.insert(arena.end(), d.begin(), d.end()); return o; }
    uint32_t reserve(size_t words) { const uint32_t o = off(); arena.resize(arena.size() + words, 0u); return o; }

    void add(PlannedProof& pp, const uint32_t* words, size_t n_words) {
        const FriPlan& f = pp.mp.fri;
        const uint64_t base = next_proof;
        c.spans.push_back({base, words, (uint64_t)n_words});
        next_proof += n_words;
        const uint64_t fb = base + pp.mp.fri_off;  // the FRI plan's offsets are relative to here
        vk::VfProof P{};
        P.log_max = f.log_max; P.log_blowup = f.log_blowup; P.n_layers = (uint32_t)f.betas.size();
        P.alpha = put_ext(f.alpha);
        P.betas = off();
        for (auto& b : f.betas) put_ext(b);
        P.final_poly = put_ext(f.final_poly);
        P.term0 = (uint32_t)terms.size(); P.n_terms = (uint32_t)f.terms.size();
        for (const FriPlan::Term& t : f.terms) {
            vk::VfTerm T{};
            T.lh = t.lh; T.width = t.width;
            T.z = put_ext(f.rounds[t.round].points[t.mat][t.point]);
            T.ys = off();
            for (auto& y : f.rounds[t.round].values[t.mat][t.point]) put_ext(y);
            T.apow = put_ext(f.alpha.pow(t.k0));
            terms.push_back(T);
        }
        std::vector<uint32_t> in_root, layer_root;
        for (auto& rd : f.rounds) in_root.push_back(put_digest(rd.commit));
        for (auto& cm : f.commits) layer_root.push_back(put_digest(cm));
        const uint32_t pi = (uint32_t)proofs.size();
        proofs.push_back(P);
        pp.slot_flag.resize(f.queries.size());
        for (size_t q = 0; q < f.queries.size(); q++) {
            const QueryPlan& Q = f.queries[q];
            vk::VfQuery VQ{};
            const uint32_t qi = (uint32_t)queries.size();
            if (Q.fold) {
                VQ.proof = pi; VQ.index = (uint32_t)Q.index;
                VQ.rows = (uint32_t)idx.size();
                for (const FriPlan::Term& t : f.terms) idx.push_back((uint32_t)(fb + Q.rows[t.round][t.mat]));
                VQ.ro = reserve(5 * f.terms.size());
                VQ.sibs = (uint32_t)idx.size();
                for (uint64_t s : Q.sib) idx.push_back((uint32_t)(fb + s));
                VQ.leaf = reserve(10 * f.betas.size());
                VQ.flag = c.n_flags++;
                queries.push_back(VQ);
                for (uint32_t t = 0; t < f.terms.size(); t++) { jobs.push_back(qi); jobs.push_back(t); }
            }
            for (const PlanSlot& s : Q.slots) {
                uint32_t flag = 0;
                if (s.kind == SLOT_FINAL) flag = VQ.flag;
                if (s.kind == SLOT_INPUT) {
                    const FriPlan::Round& R = f.in[s.at];
                    const VerifyRoundIn& rd = f.rounds[s.at];
                    vk::VfTree T{};
                    T.grp = (uint32_t)idx.size();
                    std::vector<uint32_t> segs;
                    for (size_t k = 0; k < R.order.size();) {  // groups of equally tall matrices, tallest first
                        size_t e = k;
                        while (e < R.order.size() && R.lde_h[R.order[e]] == R.lde_h[R.order[k]]) {
                            segs.push_back((uint32_t)(fb + Q.rows[s.at][R.order[e]]));
                            segs.push_back(rd.widths[R.order[e]]);
                            e++;
                        }
                        idx.push_back(vg::log2_strict_u64(R.lde_h[R.order[k]]));
                        idx.push_back((uint32_t)(e - k));
                        T.n_grp++;
                        k = e;
                    }
                    T.seg = (uint32_t)idx.size();
                    idx.insert(idx.end(), segs.begin(), segs.end());
                    T.path = (uint32_t)(fb + Q.in_path[s.at]);
                    T.path_len = R.log_h;
                    T.index = (uint32_t)(Q.index >> (f.log_max - R.log_h));
                    T.root = in_root[s.at];
                    T.flag = flag = c.n_flags++;
                    trees.push_back(T);
                } else if (s.kind == SLOT_LAYER) {
                    const unsigned lf = f.log_max - 1 - s.at;
                    vk::VfTree T{};
                    T.grp = (uint32_t)idx.size();
                    idx.push_back(lf);
                    idx.push_back(1);
                    T.n_grp = 1;
                    T.seg = (uint32_t)idx.size();
                    idx.push_back(VQ.leaf + 10 * s.at);
                    idx.push_back(10);
                    T.path = (uint32_t)(fb + Q.layer_path[s.at]);
                    T.path_len = lf;
                    T.index = (uint32_t)(Q.index >> (s.at + 1));
                    T.root = layer_root[s.at];
                    T.flag = flag = c.n_flags++;
                    trees.push_back(T);
                }
                pp.slot_flag[q].push_back(flag);
            }
        }
    }

    template <class T> void section(uint64_t& at, const std::vector<T>& v) {
        static_assert(sizeof(T) % 4 == 0, "word-sized tables");
        at = c.buf.size();
        const size_t w = v.size() * sizeof(T) / 4;
        c.buf.resize(c.buf.size() + w);
        if (w) memcpy(c.buf.data() + at, v.data(), w * 4);
    }
    VerifyChunk finish() {
        c.buf = std::move(arena);
        c.buf.reserve(c.buf.size() + idx.size() + (proofs.size() * sizeof(vk::VfProof) + terms.size() * sizeof(vk::VfTerm) + queries.size() * sizeof(vk::VfQuery) +
                                                   trees.size() * sizeof(vk::VfTree)) / 4 + jobs.size());
        section(c.idx_off, idx);
        section(c.proofs_off, proofs);
        section(c.terms_off, terms);
        section(c.queries_off, queries);
        section(c.trees_off, trees);
        section(c.jobs_off, jobs);
        if (c.total_words() >= (1ull << 32)) throw std::bad_alloc();  // offsets are 32-bit words
        c.n_open = (uint32_t)(jobs.size() / 2); c.n_queries = (uint32_t)queries.size(); c.n_trees = (uint32_t)trees.size();
        return std::move(c);
    }
};

}  // namespace detail

// Machine::verify of n proofs; results[i] is what verify_machine_proof decides for proof i (accepted, or its rejection message).
// Throws only on a failure of the stage (device or allocation).
inline std::vector<BatchVerifyResult> verify_machine_batch(const MachineDesc& machine, const FriParams& fri, const Poseidon16& perm16,
                                                           const uint32_t* const* proofs, const uint64_t* n_words, const uint32_t* preprocessed_commits,
                                                           size_t n_proofs, const VerifyStage& stage, uint64_t chunk_words = VERIFY_CHUNK_WORDS_DEFAULT,
                                                           double* plan_ms = nullptr, double* stage_ms = nullptr) {
    using clk = std::chrono::steady_clock;
    std::vector<BatchVerifyResult> out(n_proofs);
    double t_plan = 0, t_stage = 0;
    for (size_t c0 = 0; c0 < n_proofs;) {
        size_t c1 = c0 + 1;
        uint64_t words = n_words[c0];
        while (c1 < n_proofs && words + n_words[c1] <= chunk_words) words += n_words[c1++];
        const size_t n = c1 - c0;
        const auto t0 = clk::now();
        std::vector<detail::PlannedProof> pp(n);
        parallel_for(n, VERIFY_HOST_THREADS, [&](size_t i) {
            const size_t k = c0 + i;
            try {
                pp[i].mp = plan_machine_proof(machine, fri, perm16, preprocessed_commits ? preprocessed_commits + 8 * k : nullptr, proofs[k], (size_t)n_words[k]);
            } catch (const std::invalid_argument& e) { pp[i].rejected = true; pp[i].msg = e.what(); }
        });
        detail::ChunkBuilder b;
        for (size_t i = 0; i < n; i++) if (!pp[i].rejected) b.c.proof_words += n_words[c0 + i];
        for (size_t i = 0; i < n; i++) if (!pp[i].rejected) b.add(pp[i], proofs[c0 + i], (size_t)n_words[c0 + i]);
        VerifyChunk chunk = b.finish();
        const auto t1 = clk::now();
        std::vector<uint32_t> flags;
        if (chunk.n_flags) flags = stage(chunk);
        const auto t2 = clk::now();
        parallel_for(n, VERIFY_HOST_THREADS, [&](size_t i) {
            BatchVerifyResult& r = out[c0 + i];
            detail::PlannedProof& p = pp[i];
            if (p.rejected) { r.ok = false; r.msg = p.msg; return; }
            const FriPlan& f = p.mp.fri;
            for (size_t q = 0; q < f.queries.size() && r.ok; q++)
                for (size_t s = 0; s < f.queries[q].slots.size(); s++) {
                    const PlanSlot& sl = f.queries[q].slots[s];
                    const bool failed = sl.kind == SLOT_REJECT || flags.at(p.slot_flag[q][s]) != 0;
                    if (!failed) continue;
                    r.ok = false;
                    r.msg = sl.kind == SLOT_REJECT ? sl.why : sl.kind == SLOT_INPUT ? MSG_INPUT_MERKLE : sl.kind == SLOT_LAYER ? MSG_LAYER_MERKLE : MSG_FINAL_POLY;
                    break;
                }
            if (!r.ok) return;
            try { finish_machine_proof(machine, p.mp); } catch (const std::invalid_argument& e) { r.ok = false; r.msg = e.what(); }
        });
        const auto t3 = clk::now();
        t_plan += std::chrono::duration<double, std::milli>((t1 - t0) + (t3 - t2)).count();
        t_stage += std::chrono::duration<double, std::milli>(t2 - t1).count();
        c0 = c1;
    }
    if (plan_ms) *plan_ms = t_plan;
    if (stage_ms) *stage_ms = t_stage;
    return out;
}

}  // namespace vhost
