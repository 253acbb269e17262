// What the Prover::*_audit device passes (prover_audits.cpp) have in common, written once: the trace checks, the pass object that owns the
// context for the pass's duration, the out-of-memory translation, and the few per-chip pieces that are the same code in several audits.
// Everything specific to an audit (its scratch layout, its launches, the decoding of what it lists) is in that audit's method.
#pragma once
#include "prover.hpp"

namespace vhost {
#pragma GCC visibility push(hidden)  // internal to the library: the scaffold adds nothing to its exported symbols

// The pool cannot give a pass its scratch: VGPU_ERR_OOM with a message that says how much it needs.
struct AuditNoMemory : std::bad_alloc {
    std::string msg;
    explicit AuditNoMemory(std::string m) : msg(std::move(m)) {}
    const char* what() const noexcept override { return msg.c_str(); }
};

// Runs the pass.  message() is evaluated only when an allocation failed, so it reads the sizes (scratch_words, rows_words, ..) as they stood then.
template <class Body, class Message>
void audit_or_no_memory(hipStream_t st, Body&& body, Message&& message) {
    try {
        body();
    } catch (const AuditNoMemory&) {
        throw;
    } catch (const std::bad_alloc&) {
        (void)hipStreamSynchronize(st);
        throw AuditNoMemory(message());
    }
}

// The shapes the plan functions validate (Shape: BusShape or ConstraintShape) and the chips of the preprocessed traces.
template <class Shape>
struct AuditTraces {
    std::vector<Shape> ms, ps;
    std::vector<int> prep_chips;
};
template <class Shape>
AuditTraces<Shape> audit_traces(const char* name, const std::vector<const DeviceTrace*>& main, const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed) {
    AuditTraces<Shape> t;
    for (auto m : main) { if (!m) throw std::invalid_argument(std::string(name) + ": null trace"); t.ms.push_back({m->height, m->width}); }
    for (auto& pr : preprocessed) { if (!pr.second) throw std::invalid_argument(std::string(name) + ": null trace"); t.prep_chips.push_back(pr.first); t.ps.push_back({pr.second->height, pr.second->width}); }
    return t;
}
// chip i's preprocessed trace (prep_slot as the plan functions fill it), or null
inline const DeviceTrace* audit_prep(const std::vector<std::pair<int, const DeviceTrace*>>& preprocessed, const std::vector<int>& prep_slot, size_t i) {
    return prep_slot[i] >= 0 ? preprocessed[(size_t)prep_slot[i]].second : nullptr;
}

// One audit pass on a context.  A context runs one thing at a time: the audit queues like a proof (prove_mu) and counts as one
// (proofs_running: an upload that arrives meanwhile goes beside it).  Members are released in reverse order: the working-layout copies,
// the events, the count, the lock.
class AuditPass {
    DeviceCtx& c_;
    struct Activated { explicit Activated(DeviceCtx& c) { c.activate(); } } before_lock_;
    std::unique_lock<std::mutex> one_at_a_time_;
    struct Running {
        std::atomic<int>& n;
        explicit Running(std::atomic<int>& a) : n(a) { n.fetch_add(1); }
        ~Running() { n.fetch_sub(1); }
    } running_;
    struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev_;
    std::vector<DMat> own_;

public:
    const hipStream_t stream;
    AuditPass(DeviceCtx& c, size_t n_traces) : c_(c), before_lock_(c), one_at_a_time_(c.prove_mu), running_(c.proofs_running), stream(c.stream) {
        own_.reserve(n_traces);
        c.activate();  // again: whoever held the lock may have pointed the launchers' profiler hook elsewhere
        VG_HIP_CHECK(hipEventCreate(&ev_.a));
        VG_HIP_CHECK(hipEventCreate(&ev_.b));
    }
    // the trace in the working layout, as prove makes it: traces generated on the device are already column-major Montgomery, an uploaded one is
    // ingested into a copy that lives as long as the pass
    vk::DMatView working(const DeviceTrace* t) {
        if (!t->nat.empty()) return t->nat.view();
        own_.emplace_back(&c_, t->height, t->width);
        vk::launch_ingest(stream, t->raw.data, own_.back().view(), false);
        return own_.back().view();
    }
    // the traces and the program of one chip's launch arguments (Args: the *Args structs of kernels/launch.hpp)
    template <class Args>
    void bind(Args& a, const DeviceTrace* main, const DeviceTrace* prep, const DBuf& prog) {
        const vk::DMatView v = working(main);
        a.main = v.data; a.mstride = v.stride;
        if (prep) { const vk::DMatView pv = working(prep); a.prep = pv.data; a.pstride = pv.stride; }
        a.prog = (const vair::Instr*)prog.data;
    }
    // device_ms is what lies between begin() and end(): each audit says where its pass begins
    void begin() { VG_HIP_CHECK(hipEventRecord(ev_.a, stream)); }
    template <class Report>
    void end(Report& rep) {
        VG_HIP_CHECK(hipEventRecord(ev_.b, stream));
        c_.sync();
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_.a, ev_.b) == hipSuccess) rep.device_ms = ms;
    }
};

// The kernels that keep one flag per constraint in registers handle CA_MAX_CONSTRAINTS of them.
inline void audit_refuse_constraints(const char* name, const AirDesc& air) {
    if (air.program.num_asserts > vk::CA_MAX_CONSTRAINTS)
        throw std::invalid_argument(std::string(name) + ": chip " + air.name + " has " + std::to_string(air.program.num_asserts) + " constraints; the device audit handles up to " +
                                    std::to_string(vk::CA_MAX_CONSTRAINTS) + " per chip (the host audit has no limit)");
}
// shape(): one of the *_shape functions of kernels/launch.hpp, which refuse a chip that does not fit the LDS; the refusal names the chip
template <class Shape>
void audit_chip_shape(const AirDesc& air, Shape&& shape) {
    try {
        shape();
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument(std::string(e.what()) + " [chip " + air.name + "; the host audit has no limit]");
    }
}
// the sizes of one chip's launch arguments and the evaluator the kernels take for it
template <class Args>
void audit_chip_sizes(Args& a, const AirDesc& air, uint64_t height, bool interpret_air) {
    a.K = air.program.num_asserts;
    a.n = height; a.width = air.width; a.prep_width = air.prep_width;
    a.n_instrs = (uint32_t)air.program.instrs.size();
    a.n_regs = air.program.num_regs;
    a.native_chip = !a.K ? vk::MA_BUS_ONLY : (interpret_air ? vk::CA_INTERPRET : air.native_chip);
}

// u64 k of a downloaded block of totals
inline uint64_t audit_u64(const std::vector<uint32_t>& tw, size_t k) { return ((uint64_t)tw[2 * k + 1] << 32) | tw[2 * k]; }

// The scratch of a counting pass, in u32 words: per chip its u64 totals and its table [entries x workgroups], zeroed before the counting
// launches; behind them every chip's prefix table of the same size, which the scan writes whole.
struct AuditScratch {
    std::vector<uint64_t> tot_at, tab_at, pre_at, table;
    std::vector<char> has;
    uint64_t zeroed = 0, words = 0;
    explicit AuditScratch(size_t NC) : tot_at(NC, 0), tab_at(NC, 0), pre_at(NC, 0), table(NC, 0), has(NC, 0) {}
    void add(size_t i, uint64_t totals_words, uint64_t table_words) {
        tot_at[i] = zeroed; zeroed += totals_words;
        tab_at[i] = zeroed; zeroed += (table_words + 1) & ~1ull;  // the next chip's u64 totals stay 8-byte aligned
        table[i] = table_words; has[i] = 1;
    }
    uint64_t place_prefixes() {
        words = zeroed;
        for (size_t i = 0; i < has.size(); i++) if (has[i]) { pre_at[i] = words; words += table[i]; }
        return words;
    }
};

// The entries of a report ascend by chip: fn(chip, e0, e1) for every run [e0, e1) of one chip's entries.
template <class Entry, class Fn>
void audit_chip_runs(const std::vector<Entry>& entries, Fn&& fn) {
    for (size_t e0 = 0; e0 < entries.size();) {
        const uint32_t chip = entries[e0].chip;
        size_t e1 = e0;
        while (e1 < entries.size() && entries[e1].chip == chip) e1++;
        fn(chip, e0, e1);
        e0 = e1;
    }
}

#pragma GCC visibility pop
}  // namespace vhost
