// Stand-alone host test of the dense lane (valida_amd/csrc/host/dense_lane.hpp) over a MOCK event API: no GPU, no HIP.
//   dense_lane_host [threads] [pairs per thread]
// THREADS threads, each owning a "context" (a slot), run enter / leave pairs; now and then a thread destroys its context (retire, drop the slot)
// and makes a new one, sometimes while it is the lane's tail.  The mock checks, on every call,
//   * a wait only ever targets an event that is alive and has been recorded before,
//   * no context waits on its own event,
// and the driver checks at the end that the order of the published tails equals the order in which the contexts acquired the lane.
// Built by tests/test_dense_lane_cpu.py with AddressSanitizer + UBSan and with ThreadSanitizer; exit status 0 = every check held.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../../valida_amd/csrc/host/dense_lane.hpp"

namespace {

std::atomic<long> g_failures{0};
std::atomic<long> g_waits{0}, g_records{0}, g_live_events{0};
void fail(const char* what) {
    g_failures.fetch_add(1);
    fprintf(stderr, "dense_lane_host: %s\n", what);
}

struct MockEvent {
    uint64_t owner;                 // the context that created it
    std::atomic<long> records{0};   // how often it has been recorded
    std::atomic<bool> alive{true};
    explicit MockEvent(uint64_t o) : owner(o) {}
};
// what the lane's critical section appends to: guarded by the lane's own mutex (held from enter to leave), which is part of what the
// ThreadSanitizer build checks
std::vector<uint64_t> g_tails;
thread_local uint64_t t_ctx = 0;    // the context the calling thread drives (the "stream" of the mock)

struct MockApi {
    using Event = MockEvent*;
    using Stream = uint64_t;
    static Event create() { g_live_events.fetch_add(1); return new MockEvent(t_ctx); }
    static void destroy(Event e) noexcept {
        e->alive.store(false);
        g_live_events.fetch_sub(1);
        delete e;  // a later use is a heap-use-after-free under AddressSanitizer
    }
    static bool record(Event e, Stream s) noexcept {
        if (!e->alive.load()) fail("record on a destroyed event");
        if (e->owner != s) fail("a context recorded another context's event");
        e->records.fetch_add(1);
        g_records.fetch_add(1);
        g_tails.push_back(s);
        return true;
    }
    static void wait(Stream s, Event e) {
        g_waits.fetch_add(1);
        if (!e->alive.load()) fail("wait on a destroyed event");
        if (e->records.load() < 1) fail("wait on an event that has not been recorded");
        if (e->owner == s) fail("a context waits on its own event");
    }
};
using Lane = vhost::DenseLane<MockApi>;

}  // namespace

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 4;
    const int pairs = argc > 2 ? atoi(argv[2]) : 2000;
    Lane lane;
    std::vector<uint64_t> acquired;  // appended under the lane (between enter and leave)
    std::atomic<uint64_t> next_ctx{1};
    std::atomic<long> destroyed{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            std::mt19937 rng(1234u + (unsigned)t);
            t_ctx = next_ctx.fetch_add(1);
            Lane::SlotPtr slot = std::make_shared<Lane::Slot>();
            for (int i = 0; i < pairs; i++) {
                {
                    Lane::Guard g = lane.enter(slot, t_ctx);
                    if (!g.held()) fail("enter returned a guard that does not hold the lane");
                    acquired.push_back(t_ctx);
                    if (rng() % 8 == 0) std::this_thread::yield();  // "enqueue the dense launches"
                    if (rng() % 16 == 0) {
                        g.leave();  // the explicit leave of the normal path; the destructor must then do nothing
                        g.leave();
                    }
                }  // the guard's destructor leaves on every other path
                if (rng() % 32 == 0) {  // destroy this context right after it left the lane (it is the tail unless another thread has taken the lane since) and go on with a new one
                    destroyed.fetch_add(1);
                    if (rng() % 2) lane.retire(slot);  // a context that drained its stream first; the other half just drops its reference
                    slot.reset();
                    t_ctx = next_ctx.fetch_add(1);
                    slot = std::make_shared<Lane::Slot>();
                }
            }
            lane.retire(slot);
        });
    for (auto& th : pool) th.join();
    const size_t want = (size_t)threads * (size_t)pairs;
    if (acquired.size() != want || g_tails.size() != want) fail("lost enter / leave pairs");
    else
        for (size_t i = 0; i < want; i++)
            if (acquired[i] != g_tails[i]) { fail("the tail order differs from the acquisition order"); break; }
    printf("dense_lane_host: %d threads x %d pairs, %ld waits, %ld records, %ld contexts destroyed, %ld failures\n", threads, pairs, g_waits.load(),
           g_records.load(), destroyed.load(), g_failures.load());
    return g_failures.load() ? 1 : 0;
}
