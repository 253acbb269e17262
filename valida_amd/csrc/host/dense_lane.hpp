// The dense lane: one per device and process, shared by every prover context of that device.  A proof's big Merkle-tree launches (a thread
// per node over >= 2^18 rows) fill the VALU issue slots of the whole chip on their own; two of them side by side only stretch each other.
// A context ENTERS the lane before the first such launch of a tree and LEAVES it behind the last one: entering makes its stream wait for
// the event the previous user recorded when it left, so at most one proof is in its dense tree phase on the GPU at a time, while the other
// proofs' LDE, quotient, opening and latency-bound launches run beside it.
//
// Nothing here blocks on the GPU, creates a stream or touches a hardware queue: entering enqueues one stream wait, leaving records one event.
// The lane's mutex is held from enter to leave, i.e. across the ENQUEUE of one tree's dense launches: a few launch calls and the pool allocations of
// their output layers.  That is host-side exclusion between the proof threads of one device, normally microseconds; it lasts longer when an allocation
// misses the pool and reaches hipMalloc (the first proof of a shape) or a launch call blocks on a full queue, and then another context's enter() waits
// on the host for that long.  It cannot deadlock (the holder waits for nothing another context enqueues later) and never idles the GPU.  It is held so that
//   * the order in which contexts acquire the lane is the order of the tails they publish, and
//   * INVARIANT: a wait is only ever enqueued on an event that has ALREADY been recorded (the tail is published by the same critical section
//     that recorded it).  The dependency graph between the streams is therefore ordered by enqueue time and cannot form a cycle.
// A context never waits on its own event (its stream already orders its launches).  The tail is held by shared ownership: the event of a
// context that is destroyed while it is the tail stays valid, completed or completing, until another context replaces it.
//
// The event API is a template policy so that the logic can be driven by a mock on the host (tests/emu/dense_lane_host.cpp).
#pragma once
#include <memory>
#include <mutex>

namespace vhost {

template <class Api>
class DenseLane {
  public:
    using Event = typename Api::Event;
    using Stream = typename Api::Stream;
    // a context's own lane event; destroyed when neither the context nor the lane's tail refers to it any more
    struct Slot {
        Event ev;
        Slot() : ev(Api::create()) {}
        ~Slot() { Api::destroy(ev); }
        Slot(const Slot&) = delete;
        Slot& operator=(const Slot&) = delete;
    };
    using SlotPtr = std::shared_ptr<Slot>;

    // Holds the lane from enter() until leave() or destruction (every path out of a build, a throwing launch included).
    class Guard {
      public:
        Guard() = default;
        Guard(Guard&& o) noexcept : lane_(o.lane_), self_(std::move(o.self_)), stream_(o.stream_), waited_(o.waited_), lk_(std::move(o.lk_)) { o.lane_ = nullptr; }
        Guard& operator=(Guard&& o) noexcept {
            if (this != &o) { leave(); lane_ = o.lane_; self_ = std::move(o.self_); stream_ = o.stream_; waited_ = o.waited_; lk_ = std::move(o.lk_); o.lane_ = nullptr; }
            return *this;
        }
        ~Guard() { leave(); }
        bool held() const { return lane_ != nullptr; }
        bool waited() const { return waited_; }  // entering enqueued a wait on another context's event
        // record this context's event behind the dense launches and publish it as the new tail.  A record that fails publishes nothing: the
        // old tail (recorded earlier) stays, and the launch error itself is reported by the caller's own checks.
        void leave() noexcept {
            if (!lane_) return;
            if (Api::record(self_->ev, stream_)) lane_->tail_ = self_;
            lane_ = nullptr;
            self_.reset();
            lk_.unlock();
        }

      private:
        friend class DenseLane;
        DenseLane* lane_ = nullptr;
        SlotPtr self_;
        Stream stream_{};
        bool waited_ = false;
        std::unique_lock<std::mutex> lk_;
    };

    // `self`: the calling context's slot; `stream`: the stream its dense launches are enqueued on
    Guard enter(const SlotPtr& self, Stream stream) {
        Guard g;
        g.lk_ = std::unique_lock<std::mutex>(mu_);
        if (tail_ && tail_ != self) {
            Api::wait(stream, tail_->ev);  // may throw: the lock unwinds, the tail is unchanged
            g.waited_ = true;
        }
        g.lane_ = this;
        g.self_ = self;
        g.stream_ = stream;
        return g;
    }
    // A context on its way out, AFTER it has drained its stream: if it is the tail there is nothing left to wait for.
    void retire(const SlotPtr& self) noexcept {
        std::lock_guard<std::mutex> lk(mu_);
        if (tail_ == self) tail_.reset();
    }

  private:
    std::mutex mu_;
    SlotPtr tail_;
};

}  // namespace vhost
