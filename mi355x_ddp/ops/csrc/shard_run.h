// Run trackers and launch schedule of the persistent engine: ShardRun (the
// shard-bound stepper's index run, described here), SpanRun (the run of
// step(x, t) tensors) and OrderedRuns (both, in submission order), below.
//
// A caller steps through a bound shard by batch INDEX. Consecutive indices
// extend one pending run [s_start, s_next); the run is handed to
// launch(first_step, n_steps) when it reaches the current threshold, when a
// non-consecutive index arrives, on a re-bind and on flush(). Splitting a
// run over several launches never changes what is computed, only when.
//
// Threshold: max_defer, except after a public flush(). The caller flushes
// because it is about to synchronize, so the next run starts on an idle
// device; waiting max_defer steps before the first launch would leave it
// idle all that time. flush() therefore ARMS a ramp: the threshold restarts
// at ramp_first and after each launch becomes
// min(max_defer, ceil(threshold * growth)), until it reaches max_defer.
// The device stays fed only while the host counts `growth` times the steps
// of the launch in flight before that launch ends, i.e. while
// growth <= kernel time per step / host time per step.
// The flushes inside bind() and a non-consecutive step() do not arm, nor is
// a new tracker armed. ramp_first = 0 disables the ramp.
//
// Plain C++17 on purpose (no HIP, torch or Python headers): the schedule is
// tested in a stand-alone host program under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

namespace mi355x {

template <typename Launch>
class ShardRun {
 public:
  ShardRun(Launch launch, int64_t max_defer, int64_t ramp_first, double growth)
      : launch_(std::move(launch)), max_defer_(max_defer),
        ramp_first_(ramp_first), growth_(growth) {
    if (max_defer < 1) throw std::invalid_argument("max_defer must be >= 1");
    if (ramp_first < 0) throw std::invalid_argument("ramp_first must be >= 0");
    if (ramp_first > 0 && !(growth > 1.0 && growth <= 1024.0))
      throw std::invalid_argument("ramp growth must be in (1, 1024]");
  }

  // Launches what is pending, then tracks a buffer of `steps_bound` steps
  // from [0, 0). Does not arm.
  void bind(int64_t steps_bound) {
    if (steps_bound < 0) throw std::invalid_argument("steps_bound < 0");
    launch_pending();
    steps_bound_ = steps_bound;
    s_start_ = s_next_ = 0;
  }

  // Step `i` of the bound buffer. An index outside it launches the pending
  // run and throws before anything is launched for `i`.
  void step(int64_t i) {
    if (i == s_next_ && i < steps_bound_) {
      ++s_next_;
      if (s_next_ - s_start_ >= threshold_) launch_pending();
      return;
    }
    launch_pending();
    if (i < 0 || i >= steps_bound_)
      throw std::out_of_range("step index " + std::to_string(i) +
                              " is outside the bound shard of " +
                              std::to_string(steps_bound_) + " steps");
    s_start_ = i;
    s_next_ = i + 1;
    if (threshold_ <= 1) launch_pending();
  }

  // step(i) for the common case alone: true if `i` extended the pending
  // run and no launch is due, so nothing can throw; false (and nothing
  // done) otherwise. Lets a caller keep its exception handling off the
  // per-step path.
  bool extend(int64_t i) noexcept {
    if (i != s_next_ || i >= steps_bound_ ||
        s_next_ + 1 - s_start_ >= threshold_)
      return false;
    ++s_next_;
    return true;
  }

  // Launches what is pending without arming (re-bind, restart, a caller
  // that orders other work behind the run).
  void launch_pending() {
    const int64_t first = s_start_, n = s_next_ - s_start_;
    if (n <= 0) return;
    s_start_ = s_next_;  // before the call: consistent if launch_ throws
    ++launch_count_;
    if (threshold_ < max_defer_) {  // ramping
      const double next = std::ceil((double)threshold_ * growth_);
      threshold_ = next >= (double)max_defer_ ? max_defer_ : (int64_t)next;
    }
    launch_(first, n);
  }

  // Launches what is pending and arms the ramp: the caller is about to
  // synchronize, so the next run meets an idle device.
  void flush() {
    launch_pending();
    threshold_ = ramp_first_ > 0 && ramp_first_ < max_defer_ ? ramp_first_
                                                            : max_defer_;
  }

  int64_t pending() const { return s_next_ - s_start_; }
  int64_t launch_count() const { return launch_count_; }
  int64_t max_defer() const { return max_defer_; }
  int64_t threshold() const { return threshold_; }
  int64_t steps_bound() const { return steps_bound_; }

 private:
  Launch launch_;
  const int64_t max_defer_, ramp_first_;
  const double growth_;
  int64_t threshold_ = max_defer_;  // < max_defer_ exactly while ramping
  int64_t steps_bound_ = 0;
  int64_t s_start_ = 0, s_next_ = 0;  // pending run [s_start_, s_next_)
  int64_t launch_count_ = 0;
};

// The tensor-level run: a caller that steps by (x, t) tensors instead of
// indices. A span is one step's x and t as addresses; consecutive spans that
// lie back to back in memory extend one pending run, handed to
// launch(first_span, n_steps) when it reaches max_defer, when a span arrives
// that does not extend it, and by launch_pending(). No ramp, never armed.
struct Span {
  uintptr_t x = 0, t = 0;            // addresses of the step's x and t
  int64_t x_bytes = 0, t_bytes = 0;  // their sizes: the run's per-step strides
  int64_t rows = 0, cols = 0;        // shape of x
  int64_t dtype = 0;                 // opaque code of the element types
  // Opaque identities of the buffers x and t lie in. Only the run's first
  // span is kept alive by the caller, so a span of another buffer must not
  // extend the run even where the two allocations happen to be adjacent.
  const void* x_buf = nullptr;
  const void* t_buf = nullptr;
};

template <typename Launch>
class SpanRun {
 public:
  SpanRun(Launch launch, int64_t max_defer)
      : launch_(std::move(launch)), max_defer_(max_defer) {
    if (max_defer < 1) throw std::invalid_argument("max_defer must be >= 1");
  }

  // `s` starts exactly where the pending run ends, with the first span's
  // shape and dtype, in the first span's buffers.
  bool continues(const Span& s) const noexcept {
    const Span& f = first_;
    return count_ > 0 && s.x == f.x + (uintptr_t)(count_ * f.x_bytes) &&
           s.t == f.t + (uintptr_t)(count_ * f.t_bytes) &&
           s.x_bytes == f.x_bytes && s.t_bytes == f.t_bytes &&
           s.rows == f.rows && s.cols == f.cols && s.dtype == f.dtype &&
           s.x_buf == f.x_buf && s.t_buf == f.t_buf;
  }

  void step(const Span& s) {
    if (!continues(s)) {
      launch_pending();
      first_ = s;
    }
    if (++count_ >= max_defer_) launch_pending();
  }

  void launch_pending() {
    const int64_t n = count_;
    if (n == 0) return;
    count_ = 0;  // before the call: consistent if launch_ throws
    ++launch_count_;
    launch_(first_, n);
  }

  int64_t pending() const { return count_; }
  int64_t launch_count() const { return launch_count_; }

 private:
  Launch launch_;
  const int64_t max_defer_;
  Span first_;
  int64_t count_ = 0;
  int64_t launch_count_ = 0;
};

// Both runs of one engine. Whatever the interleaving of index steps, spans,
// binds and flushes, the steps execute in the order they were submitted:
//   - at most one run of each kind is pending;
//   - if both are pending, the span run is the older one. So a span launches
//     a pending index run (and the span run before it) and starts a new run,
//     and the index run's launch callable launches a pending span run first;
//   - bind, launch_pending and flush launch the span run, then the index
//     run; flush then arms the index run's ramp.
// Index steps go to index() directly: a step that only extends the index
// run touches nothing here.
template <typename IndexLaunch, typename SpanLaunch>
class OrderedRuns {
  struct OlderFirst {
    OrderedRuns* self;
    void operator()(int64_t first, int64_t n) const {
      self->spans_.launch_pending();
      self->index_launch_(first, n);
    }
  };

 public:
  OrderedRuns(IndexLaunch index_launch, SpanLaunch span_launch,
              int64_t max_defer, int64_t ramp_first, double growth)
      : index_launch_(std::move(index_launch)),
        spans_(std::move(span_launch), max_defer),
        index_(OlderFirst{this}, max_defer, ramp_first, growth) {}
  OrderedRuns(const OrderedRuns&) = delete;  // index_ points back here
  OrderedRuns& operator=(const OrderedRuns&) = delete;

  ShardRun<OlderFirst>& index() { return index_; }
  const SpanRun<SpanLaunch>& spans() const { return spans_; }

  // `s` would only extend the pending span run: nothing gets launched, so a
  // caller has nothing to validate or to keep alive for it.
  bool continues(const Span& s) const noexcept {
    return index_.pending() == 0 && spans_.continues(s);
  }

  void step_span(const Span& s) {
    if (!continues(s)) launch_pending();
    spans_.step(s);
  }

  void bind(int64_t steps_bound) {
    if (steps_bound < 0) throw std::invalid_argument("steps_bound < 0");
    launch_pending();
    index_.bind(steps_bound);
  }

  void launch_pending() {
    spans_.launch_pending();
    index_.launch_pending();
  }

  void flush() {
    spans_.launch_pending();
    index_.flush();
  }

  int64_t launch_count() const {
    return index_.launch_count() + spans_.launch_count();
  }

 private:
  IndexLaunch index_launch_;
  SpanRun<SpanLaunch> spans_;
  ShardRun<OlderFirst> index_;
};

}  // namespace mi355x
