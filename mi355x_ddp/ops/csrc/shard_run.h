// Run tracker and launch schedule of the shard-bound stepper.
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

}  // namespace mi355x
