// Stand-alone check of mi355x_ddp/ops/csrc/shard_run.h (no HIP, torch or
// Python): the documented schedules, the bounds, and a randomized sequence
// of step / bind / flush calls against a naive model that keeps the whole
// history. Built with -fsanitize=address,undefined and run as a child
// process by tests/test_shard_run_native.py. Exit status 0 = all passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

#include "shard_run.h"

using Launches = std::vector<std::pair<int64_t, int64_t>>;
using Run = mi355x::ShardRun<std::function<void(int64_t, int64_t)>>;

static int g_failures = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,       \
                   __LINE__, #cond);                                    \
      ++g_failures;                                                     \
    }                                                                   \
  } while (0)

static std::vector<int64_t> sizes(const Launches& l, size_t since = 0) {
  std::vector<int64_t> out;
  for (size_t k = since; k < l.size(); ++k) out.push_back(l[k].second);
  return out;
}

static Run make(Launches& rec, int64_t bound, int64_t max_defer,
                int64_t ramp_first, double growth) {
  Run r([&rec](int64_t first, int64_t n) { rec.emplace_back(first, n); },
        max_defer, ramp_first, growth);
  r.bind(bound);
  return r;
}

static void schedules() {
  using V = std::vector<int64_t>;
  {  // unarmed: a new tracker launches at max_defer
    Launches rec;
    Run r = make(rec, 64, 16, 2, 2.0);
    for (int i = 0; i < 40; ++i) r.step(i);
    CHECK(r.pending() == 8);
    r.flush();
    CHECK((sizes(rec) == V{16, 16, 8}));
    CHECK(r.launch_count() == 3);
  }
  {  // armed by a public flush
    Launches rec;
    Run r = make(rec, 64, 16, 2, 2.0);
    r.flush();
    CHECK(rec.empty() && r.threshold() == 2);
    for (int i = 0; i < 40; ++i) r.step(i);
    r.flush();
    CHECK((sizes(rec) == V{2, 4, 8, 16, 10}));
    CHECK(rec[3].first == 14 && rec[3].second == 16);
  }
  {  // growth 3/2 rounds up
    Launches rec;
    Run r = make(rec, 100, 16, 2, 1.5);
    r.flush();
    for (int i = 0; i < 60; ++i) r.step(i);
    r.flush();
    CHECK((sizes(rec) == V{2, 3, 5, 8, 12, 16, 14}));
  }
  {  // ramp_first = 0: no ramp
    Launches rec;
    Run r = make(rec, 64, 16, 0, 2.0);
    r.flush();
    for (int i = 0; i < 40; ++i) r.step(i);
    r.flush();
    CHECK((sizes(rec) == V{16, 16, 8}));
  }
  {  // the internal flushes (re-bind, restart) do not arm
    Launches rec;
    Run r = make(rec, 64, 16, 2, 2.0);
    for (int i = 0; i < 5; ++i) r.step(i);
    r.bind(64);
    for (int i = 0; i < 10; ++i) r.step(i);
    for (int i = 3; i < 23; ++i) r.step(i);
    r.flush();
    CHECK((sizes(rec) == V{5, 10, 16, 4}));
  }
  {  // max_defer 1: every step is its own launch, restarts included
    Launches rec;
    Run r = make(rec, 8, 1, 0, 2.0);
    r.step(0);
    r.step(5);
    r.step(6);
    CHECK((sizes(rec) == V{1, 1, 1}) && r.pending() == 0);
  }
  {  // out of range: pending run launched, nothing for the bad index
    Launches rec;
    Run r = make(rec, 8, 16, 2, 2.0);
    for (int i = 0; i < 6; ++i) r.step(i);
    for (int64_t bad : {(int64_t)8, (int64_t)-1, INT64_MAX, INT64_MIN}) {
      bool threw = false;
      try {
        r.step(bad);
      } catch (const std::out_of_range&) {
        threw = true;
      }
      CHECK(threw && rec.size() == 1 && r.pending() == 0);
    }
    CHECK(!r.extend(8) && !r.extend(-1));
    r.step(6);
    CHECK(r.extend(7) && r.pending() == 2);
    bool threw = false;
    try {
      r.step(8);
    } catch (const std::out_of_range&) {
      threw = true;
    }
    CHECK(threw && (sizes(rec) == V{6, 2}));
  }
  {  // a launch that throws leaves the tracker consistent
    int calls = 0;
    Run r([&calls](int64_t, int64_t) {
            if (++calls == 1) throw std::runtime_error("launch failed");
          },
          4, 0, 2.0);
    r.bind(16);
    bool threw = false;
    try {
      for (int i = 0; i < 4; ++i) r.step(i);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw && r.pending() == 0);
    for (int i = 4; i < 8; ++i) r.step(i);
    CHECK(calls == 2 && r.pending() == 0);
  }
  for (int bad = 0; bad < 4; ++bad) {  // constructor arguments
    bool threw = false;
    try {
      Launches rec;
      Run r([](int64_t, int64_t) {}, bad == 0 ? 0 : 16, bad == 1 ? -1 : 2,
            bad == 2 ? 1.0 : bad == 3 ? 1e9 : 2.0);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
}

// Naive model: the list of executed steps, one entry per step, tagged with
// the number of the bind it ran under. The tracker must execute exactly
// the accepted steps, in order, under the bind that was current when each
// was accepted, in launches of at most max_defer steps inside the bound.
static void randomized(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&rng](int64_t lo, int64_t hi) {
    return std::uniform_int_distribution<int64_t>(lo, hi)(rng);
  };
  const int64_t max_defer = pick(1, 40);
  const int64_t ramp_first = pick(0, 12);
  const double growths[] = {1.25, 1.5, 2.0, 3.0};
  const double growth = growths[pick(0, 3)];

  std::vector<std::pair<int, int64_t>> want, got;  // (bind number, step)
  int bind_no = 0;
  int64_t bound = 0;
  bool ok_bounds = true;
  Run r([&](int64_t first, int64_t n) {
          if (n < 1 || n > max_defer || first < 0 || first + n > bound)
            ok_bounds = false;
          for (int64_t i = first; i < first + n; ++i)
            got.emplace_back(bind_no, i);
        },
        max_defer, ramp_first, growth);

  int64_t next = 0;
  for (int op = 0; op < 600; ++op) {
    const int64_t what = pick(0, 99);
    if (what < 4 || bound == 0) {  // (re-)bind: pending runs on the OLD one
      const int64_t nb = pick(0, 60);
      r.bind(nb);  // the launch callable still sees the old bind_no/bound
      ++bind_no;
      bound = nb;
      next = 0;
    } else if (what < 10) {
      r.flush();
      CHECK(r.pending() == 0);
    } else if (what < 14) {
      r.launch_pending();
      CHECK(r.pending() == 0);
    } else {
      int64_t i = next;
      if (what < 24) i = pick(-2, bound + 2);  // a jump, maybe out of range
      const bool in_range = i >= 0 && i < bound;
      bool threw = false;
      try {
        if (pick(0, 1) == 0 || !r.extend(i)) r.step(i);
      } catch (const std::out_of_range&) {
        threw = true;
      }
      CHECK(threw == !in_range);
      if (in_range) {
        want.emplace_back(bind_no, i);
        next = i + 1;
      } else {
        CHECK(r.pending() == 0);
      }
    }
    CHECK(r.pending() >= 0 && r.pending() < std::max<int64_t>(max_defer, 2));
    CHECK(r.threshold() >= 1 && r.threshold() <= max_defer);
  }
  r.flush();
  CHECK(ok_bounds);
  CHECK(got == want);
  if (got != want)
    std::fprintf(stderr, "seed %llu: executed %zu steps, wanted %zu\n",
                 (unsigned long long)seed, got.size(), want.size());
}

int main() {
  schedules();
  for (uint64_t seed = 1; seed <= 300; ++seed) randomized(seed);
  if (g_failures) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  std::puts("shard_run_check: ok");
  return 0;
}
