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

// -- the tensor-level run ---------------------------------------------------
using mi355x::Span;
using SpanLaunches = std::vector<std::pair<Span, int64_t>>;
using Spans = mi355x::SpanRun<std::function<void(const Span&, int64_t)>>;

// Two pretend buffers per operand, adjacent in address: buffer 1 starts at
// the byte where buffer 0 ends. Only the identity tells them apart.
static const char kBufId[4] = {};
static constexpr uintptr_t kXBase = 0x100000, kTBase = 0x900000;
static constexpr int64_t kBufSteps = 64;  // steps of the widest shape

// a [rows, 8] f32 step of buffer `buf` at the given addresses
static Span span_at(int buf, int64_t rows, uintptr_t x, uintptr_t t) {
  Span s;
  s.x = x;
  s.t = t;
  s.x_bytes = rows * 8 * 4;
  s.t_bytes = rows * 4;
  s.rows = rows;
  s.cols = 8;
  s.dtype = 7;
  s.x_buf = &kBufId[buf];
  s.t_buf = &kBufId[2 + buf];
  return s;
}

static bool same_span(const Span& a, const Span& b) {
  return a.x == b.x && a.t == b.t && a.x_bytes == b.x_bytes &&
         a.t_bytes == b.t_bytes && a.rows == b.rows && a.cols == b.cols &&
         a.dtype == b.dtype && a.x_buf == b.x_buf && a.t_buf == b.t_buf;
}

// step k of a launched run, as the kernel will address it
static Span kth(const Span& first, int64_t k) {
  Span s = first;
  s.x += (uintptr_t)(k * first.x_bytes);
  s.t += (uintptr_t)(k * first.t_bytes);
  return s;
}

static void adjacent_buffers_do_not_merge() {
  SpanLaunches rec;
  Spans r([&rec](const Span& f, int64_t n) { rec.emplace_back(f, n); }, 16);
  const int64_t rows = 4;
  const Span last0 = span_at(0, rows, kXBase + 10 * rows * 32,
                             kTBase + 10 * rows * 4);
  // buffer 1 begins exactly where that span ends, in x and in t
  const Span first1 = span_at(1, rows, last0.x + (uintptr_t)last0.x_bytes,
                              last0.t + (uintptr_t)last0.t_bytes);
  r.step(last0);
  CHECK(!r.continues(first1));
  r.step(first1);
  r.launch_pending();
  CHECK(rec.size() == 2 && rec[0].second == 1 && rec[1].second == 1);
  CHECK(r.launch_count() == 2);
  // the same addresses in ONE buffer do merge
  rec.clear();
  Span same = first1;
  same.x_buf = last0.x_buf;
  same.t_buf = last0.t_buf;
  r.step(last0);
  CHECK(r.continues(same));
  r.step(same);
  r.launch_pending();
  CHECK(rec.size() == 1 && rec[0].second == 2);
  // x in the same buffer, t in another: no merge either
  rec.clear();
  same.t_buf = first1.t_buf;
  r.step(last0);
  r.step(same);
  r.launch_pending();
  CHECK(rec.size() == 2);
}

// Naive model of the span run: the submitted spans in order, with a cut
// mark where a launch boundary is due (a span that does not continue the
// one before it, max_defer reached, a flush). The tracker must launch
// exactly those groups.
static void randomized_spans(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&rng](int64_t lo, int64_t hi) {
    return std::uniform_int_distribution<int64_t>(lo, hi)(rng);
  };
  const int64_t max_defer = pick(1, 12);
  SpanLaunches rec;
  Spans r([&rec](const Span& f, int64_t n) { rec.emplace_back(f, n); },
          max_defer);

  std::vector<Span> want;           // every submitted span
  std::vector<int64_t> want_sizes;  // the groups they must be launched in
  int64_t group = 0;                // spans of the group being built
  auto cut = [&] {
    if (group) want_sizes.push_back(group);
    group = 0;
  };
  int buf = 0;
  int64_t rows = 4;
  uintptr_t x = kXBase, t = kTBase;  // where the next contiguous span starts
  for (int op = 0; op < 400; ++op) {
    const int64_t what = pick(0, 99);
    if (what < 6) {  // flush
      r.launch_pending();
      CHECK(r.pending() == 0);
      cut();
      continue;
    }
    bool contiguous = true;
    if (what < 14) {  // a gap: skip one step
      x += (uintptr_t)(rows * 32);
      t += (uintptr_t)(rows * 4);
      contiguous = false;
    } else if (what < 22) {  // another shape at the contiguous address
      rows = rows == 4 ? 2 : 4;
      contiguous = false;
    } else if (what < 28) {  // the other buffer, at its first byte
      buf ^= 1;
      x = kXBase + (uintptr_t)(buf * kBufSteps * 4 * 32);
      t = kTBase + (uintptr_t)(buf * kBufSteps * 4 * 4);
      contiguous = false;
    } else if (what < 32) {  // a gap in t only
      t += (uintptr_t)(rows * 4);
      contiguous = false;
    }
    const Span s = span_at(buf, rows, x, t);
    CHECK(r.continues(s) == (contiguous && group > 0));
    if (!contiguous) cut();
    r.step(s);
    want.push_back(s);
    if (++group >= max_defer) cut();
    CHECK(r.pending() == group);
    x += (uintptr_t)s.x_bytes;
    t += (uintptr_t)s.t_bytes;
  }
  r.launch_pending();
  cut();
  std::vector<int64_t> got_sizes;
  std::vector<Span> got;
  for (const auto& l : rec) {
    got_sizes.push_back(l.second);
    for (int64_t k = 0; k < l.second; ++k) got.push_back(kth(l.first, k));
  }
  CHECK(got_sizes == want_sizes);
  CHECK(r.launch_count() == (int64_t)rec.size());
  CHECK(got.size() == want.size());
  for (size_t k = 0; k < got.size() && k < want.size(); ++k)
    CHECK(same_span(got[k], want[k]));
}

// The ordering rule of OrderedRuns: over random interleavings of index
// steps, spans, binds and flushes, the launch stream expanded to steps is
// the submission order.
static void randomized_ordering(uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&rng](int64_t lo, int64_t hi) {
    return std::uniform_int_distribution<int64_t>(lo, hi)(rng);
  };
  const int64_t max_defer = pick(1, 20);
  const int64_t ramp_first = pick(0, 6);
  // a step: (bind number, index) of an index step, (-1, x address) of a span
  std::vector<std::pair<int64_t, int64_t>> want, got;
  int64_t bind_no = 0, bound = 0;
  bool ok = true;
  using Runs = mi355x::OrderedRuns<std::function<void(int64_t, int64_t)>,
                                   std::function<void(const Span&, int64_t)>>;
  Runs runs(
      [&](int64_t first, int64_t n) {
        if (n < 1 || n > max_defer || first < 0 || first + n > bound)
          ok = false;
        for (int64_t i = first; i < first + n; ++i)
          got.emplace_back(bind_no, i);
      },
      [&](const Span& f, int64_t n) {
        if (n < 1 || n > max_defer) ok = false;
        for (int64_t k = 0; k < n; ++k)
          got.emplace_back(-1, (int64_t)kth(f, k).x);
      },
      max_defer, ramp_first, 2.0);

  int64_t next = 0;
  uintptr_t x = kXBase, t = kTBase;
  for (int op = 0; op < 500; ++op) {
    const int64_t what = pick(0, 99);
    if (what < 4 || bound == 0) {
      const int64_t nb = pick(1, 50);
      runs.bind(nb);  // the launches it makes still belong to the old bind
      ++bind_no;
      bound = nb;
      next = 0;
      CHECK(runs.index().pending() == 0 && runs.spans().pending() == 0);
    } else if (what < 9) {
      runs.flush();
      CHECK(runs.index().pending() == 0 && runs.spans().pending() == 0);
    } else if (what < 12) {
      runs.launch_pending();
      CHECK(runs.index().pending() == 0 && runs.spans().pending() == 0);
    } else if (what < 55) {  // index step, now and then a jump
      int64_t i = what < 18 ? pick(0, bound - 1) : next;
      if (i >= bound) i = 0;
      if (pick(0, 1) == 0 || !runs.index().extend(i)) runs.index().step(i);
      want.emplace_back(bind_no, i);
      next = i + 1;
    } else {  // span, now and then after a gap
      if (what < 62) {
        x += 128;
        t += 16;
      }
      const Span s = span_at(0, 4, x, t);
      const bool extends = runs.continues(s);
      const int64_t before = runs.spans().pending();
      runs.step_span(s);
      if (extends) CHECK(runs.spans().pending() == (before + 1) % max_defer);
      want.emplace_back(-1, (int64_t)s.x);
      x += (uintptr_t)s.x_bytes;
      t += (uintptr_t)s.t_bytes;
    }
  }
  runs.flush();
  CHECK(ok);
  CHECK(got == want);
  CHECK(runs.launch_count() ==
        runs.index().launch_count() + runs.spans().launch_count());
  if (got != want)
    std::fprintf(stderr, "ordering seed %llu: executed %zu steps of %zu\n",
                 (unsigned long long)seed, got.size(), want.size());
}

int main() {
  schedules();
  for (uint64_t seed = 1; seed <= 300; ++seed) randomized(seed);
  adjacent_buffers_do_not_merge();
  for (uint64_t seed = 1; seed <= 200; ++seed) randomized_spans(seed);
  for (uint64_t seed = 1; seed <= 200; ++seed) randomized_ordering(seed);
  if (g_failures) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  std::puts("shard_run_check: ok");
  return 0;
}
