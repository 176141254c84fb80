"""Host cost per step of the shard-bound driving loop, without a GPU.

The fp32 chain kernel runs a step in about 180 ns, so the loop that feeds
it — bench.drive_shard_bound calling the engine's step_shard once per step
— has to be clearly faster than that or the GPU waits for the host. This
tool times that loop, driven exactly as bench.py drives it, against

- the Python closure the engine used before the native stepper (kept here
  as the reference), and
- the native stepper's recorder (ToyShardRun.recorder: the same tracker and
  the same C entry point as the real one, launches only noted).

    python tools/bench_host_loop.py [--steps 30000] [--spe 64] [--eb 16]

Prints ns/step for both, best of 7, and one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the driver under test: bench.drive_shard_bound)


class _Data:
    """What drive_shard_bound needs of bench.DeviceData, with no tensors."""

    def __init__(self):
        self.bound_epoch = -1
        self.bound_block = -1

    def shard_for(self, e):
        return None, None

    def shards_for_block(self, e0, epochs):
        return None, None


def closure_engine(max_defer):
    """The tracker PersistentToyStep had before the native stepper:
    closures over nonlocal counters; a launch only counts. Also the oracle
    of the unramped schedule in tests/test_shard_run.py."""
    launches = []
    s_start = s_next = 0

    def bind_shard(xs, ts, batch):
        nonlocal s_start, s_next
        flush()
        s_start = s_next = 0

    def step_shard(i):
        nonlocal s_start, s_next
        if i == s_next:
            s_next += 1
            if s_next - s_start >= max_defer:
                flush()
            return
        flush()
        s_start, s_next = i, i + 1

    def flush():
        nonlocal s_start, s_next
        if s_next > s_start:
            launches.append((s_start, s_next - s_start))
            s_start = s_next

    return bind_shard, step_shard, flush, launches


def native_engine(steps_bound, max_defer, ramp_first, growth):
    from mi355x_ddp import ops
    run = ops.ext().ToyShardRun.recorder(steps_bound, max_defer, ramp_first,
                                         growth)

    def bind_shard(xs, ts, batch):
        run.bind_steps(steps_bound)

    return bind_shard, run.step_shard, run.flush, run


def time_loop(make, spe, eb, batch, steps, repeats=7):
    best = float("inf")
    for _ in range(repeats):
        bind, step_shard, flush, _ = make()
        data = _Data()
        t0 = time.perf_counter()
        bench.drive_shard_bound(data, spe, batch, eb, bind, step_shard, 0,
                                steps)
        flush()
        best = min(best, time.perf_counter() - t0)
    return best / steps * 1e9


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30000)
    p.add_argument("--spe", type=int, default=64)
    p.add_argument("--eb", type=int, default=16)
    p.add_argument("--max-defer", type=int, default=1024)
    p.add_argument("--ramp-first", type=int, default=64)
    p.add_argument("--growth", type=float, default=1.5)
    a = p.parse_args()

    closure = time_loop(lambda: closure_engine(a.max_defer), a.spe, a.eb, 32,
                        a.steps)
    native = time_loop(
        lambda: native_engine(a.spe * a.eb, a.max_defer, a.ramp_first,
                              a.growth), a.spe, a.eb, 32, a.steps)
    print(f"closure step_shard: {closure:7.1f} ns/step")
    print(f"native  step_shard: {native:7.1f} ns/step")
    print(json.dumps({"steps": a.steps, "spe": a.spe, "eb": a.eb,
                      "closure_ns_per_step": round(closure, 1),
                      "native_ns_per_step": round(native, 1)}))


if __name__ == "__main__":
    main()
