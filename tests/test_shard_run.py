"""CPU tests of the native shard-bound stepper's schedule, through its
recorder: the tracker and the step_shard C entry point are the ones the
GPU engine uses, the launch callable only notes (first_step, n_steps)."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from mi355x_ddp import _C
except ImportError:  # pragma: no cover
    _C = None

pytestmark = pytest.mark.skipif(_C is None,
                                reason="mi355x_ddp._C is not built")


def _rec(steps_bound=64, max_defer=16, ramp_first=2, growth=2.0):
    return _C.ToyShardRun.recorder(steps_bound, max_defer, ramp_first, growth)


def _sizes(run, since=0):
    return [n for _, n in run.launches[since:]]


def _covered(launches):
    return [i for first, n in launches for i in range(first, first + n)]


def test_unarmed_schedule():
    run = _rec()
    step = run.step_shard
    for i in range(40):
        step(i)
    assert run.pending == 8
    run.flush()
    assert run.launches == [(0, 16), (16, 16), (32, 8)]
    assert run.launch_count == 3 and run.pending == 0
    assert run.max_defer == 16


def test_armed_schedule():
    run = _rec()
    run.flush()  # nothing pending: launches nothing, arms
    assert run.launches == []
    for i in range(40):
        run.step_shard(i)
    run.flush()
    assert run.launches == [(0, 2), (2, 4), (6, 8), (14, 16), (30, 10)]
    # the flush armed again: the next run ramps from ramp_first once more
    for i in range(40, 50):
        run.step_shard(i)
    run.flush()
    assert _sizes(run, 5) == [2, 4, 4]


def test_growth_three_halves_rounds_up():
    run = _rec(steps_bound=100, max_defer=16, ramp_first=2, growth=1.5)
    run.flush()
    for i in range(60):
        run.step_shard(i)
    run.flush()
    assert _sizes(run) == [2, 3, 5, 8, 12, 16, 14]


def test_ramp_first_zero_disables_the_ramp():
    run = _rec(ramp_first=0)
    run.flush()
    for i in range(40):
        run.step_shard(i)
    run.flush()
    assert _sizes(run) == [16, 16, 8]


def test_ramp_first_at_or_above_max_defer_is_no_ramp():
    run = _rec(max_defer=16, ramp_first=16)
    run.flush()
    for i in range(40):
        run.step_shard(i)
    run.flush()
    assert _sizes(run) == [16, 16, 8]


def test_rebind_launches_the_rest_and_does_not_arm():
    run = _rec()
    for i in range(5):
        run.step_shard(i)
    run.bind_steps(64)  # re-bind mid-run
    assert run.launches == [(0, 5)]
    for i in range(20):
        run.step_shard(i)
    assert run.launches[1:] == [(0, 16)]  # not 2, 4, 8: not armed
    assert run.pending == 4


def test_nonsequential_index_launches_the_rest_and_does_not_arm():
    run = _rec()
    for i in range(10):
        run.step_shard(i)
    for i in range(3, 23):
        run.step_shard(i)
    run.flush()
    assert run.launches == [(0, 10), (3, 16), (19, 4)]


def test_internal_flush_while_ramping_keeps_the_ramp_going():
    run = _rec()
    run.flush()
    for i in range(3):      # 2 launched, 1 pending, threshold now 4
        run.step_shard(i)
    run.bind_steps(64)      # launches the 1; the threshold moves on to 8
    for i in range(30):
        run.step_shard(i)
    run.flush()
    assert run.launches == [(0, 2), (2, 1), (0, 8), (8, 16), (24, 6)]


def test_out_of_range_index():
    run = _rec(steps_bound=8)
    for i in range(6):
        run.step_shard(i)
    for bad in (8, 9, -1, 2 ** 40, 2 ** 80):
        with pytest.raises(IndexError):
            run.step_shard(bad)
        # the run that was pending is launched, nothing for the bad index
        assert run.launches == [(0, 6)]
        assert run.pending == 0
    # the tracker is still usable: the last in-range steps
    run.step_shard(6)
    run.step_shard(7)
    with pytest.raises(IndexError):
        run.step_shard(8)  # sequential, but one past the end
    assert run.launches == [(0, 6), (6, 2)]
    assert max(_covered(run.launches)) == 7


def test_step_before_any_bind_is_out_of_range():
    run = _rec(steps_bound=0)
    with pytest.raises(IndexError):
        run.step_shard(0)
    assert run.launches == []


@pytest.mark.parametrize("arg", [1.0, "3", None, (1,), [2]])
def test_non_int_argument(arg):
    run = _rec()
    run.step_shard(0)
    with pytest.raises(TypeError):
        run.step_shard(arg)
    assert run.pending == 1 and run.launches == []
    with pytest.raises(TypeError):
        run.step_shard()  # METH_O: exactly one argument


def test_step_function_outlives_the_python_handle():
    run = _rec()
    step = run.step_shard
    del run
    for i in range(16):
        step(i)  # the function owns the run
    assert step.__name__ == "step_shard"


def test_bad_constructor_arguments():
    for kw in (dict(max_defer=0), dict(ramp_first=-1), dict(growth=1.0),
               dict(growth=0.5), dict(growth=float("nan"))):
        with pytest.raises(ValueError):
            _rec(**kw)
    _rec(ramp_first=0, growth=1.0)  # growth is unused without a ramp


# -- the mesh schedule, and the tensor-level run ---------------------------
def test_unramped_schedule_equals_the_closure_tracker_it_replaced():
    """With a mesh the engine runs this tracker with ramp_first = 0 where it
    ran a Python closure tracker before. Every rank must keep issuing the
    same launches, so the two must cut any in-range sequence of steps, binds
    and flushes into the same launches. max_defer >= 2: at 1 the closure
    launched a restarted run only with its second step, (5, 2) for steps
    5, 6, which a max_defer of 1 does not allow."""
    import random
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_host_loop import closure_engine

    rng = random.Random(20)
    for trial in range(150):
        md = rng.choice([2, 3, 5, 16, 64])
        bound = rng.randrange(1, 80)
        run = _rec(steps_bound=bound, max_defer=md, ramp_first=0)
        bind, step, flush, want = closure_engine(md)
        nxt = 0
        for _ in range(rng.randrange(1, 300)):
            r = rng.random()
            if r < 0.03:
                bound = rng.randrange(1, 80)
                run.bind_steps(bound)
                bind(None, None, 32)
                nxt = 0
            elif r < 0.08:
                run.flush()
                flush()
            else:
                i = nxt if r > 0.2 and nxt < bound else rng.randrange(bound)
                run.step_shard(i)
                step(i)
                nxt = i + 1
        run.flush()
        flush()
        assert run.launches == want, (trial, md)
        assert run.launch_count == len(want)


def _tiles(n=48, rows=4, cols=3):
    import torch
    X = torch.zeros(n * rows, cols)
    T = torch.zeros(n * rows, 1)
    return [(X[i * rows:(i + 1) * rows], T[i * rows:(i + 1) * rows])
            for i in range(n)]


def _expand(launches, x_bytes):
    """The recorded launches as steps: ("s", index) and ("t", x address)."""
    out = []
    for l in launches:
        if l[0] == "t":
            out += [("t", l[1] + k * x_bytes) for k in range(l[2])]
        else:
            out += [("s", i) for i in range(l[0], l[0] + l[1])]
    return out


def test_tensor_run_merges_contiguous_tiles_up_to_max_defer():
    tiles = _tiles()
    run = _rec(max_defer=16)
    for x, t in tiles[:40]:
        run.step_tensors(x, t)
    assert run.pending_tensors == 8 and run.pending == 0
    run.step_tensors(*tiles[41])          # a gap: launches the 8
    assert run.pending_tensors == 1
    run.flush()
    a = tiles[0][0].data_ptr()
    nb = tiles[0][0].numel() * 4
    assert run.launches == [("t", a, 16), ("t", a + 16 * nb, 16),
                            ("t", a + 32 * nb, 8), ("t", a + 41 * nb, 1)]
    assert run.launch_count == 4
    # a flush does not arm the tensor run: it has no ramp
    for x, t in tiles[:20]:
        run.step_tensors(x, t)
    run.flush()
    assert _sizes_t(run, 4) == [16, 4]


def _sizes_t(run, since):
    return [l[2] for l in run.launches[since:]]


def test_tensor_run_does_not_cross_storages_shapes_or_dtypes():
    import torch
    (x0, t0), (x1, t1) = _tiles()[:2]
    other_x, other_t = _tiles()[1]        # same shapes, storages of its own
    run = _rec()
    run.step_tensors(x0, t0)
    run.step_tensors(other_x, other_t)
    run.step_tensors(x0, t0)
    run.step_tensors(x1, other_t)         # x continues, t does not
    run.step_tensors(x0, t0)
    run.step_tensors(x1.view(2, 6), t1)   # the next bytes, another shape
    run.step_tensors(x0, t0)
    run.step_tensors(x1.view(torch.int32), t1)
    run.flush()
    assert _sizes_t(run, 0) == [1] * 8
    run.step_tensors(x0, t0)
    run.step_tensors(x1, t1)
    run.flush()
    assert _sizes_t(run, 8) == [2]


def test_tensor_and_index_steps_execute_in_submission_order():
    import random
    tiles = _tiles()
    x_bytes = tiles[0][0].numel() * 4
    rng = random.Random(5)
    for trial in range(60):
        md = rng.choice([1, 2, 7, 16])
        run = _rec(steps_bound=64, max_defer=md,
                   ramp_first=rng.choice([0, 2]))
        step = run.step_shard
        want, nxt, nxt_tile = [], 0, 0
        for _ in range(200):
            r = rng.random()
            if r < 0.45:
                i = nxt if r > 0.08 and nxt < 64 else rng.randrange(64)
                step(i)
                want.append(("s", i))
                nxt = i + 1
            elif r < 0.9:
                j = (nxt_tile if r > 0.53 and nxt_tile < len(tiles)
                     else rng.randrange(len(tiles)))
                run.step_tensors(*tiles[j])
                want.append(("t", tiles[j][0].data_ptr()))
                nxt_tile = j + 1
            elif r < 0.95:
                run.flush()
                assert run.pending == 0 and run.pending_tensors == 0
            else:
                # the same bound: the launches' indices keep their meaning
                run.bind_steps(64)
                nxt = 0
            # both pending: the tensor run is the older one, so a tensor
            # step never leaves index steps pending behind it
            if want and want[-1][0] == "t":
                assert run.pending == 0
        run.flush()
        assert _expand(run.launches, x_bytes) == want, (trial, md)
        assert all(l[-1] <= md for l in run.launches)
        assert run.launch_count == len(run.launches)


# -- through bench.drive_shard_bound, as the benchmark drives it ----------
class _Data:
    def __init__(self):
        self.bound_epoch = -1
        self.bound_block = -1

    def shard_for(self, e):
        return ("epoch", e, 1), None

    def shards_for_block(self, e0, epochs):
        return ("block", e0, epochs), None


def _drive(spe, eb, segments, max_defer, ramp_first, growth, flush_between):
    """Drive the recorder over (start, n) segments; returns the executed
    (epoch, in-epoch step) stream. Asserts the launch bounds on the way."""
    import torch  # noqa: F401  (bench imports torch at module load)
    sys.path.insert(0, ROOT)
    import bench

    run = _C.ToyShardRun.recorder(0, max_defer, ramp_first, growth)
    step = run.step_shard
    binds = []  # (bound buffer, number of launches recorded before it)

    def bind(xs, ts, batch):
        run.bind_steps(xs[2] * spe)
        binds.append((xs, len(run.launches)))

    data = _Data()
    for start, n in segments:
        bench.drive_shard_bound(data, spe, 32, eb, bind, step, start, n)
        if flush_between:
            run.flush()
    run.flush()
    assert run.pending == 0
    launches = run.launches
    assert run.launch_count == len(launches)
    executed = []
    for k, (first, n) in enumerate(launches):
        # the buffer bound when launch k was made: bind() launches what is
        # pending BEFORE it re-binds, so a launch recorded at position
        # `before` of a bind still belongs to the previous buffer
        buf = None
        for b, before in binds:
            if before <= k:
                buf = b
        assert buf is not None, "launched before any bind"
        _, e0, epochs = buf
        assert 1 <= n <= max_defer, "launch longer than max_defer"
        assert 0 <= first and first + n <= epochs * spe, \
            "launch leaves the bound shard"
        for idx in range(first, first + n):
            e_loc, i = divmod(idx, spe)
            executed.append((e0 + e_loc, i))
    return executed


def _expected(spe, segments):
    out = []
    for start, n in segments:
        out += [divmod(s, spe) for s in range(start, start + n)]
    return out


@pytest.mark.parametrize("spe,eb", [(64, 16), (8, 128), (64, 1), (7, 3)])
@pytest.mark.parametrize("flush_between", [False, True])
def test_drive_shard_bound_shapes(spe, eb, flush_between):
    segments = [(0, 200), (200, 2000), (2200, 37)]
    got = _drive(spe, eb, segments, 1024, 32, 2.0, flush_between)
    assert got == _expected(spe, segments)


def test_drive_shard_bound_property_fuzz():
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=80, deadline=None)
    @given(st.integers(1, 96), st.integers(1, 160), st.integers(1, 2048),
           st.integers(0, 80), st.sampled_from([1.25, 1.5, 2.0, 3.0]),
           st.lists(st.integers(1, 700), min_size=1, max_size=4),
           st.booleans())
    def run(spe, eb, md, ramp_first, growth, seg_lens, flush_between):
        segments, start = [], 0
        for n in seg_lens:
            segments.append((start, n))
            start += n
        got = _drive(spe, eb, segments, md, ramp_first, growth,
                     flush_between)
        assert got == _expected(spe, segments)

    run()
