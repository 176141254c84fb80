"""GPU tests of the native shard-bound stepper (ToyShardRun behind
PersistentToyStep at world 1): however the launch schedule cuts a run —
ramped after a flush, re-bound, restarted, interleaved with step(x, t) —
the params and the loss word carry the same BITS as the same steps launched
one by one. Every shard buffer ends in a NaN tile behind the last step, so
a launch one step too long shows up as NaN params."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.05
N = 40                      # steps per case
MD, RF, GR = 16, 2, 2.0     # max_defer, ramp_first, growth


def _ext():
    from mi355x_ddp import ops
    return ops.ext()


@pytest.fixture(autouse=True)
def _restore_impl():
    before = _ext().get_toy_multistep_impl()
    yield
    _ext().set_toy_multistep_impl(before)


@functools.lru_cache(maxsize=None)
def _shard(B, K, dtype, seed=0, steps=N):
    """`steps` tiles of data and one NaN tile behind them (never changed)."""
    g = torch.Generator().manual_seed(100 + seed + 7 * B + K)
    X = torch.rand((steps + 1) * B, K, generator=g)
    T = torch.rand((steps + 1) * B, 1, generator=g)
    X[steps * B:] = float("nan")
    T[steps * B:] = float("nan")
    return X.to(DEV).to(dtype), T.to(DEV).to(dtype)


def _engine(K=20, dtype=torch.float32, ramp_first=RF, max_defer=MD):
    from mi355x_ddp.engine import PersistentToyStep
    from mi355x_ddp.models import toy_model
    torch.manual_seed(7)
    model = toy_model(K, 1).to(DEV).to(dtype)
    eng = PersistentToyStep(model, comm=None, lr=LR, use_mse=True,
                            track_loss=True, max_defer=max_defer,
                            ramp_first=ramp_first, ramp_growth=GR)
    assert eng._run is not None, "world 1 must take the native stepper"
    assert type(eng.step_shard).__name__ == "builtin_function_or_method"
    return eng


def _bits(eng):
    """(param words, loss word, params as f32) after everything ran."""
    torch.cuda.synchronize()
    p = eng.flat_param
    words = p.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32)
    return (words.cpu().clone(),
            eng.loss_out.reshape(1).view(torch.int32).cpu().clone(),
            p.float().cpu())


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (
        f"{what}: params differ: {a[0].tolist()} vs {b[0].tolist()}")
    assert torch.equal(a[1], b[1]), (
        f"{what}: loss word {a[1].tolist()} vs {b[1].tolist()}")
    assert torch.isfinite(a[2]).all(), f"{what}: a launch read the NaN tile"


def _one_by_one(tiles, B, K=20, dtype=torch.float32):
    """The reference: every (x, t) tile as its own S=1 toy_multistep launch
    on a fresh engine's params."""
    eng = _engine(K, dtype)
    for x, t in tiles:
        _ext().toy_multistep(x, t, eng.flat_param, eng.loss_out, True,
                             eng.w_off, eng.b_off, LR, B)
    return _bits(eng)


def _tiles(X, T, B, idx):
    return [(X[i * B:(i + 1) * B], T[i * B:(i + 1) * B]) for i in idx]


@functools.lru_cache(maxsize=None)
def _ref40(B=32, K=20, dtype=torch.float32):
    X, T = _shard(B, K, dtype)
    return _one_by_one(_tiles(X, T, B, range(N)), B, K, dtype)


def _run40(B=32, K=20, dtype=torch.float32, ramp_first=RF):
    """Warm-up-like prelude is left out on purpose: flush() on a new engine
    arms with nothing pending, then the 40 steps run and are flushed."""
    X, T = _shard(B, K, dtype)
    eng = _engine(K, dtype, ramp_first=ramp_first)
    eng.bind_shard(X, T, B)
    eng.flush()
    before = eng.launch_count
    for i in range(N):
        eng.step_shard(i)
    eng.flush()
    return _bits(eng), eng.launch_count - before


def test_ramped_equals_unramped_equals_single_steps():
    ramped, n_ramped = _run40()
    plain, n_plain = _run40(ramp_first=0)
    assert (n_ramped, n_plain) == (5, 3)  # 2 4 8 16 10 | 16 16 8
    _same(ramped, plain, "ramped vs ramp_first=0")
    _same(ramped, _ref40(), "ramped vs 40 single-step launches")
    p0 = _bits(_engine())[0]
    assert not torch.equal(ramped[0], p0)  # it really trained


def test_unarmed_new_engine_launches_at_max_defer():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    for i in range(N):
        eng.step_shard(i)
    eng.flush()
    assert eng.launch_count == 3
    _same(_bits(eng), _ref40(), "unarmed")


def test_run_crossing_two_binds():
    X, T = _shard(32, 20, torch.float32)
    X2, T2 = _shard(32, 20, torch.float32, seed=1)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    eng.flush()
    for i in range(13):
        eng.step_shard(i)
    eng.bind_shard(X2, T2, 32)   # 13 = 2 + 4 + 7: the 7 launch on X
    for i in range(21):
        eng.step_shard(i)
    eng.bind_shard(X, T, 32)
    for i in range(5, 11):
        eng.step_shard(i)
    eng.flush()
    ref = _one_by_one(_tiles(X, T, 32, range(13))
                      + _tiles(X2, T2, 32, range(21))
                      + _tiles(X, T, 32, range(5, 11)), 32)
    _same(_bits(eng), ref, "two binds")


def test_non_sequential_restart():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    eng.flush()
    order = list(range(10)) + list(range(3, 13))
    for i in order:
        eng.step_shard(i)
    eng.flush()
    _same(_bits(eng), _one_by_one(_tiles(X, T, 32, order), 32), "restart")


def test_flush_in_the_middle_and_with_nothing_pending():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    for i in range(N):
        eng.step_shard(i)
        if i in (0, 6, 7, 29):
            eng.flush()
        if i == 7:
            n = eng.launch_count
            eng.flush()          # nothing pending: no launch
            eng.flush()
            assert eng.launch_count == n
    eng.flush()
    _same(_bits(eng), _ref40(), "flush in the middle")


def test_tensor_steps_between_shard_steps():
    X, T = _shard(32, 20, torch.float32)
    P, PT = _shard(32, 20, torch.float32, seed=2)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    eng.flush()
    seq = []
    for i in range(9):
        eng.step_shard(i)
        seq.append(("s", i))
    for j in (4, 5, 6, 20):          # a deferred tensor run 4..6, then 20
        eng.step(*_tiles(P, PT, 32, [j])[0])
        seq.append(("x", j))
    for i in range(9, 30):           # crosses a ramp threshold while the
        eng.step_shard(i)            # tensor step 20 is still pending
        seq.append(("s", i))
    eng.step(*_tiles(P, PT, 32, [1])[0])
    seq.append(("x", 1))
    eng.step_shard(2)                # restart behind a pending tensor step
    seq.append(("s", 2))
    eng.flush()
    tiles = [_tiles(X, T, 32, [k])[0] if kind == "s"
             else _tiles(P, PT, 32, [k])[0] for kind, k in seq]
    _same(_bits(eng), _one_by_one(tiles, 32), "step(x, t) between")


def test_loss_is_the_last_executed_steps():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    eng.bind_shard(X, T, 32)
    eng.flush()
    for i in range(11):
        eng.step_shard(i)
    eng.flush()
    got = _bits(eng)
    ref = _one_by_one(_tiles(X, T, 32, range(11)), 32)
    _same(got, ref, "11 steps")
    # and it is that step's loss: one more single step changes the word
    again = _one_by_one(_tiles(X, T, 32, range(12)), 32)
    assert not torch.equal(got[1], again[1])
    assert got[1].view(torch.float32).item() > 0


@pytest.mark.parametrize("B,K,dtype", [
    (64, 20, torch.float32),      # the batch-64 chain instantiation
    (32, 20, torch.bfloat16),     # the wide-MFMA bf16 kernel
    (16, 8, torch.float32),       # the generic k_toy_multistep
], ids=["batch64", "bf16", "generic16x8"])
def test_other_kernels_ramped_equals_unramped(B, K, dtype):
    ramped, n_ramped = _run40(B, K, dtype)
    plain, n_plain = _run40(B, K, dtype, ramp_first=0)
    assert (n_ramped, n_plain) == (5, 3)
    _same(ramped, plain, f"B={B} K={K} {dtype}")
    if dtype == torch.float32:
        _same(ramped, _ref40(B, K, dtype), f"B={B} K={K} single steps")


def test_out_of_range_index_raises_and_runs_nothing_for_it():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    eng.bind_shard(X[:N * 32], T[:N * 32], 32)  # the NaN tile is NOT bound
    eng.flush()
    for i in range(30, N):
        eng.step_shard(i)
    with pytest.raises(IndexError):
        eng.step_shard(N)        # sequential, one past the end
    assert eng._run.pending == 0
    with pytest.raises(IndexError):
        eng.step_shard(-1)
    eng.flush()
    _same(_bits(eng), _one_by_one(_tiles(X, T, 32, range(30, N)), 32),
          "out of range")


def test_bind_shard_validates_once():
    X, T = _shard(32, 20, torch.float32)
    eng = _engine()
    with pytest.raises(RuntimeError):
        eng.bind_shard(X, T, 33)                  # rows % batch
    with pytest.raises(RuntimeError):
        eng.bind_shard(X.cpu(), T.cpu(), 32)      # not on the device
    with pytest.raises(RuntimeError):
        eng.bind_shard(X.bfloat16(), T.bfloat16(), 32)  # dtype
    with pytest.raises(RuntimeError):
        eng.bind_shard(X, T[:-32], 32)            # rows differ
    with pytest.raises(RuntimeError):
        eng.bind_shard(X.t(), T, 32)              # not contiguous
    with pytest.raises(IndexError):
        eng.step_shard(0)                         # nothing bound yet


def test_mfma_selector_still_respected():
    chain, _ = _run40()
    _ext().set_toy_multistep_impl("mfma")
    mfma, n = _run40()
    assert n == 5
    _same(mfma, chain, "mfma vs chain through the native stepper")
    _same(mfma, _ref40(), "mfma vs single steps")
