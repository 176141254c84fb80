"""GPU tests: the step loops of `k_toy_multistep_chain`'s compute wave.

The compute wave runs whole turns of the LDS ring as straight-line code
(depth a compile-time constant, slot offsets as immediates, barriers at
fixed places) and hands the last 1 .. 2H steps of a launch to the general
loop; `use_mse` selects between two loop bodies. These tests target what
that structure can get wrong: the hand-over and the barrier count at every
small S around a turn, a tile past the launched range reaching a chain, an
operand set consumed a step early or late, LDS left over from the previous
launch, and the hoisted `use_mse` choice. Every comparison is raw int32
words of the params and the last-step loss against the MFMA kernel on the
same inputs."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 20
W_OFF, B_OFF = 0, K  # flat param buffer: w[0..K) | b
LR = 0.05

# (batch, depth passed to the setter, H it selects): every depth the setter
# accepts at batch 32; batch 64 holds two slots per ring half whatever is set
DEPTHS = [(32, 2, 2), (32, 3, 3), (32, 4, 4), (64, 0, 2)]


def _ext():
    from mi355x_ddp import ops
    return ops.ext()


@pytest.fixture(autouse=True)
def _restore_impl():
    ext = _ext()
    before = ext.get_toy_multistep_impl()
    yield
    ext.set_toy_multistep_impl(before)
    ext.set_toy_multistep_chain_depth(0)


def _params(seed=3):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(K + 1, generator=g) - 0.5) * 0.4).to(DEV)


@functools.lru_cache(maxsize=None)
def _pool(B, tiles=48):
    """`tiles` distinct random tiles; tests copy what they change."""
    g = torch.Generator().manual_seed(59 + 977 * B + tiles)
    X = torch.rand(tiles * B, K, generator=g).to(DEV)
    T = torch.rand(tiles * B, 1, generator=g).to(DEV)
    return X, T


def _launch(impl, X, T, B, p, use_mse=True, depth=0, lr=LR, sync=True):
    """One toy_multistep launch that updates `p` in place; returns the
    last-step loss word (a device tensor when not synchronising)."""
    ext = _ext()
    ext.set_toy_multistep_impl(impl)
    ext.set_toy_multistep_chain_depth(depth)
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(X, T, p, loss, use_mse, W_OFF, B_OFF, lr, B)
    if not sync:
        return loss
    torch.cuda.synchronize()
    return loss.view(torch.int32).cpu()


def _run(impl, X, T, B, use_mse=True, depth=0, lr=LR):
    p = _params()
    loss = _launch(impl, X, T, B, p, use_mse, depth, lr)
    return p.view(torch.int32).cpu(), loss


def _assert_same_bits(got, ref, what):
    pa, la = got
    pb, lb = ref
    assert torch.equal(pa, pb), (
        f"{what}: params differ at {(pa != pb).nonzero().flatten().tolist()}: "
        f"{pa.tolist()} vs {pb.tolist()}")
    assert torch.equal(la, lb), f"{what}: loss {la.tolist()} vs {lb.tolist()}"


# ---- tail fetch and barrier count ----

@functools.lru_cache(maxsize=None)
def _nan_behind(B, S):
    """Tiles 0 .. S - 1 of the pool followed by four NaN tiles, X and T, and
    the MFMA result of launching on the first S."""
    Xp, Tp = _pool(B)
    X = Xp[:(S + 4) * B].clone()
    T = Tp[:(S + 4) * B].clone()
    X[S * B:] = float("nan")
    T[S * B:] = float("nan")
    ref = _run("mfma", X[:S * B].clone(), T[:S * B].clone(), B)
    return X, T, ref


def _tail_cases():
    for B, depth, H in DEPTHS:
        for S in sorted({1, 2, 3, 2 * H - 1, 2 * H, 2 * H + 1, 4 * H + 1}):
            yield pytest.param(B, depth, S, id=f"B{B}-H{H}-S{S}")


@pytest.mark.parametrize("B,depth,S", _tail_cases())
def test_tail_reads_no_tile_past_the_range_and_barriers_match(B, depth, S):
    # a read of tile >= S that reached a chain would turn the params NaN;
    # a barrier more or fewer than the loaders' would hang the launch
    X, T, ref = _nan_behind(B, S)
    got = _run("chain", X[:S * B], T[:S * B], B, depth=depth)
    assert torch.isfinite(got[0].view(torch.float32)).all()
    assert torch.isfinite(got[1].view(torch.float32)).all()
    _assert_same_bits(got, ref, f"B={B} depth={depth} S={S}")


# ---- a set consumed a step early or late ----

# Even tiles at 2^10, odd tiles at 2^-20. The step size keeps the large
# steps contracting: lr * (2 / B) * lambda_max(X^T X) is about
# lr * 2 K * (2^10 / 2)^2 = lr * 2^23.3, below 2 for lr = 2^-24.
BIG, SMALL, LR_SCALED = 2.0 ** 10, 2.0 ** -20, 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _two_scales(B, S):
    Xp, Tp = _pool(B)
    X = Xp[:S * B].clone().view(S, B, K)
    T = Tp[:S * B].clone().view(S, B, 1)
    for buf in (X, T):
        buf[0::2] *= BIG
        buf[1::2] *= SMALL
    X, T = X.view(S * B, K), T.view(S * B, 1)
    return X, T, _run("mfma", X, T, B, lr=LR_SCALED)


@pytest.mark.parametrize("S", [2, 5, 8, 33])
@pytest.mark.parametrize("B,depth,H", DEPTHS)
def test_each_operand_set_is_consumed_by_its_own_step(B, depth, H, S):
    # an operand set from two steps earlier (the same registers), from the
    # neighbouring step, or not yet arrived differs in scale or in data
    # from the right one, so it changes bits and never rounds the same
    X, T, ref = _two_scales(B, S)
    assert torch.isfinite(ref[0].view(torch.float32)).all()
    got = _run("chain", X, T, B, depth=depth, lr=LR_SCALED)
    _assert_same_bits(got, ref, f"two scales B={B} H={H} S={S}")


# ---- back-to-back launches ----

@pytest.mark.parametrize("B,depth,H", DEPTHS)
def test_back_to_back_launches_see_no_stale_slots(B, depth, H):
    # three launches of 2H + 1 steps on consecutive ranges, nothing between
    # them: each finds the previous launch's tiles in every LDS slot
    S = 2 * H + 1
    Xp, Tp = _pool(B)
    X, T = Xp[:3 * S * B], Tp[:3 * S * B]
    p = _params()
    for i in range(3):
        lo, hi = i * S * B, (i + 1) * S * B
        loss = _launch("chain", X[lo:hi], T[lo:hi], B, p, depth=depth,
                       sync=False)
    torch.cuda.synchronize()
    got = (p.view(torch.int32).cpu(), loss.view(torch.int32).cpu())
    _assert_same_bits(got, _run("mfma", X, T, B), f"3 x {S} steps B={B} H={H}")
    _assert_same_bits(got, _run("chain", X, T, B, depth=depth),
                      f"3 x {S} steps vs one chain launch B={B} H={H}")


# ---- degenerate CE path ----

@pytest.mark.parametrize("B,depth,H", DEPTHS)
def test_ce_path_ignores_nan_and_inf_targets(B, depth, H):
    # use_mse = False: dy is exactly 0 whatever d is, so NaN and Inf
    # residuals inside the launched range must not reach the params
    S = 4 * H + 1
    Xp, Tp = _pool(B)
    X, T = Xp[:S * B], Tp[:S * B].clone()
    T[0::3] = float("nan")
    T[1::7] = float("inf")
    T[2::11] = float("-inf")
    got = _run("chain", X, T, B, use_mse=False, depth=depth)
    assert torch.equal(got[0], _params().view(torch.int32).cpu())
    assert got[1].item() == 0  # +0.0f
    _assert_same_bits(got, _run("mfma", X, T, B, use_mse=False),
                      f"CE B={B} H={H}")
