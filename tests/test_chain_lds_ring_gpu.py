"""GPU tests: the LDS ring of `k_toy_multistep_chain`.

Loader waves stage each tile in a ring of LDS slots (two halves of H steps,
one workgroup barrier per half) and one compute wave consumes them. These
tests target what that structure can get wrong: chunk boundaries and tails,
a slot consumed stale or overwritten early, a tile outside the launched
range being touched, state carried across launches, and the constant-ones
row of the bias gradient. Every comparison is raw int32 words of the params
and the last-step loss against the MFMA kernel on the same inputs."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 20
W_OFF, B_OFF = 0, K  # flat param buffer: w[0..K) | b
LR = 0.05


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
def _pool(B, tiles):
    """`tiles` distinct random tiles, drawn as bench.py draws them; tests
    launch on prefixes and slices of it and never write to it."""
    g = torch.Generator().manual_seed(41 + 977 * B + tiles)
    X = torch.rand(tiles * B, K, generator=g).to(DEV)
    T = torch.rand(tiles * B, 1, generator=g).to(DEV)
    return X, T


def _launch(impl, X, T, B, p, use_mse=True, depth=0):
    """One toy_multistep launch that updates `p` in place; returns the
    last-step loss word."""
    ext = _ext()
    ext.set_toy_multistep_impl(impl)
    ext.set_toy_multistep_chain_depth(depth)
    assert ext.get_toy_multistep_impl() == impl
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(X, T, p, loss, use_mse, W_OFF, B_OFF, LR, B)
    torch.cuda.synchronize()
    return loss.view(torch.int32).cpu()


def _run(impl, X, T, B, use_mse=True, depth=0):
    p = _params()
    loss = _launch(impl, X, T, B, p, use_mse, depth)
    return p.view(torch.int32).cpu(), loss


def _assert_same_bits(got, ref, what):
    pa, la = got
    pb, lb = ref
    assert torch.equal(pa, pb), (
        f"{what}: params differ at {(pa != pb).nonzero().flatten().tolist()}: "
        f"{pa.tolist()} vs {pb.tolist()}")
    assert torch.equal(la, lb), f"{what}: loss {la.tolist()} vs {lb.tolist()}"


@pytest.mark.parametrize("S", range(1, 41))
@pytest.mark.parametrize("B", [32, 64])
def test_every_chunk_boundary_at_default_depth(B, S):
    # S below, at and above any ring half the LDS budget allows, with
    # every tail length
    X, T = _pool(B, 40)
    X, T = X[:S * B], T[:S * B]
    _assert_same_bits(_run("chain", X, T, B), _run("mfma", X, T, B),
                      f"B={B} S={S}")


@pytest.mark.parametrize("B,S,depth", [
    (32, 257, 0), (32, 1024, 0), (64, 257, 0), (64, 1024, 0),
    (32, 257, 2), (32, 1024, 2), (32, 257, 4), (32, 1024, 4)])
def test_ring_reuse_many_trips(B, S, depth):
    # every slot is refilled many times while the compute wave runs: a
    # stale or early-overwritten slot changes the bits
    X, T = _pool(B, 1024)
    X, T = X[:S * B], T[:S * B]
    _assert_same_bits(_run("chain", X, T, B, depth=depth),
                      _run("mfma", X, T, B), f"B={B} S={S} depth={depth}")


@pytest.mark.parametrize("S", [1, 5, 9])
@pytest.mark.parametrize("B", [32, 64])
def test_nothing_outside_the_launched_range_is_consumed(B, S):
    # NaN tiles on both sides of an interior slice with a non-zero base
    Xp, Tp = _pool(B, 40)
    X = Xp[:(S + 8) * B].clone()
    T = Tp[:(S + 8) * B].clone()
    for buf in (X, T):
        buf[:4 * B] = float("nan")
        buf[(4 + S) * B:] = float("nan")
    Xi, Ti = X[4 * B:(4 + S) * B], T[4 * B:(4 + S) * B]
    assert Xi.data_ptr() != X.data_ptr() and Xi.is_contiguous()
    got = _run("chain", Xi, Ti, B)
    ref = _run("mfma", Xi.clone(), Ti.clone(), B)
    assert torch.isfinite(got[0].view(torch.float32)).all()
    assert torch.isfinite(got[1].view(torch.float32)).all()
    _assert_same_bits(got, ref, f"interior slice B={B} S={S}")


@pytest.mark.parametrize("B", [32, 64])
def test_launch_boundaries_carry_no_state(B):
    X, T = _pool(B, 40)
    X, T = X[:12 * B], T[:12 * B]
    p = _params()
    _launch("chain", X[:5 * B], T[:5 * B], B, p)
    loss = _launch("chain", X[5 * B:], T[5 * B:], B, p)
    _assert_same_bits((p.view(torch.int32).cpu(), loss),
                      _run("mfma", X, T, B), f"5 + 7 steps B={B}")


@pytest.mark.parametrize("B", [32, 64])
def test_degenerate_ce_leaves_params_untouched(B):
    # one-logit CE: dy == 0, so neither the tiles nor the LDS ones row may
    # reach the weights or the bias
    S = 9
    X, T = _pool(B, 40)
    X, T = X[:S * B], T[:S * B]
    got = _run("chain", X, T, B, use_mse=False)
    assert torch.equal(got[0], _params().view(torch.int32).cpu())
    assert got[1].item() == 0  # +0.0f
    _assert_same_bits(got, _run("mfma", X, T, B, use_mse=False),
                      f"CE B={B}")
