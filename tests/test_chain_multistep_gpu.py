"""GPU tests: the lane-parallel fmaf-chain multi-step kernel
(`k_toy_multistep_chain`, the fp32 default at batch 32/64, K 20) produces
the same BITS as the MFMA spec kernel it replaces on the hot path — params
and last-step loss compared as raw int32 words, never with a tolerance."""

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


def _inputs(kind, B, S, seed=11):
    g = torch.Generator().manual_seed(seed + 97 * B + S)
    n = S * B
    if kind == "normal100":  # cancellation + large magnitudes
        X = torch.randn(n, K, generator=g) * 100.0
        T = torch.randn(n, 1, generator=g) * 100.0
    else:  # as bench.py draws them
        X = torch.rand(n, K, generator=g)
        T = torch.rand(n, 1, generator=g)
    if kind == "special":  # exact zeros, -0.0 and f32 subnormals salted in
        for buf in (X, T):
            flat = buf.view(-1)
            idx = torch.randperm(flat.numel(), generator=g)
            m = max(flat.numel() // 8, 3)
            flat[idx[0 * m:1 * m]] = 0.0
            flat[idx[1 * m:2 * m]] = -0.0
            flat[idx[2 * m:3 * m]] = 1e-40
            flat[idx[3 * m:3 * m + m // 2]] = -1e-40
    return X.to(DEV), T.to(DEV)


def _run(impl, X, T, B, use_mse=True, depth=0):
    """One toy_multistep launch from the shared initial params; returns the
    final param words and the last-step loss word."""
    ext = _ext()
    ext.set_toy_multistep_impl(impl)
    ext.set_toy_multistep_chain_depth(depth)
    assert ext.get_toy_multistep_impl() == impl
    p = _params()
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(X, T, p, loss, use_mse, W_OFF, B_OFF, LR, B)
    torch.cuda.synchronize()
    return p.view(torch.int32).cpu(), loss.view(torch.int32).cpu()


def _assert_same_bits(a, b, what):
    pa, la = a
    pb, lb = b
    assert torch.equal(pa, pb), (
        f"{what}: params differ at {(pa != pb).nonzero().flatten().tolist()}: "
        f"{pa.tolist()} vs {pb.tolist()}")
    assert torch.equal(la, lb), f"{what}: loss {la.tolist()} vs {lb.tolist()}"


@pytest.mark.parametrize("S", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("kind,use_mse", [
    ("rand", True), ("normal100", True), ("special", True), ("rand", False)])
def test_chain_matches_mfma_bitwise(kind, use_mse, B, S):
    X, T = _inputs(kind, B, S)
    ref = _run("mfma", X, T, B, use_mse)
    got = _run("chain", X, T, B, use_mse)
    _assert_same_bits(got, ref, f"{kind} mse={use_mse} B={B} S={S}")
    p0 = _params().view(torch.int32).cpu()
    if use_mse:  # the kernel really trained
        assert not torch.equal(got[0], p0)
    else:        # degenerate one-logit CE: dy == 0, params untouched
        assert torch.equal(got[0], p0)
        assert got[1].item() == 0  # +0.0f


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_every_ring_depth_same_bits(depth):
    # S below, equal to and above each depth, odd and even tails
    for S in (1, 2, 3, 4, 7):
        X, T = _inputs("rand", 32, S)
        ref = _run("mfma", X, T, 32)
        got = _run("chain", X, T, 32, depth=depth)
        _assert_same_bits(got, ref, f"depth={depth} S={S}")


@pytest.mark.parametrize("B", [32, 64])
def test_misaligned_tile_base(B):
    # rows are 80 B: a base 4 bytes off 16-byte alignment must take the
    # dword-load variant and still give the aligned copy's bits
    S = 7
    X, T = _inputs("rand", B, S)
    pad = torch.empty(X.numel() + 4, device=DEV)
    Xm = pad[1:1 + X.numel()].view(S * B, K)
    Xm.copy_(X)
    assert X.data_ptr() % 16 == 0 and Xm.data_ptr() % 16 == 4
    assert Xm.is_contiguous()
    aligned = _run("chain", X, T, B)
    _assert_same_bits(_run("chain", Xm, T, B), aligned, "misaligned chain")
    _assert_same_bits(_run("mfma", Xm, T, B), aligned, "misaligned mfma")


def _shard_bound(impl):
    from mi355x_ddp.engine import PersistentToyStep
    from mi355x_ddp.models import toy_model
    _ext().set_toy_multistep_impl(impl)
    runs, per = 3, 64
    g = torch.Generator().manual_seed(5)
    X = torch.rand(runs * per * 32, K, generator=g).to(DEV)
    T = torch.rand(runs * per * 32, 1, generator=g).to(DEV)
    torch.manual_seed(7)
    model = toy_model(K, 1).to(DEV)
    eng = PersistentToyStep(model, comm=None, lr=LR, use_mse=True,
                            track_loss=True, max_defer=per)
    eng.bind_shard(X, T, 32)
    for i in range(runs * per):
        eng.step_shard(i)
    eng.flush()
    torch.cuda.synchronize()
    assert eng.launch_count == runs
    return (torch.cat([model.weight.detach().flatten(),
                       model.bias.detach().flatten()]).view(torch.int32).cpu(),
            eng.loss_out.reshape(1).view(torch.int32).cpu())


def test_shard_bound_run_default_is_chain_and_matches_mfma():
    import os
    ext = _ext()
    if not os.environ.get("MI355X_TOY_MULTISTEP"):
        assert ext.get_toy_multistep_impl() == "chain"  # the default
    _assert_same_bits(_shard_bound("chain"), _shard_bound("mfma"),
                      "shard-bound 3x64")

