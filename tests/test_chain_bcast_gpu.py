"""GPU tests: the broadcast routing of `k_toy_multistep_chain`.

The kernel hands `w[k]` to the row lanes and `dy[i]` to the column lanes
inside the multiply-add (`v_fmac_f32_dpp ... row_newbcast:n` on registers
prepared by `v_permlane16/32_swap`). Each term has its own lane index and
its own low/high source register, so every one of them is exercised alone
here, against the MFMA kernel, as raw int32 words."""

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


def _run(impl, X, T, B, params, depth=0):
    """One toy_multistep launch on a copy of `params`; returns the final
    param words and the last-step loss word."""
    ext = _ext()
    ext.set_toy_multistep_impl(impl)
    ext.set_toy_multistep_chain_depth(depth)
    p = params.clone()
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(X, T, p, loss, True, W_OFF, B_OFF, LR, B)
    torch.cuda.synchronize()
    return p.view(torch.int32).cpu(), loss.view(torch.int32).cpu()


def _same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def _rand_inputs(B, S):
    """X, T as bench.py draws them (uniform [0, 1))."""
    g = torch.Generator().manual_seed(23 + 131 * B + S)
    X = torch.rand(S * B, K, generator=g).to(DEV)
    T = torch.rand(S * B, 1, generator=g).to(DEV)
    return X, T


@functools.lru_cache(maxsize=None)
def _rand_params():
    g = torch.Generator().manual_seed(3)
    return ((torch.rand(K + 1, generator=g) - 0.5) * 0.4).to(DEV)


# ---- forward: w[k] (k = 20: the bias) must reach every row lane ----------

@pytest.mark.parametrize("k", range(K + 1))
@pytest.mark.parametrize("B", [32, 64])
def test_forward_routing_one_hot_param(B, k):
    # only term k of the forward chain is non-zero in step 1: a wrong
    # row_newbcast index or low/high register reads a zero weight instead
    X, T = _rand_inputs(B, 2)
    p0 = torch.zeros(K + 1, device=DEV)
    p0[k] = 0.37
    ref = _run("mfma", X, T, B, p0)
    got = _run("chain", X, T, B, p0)
    assert torch.equal(got[0], ref[0]), (
        f"B={B} one-hot k={k}: params differ at "
        f"{(got[0] != ref[0]).nonzero().flatten().tolist()}")
    assert torch.equal(got[1], ref[1]), f"B={B} one-hot k={k}: loss differs"
    assert not torch.equal(got[0], p0.view(torch.int32).cpu())


# ---- backward: dy[i] must reach every column lane -------------------------

@functools.lru_cache(maxsize=None)
def _exact_problem(B):
    """Random X, params and the prediction X @ w + b, drawn on a 1/64 grid
    so every product (<= 12 bits) and every partial sum (<= 18 bits) is
    exact in f32: the prediction is the same number in any summation order,
    and T = prediction gives d == 0 exactly in both kernels."""
    g = torch.Generator().manual_seed(41 + B)
    X = torch.randint(1, 64, (B, K), generator=g).float() / 64.0  # no zeros
    p = torch.randint(-12, 13, (K + 1,), generator=g).float() / 64.0
    p[p == 0] = 1.0 / 64.0
    pred = (X.double() @ p[:K].double() + p[K].double()).float().view(B, 1)
    return X.to(DEV), p.to(DEV), pred.to(DEV)


@pytest.mark.parametrize("B", [32, 64])
def test_backward_routing_single_row_residual(B):
    X, p0, pred = _exact_problem(B)
    p0_words = p0.view(torch.int32).cpu()
    # the MFMA kernel's own forward confirms the prediction: zero residual
    # on every row, so loss == +0.0 and the params do not move
    words, loss = _run("mfma", X, pred, B, p0)
    assert loss.item() == 0 and torch.equal(words, p0_words)

    bad = []
    for i in range(B):
        # dy is exactly zero except on row i, so only term i of each
        # backward chain is non-zero
        T = pred.clone()
        T[i, 0] = 1.0
        ref = _run("mfma", X, T, B, p0)
        got = _run("chain", X, T, B, p0)
        if not _same_bits(got, ref):
            bad.append((i, "differs from mfma"))
        elif torch.equal(got[0], p0_words):
            bad.append((i, "nothing trained"))  # a dropped term
    assert not bad, f"B={B}: rows {bad}"


# ---- ring tail: S not a multiple of the depth, several trips of the loop --

TAIL_STEPS = [5, 6, 9, 13, 33]


@functools.lru_cache(maxsize=None)
def _mfma_ref(B, S):
    X, T = _rand_inputs(B, S)
    return _run("mfma", X, T, B, _rand_params())


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("S", TAIL_STEPS)
def test_ring_tail_batch32(S, depth):
    X, T = _rand_inputs(32, S)
    got = _run("chain", X, T, 32, _rand_params(), depth=depth)
    ref = _mfma_ref(32, S)
    assert torch.equal(got[0], ref[0]), f"S={S} depth={depth}: params differ"
    assert torch.equal(got[1], ref[1]), f"S={S} depth={depth}: loss differs"


@pytest.mark.parametrize("S", TAIL_STEPS)
def test_ring_tail_batch64_default_depth(S):
    X, T = _rand_inputs(64, S)
    got = _run("chain", X, T, 64, _rand_params())
    ref = _mfma_ref(64, S)
    assert torch.equal(got[0], ref[0]), f"S={S}: params differ"
    assert torch.equal(got[1], ref[1]), f"S={S}: loss differs"
