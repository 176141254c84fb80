"""GPU tests: the loader side of `k_toy_multistep_chain`.

The workgroup has four waves: wave 0 computes, waves 1 and 3 load, wave 2
is parked and executes the barriers only. The loaders no longer walk the
tile by its flat index: each 32-lane group takes a block of 4 rows x 8 k
(or 8 rows x 4 k for k = 16..19), the same lane-to-element map for the
global load, the row image and the transposed image. These tests target
what that can break: an element of either image dropped, written twice or
put in the wrong place, a wave that executes one barrier more or fewer than
the others, a tile past the launched range addressed, LDS left from the
launch before, a base that is not 16-byte aligned, and the CE path. Every
comparison is raw int32 words of the params and the last-step loss against
the MFMA kernel on the same inputs."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 20
P = K + 1  # one flat param block: w[0..K) | b
LR = 0.05

# (batch, depth passed to the setter, H it selects)
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


def _params(n=1, seed=3):
    """n copies of one non-zero param block, flat."""
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(P, generator=g) - 0.5) * 0.4
    assert (p != 0).all()
    return p.repeat(n).to(DEV)


@functools.lru_cache(maxsize=None)
def _pool(B, tiles=48):
    """`tiles` distinct random tiles; tests copy what they change."""
    g = torch.Generator().manual_seed(131 + 977 * B + tiles)
    X = torch.rand(tiles * B, K, generator=g).to(DEV)
    T = torch.rand(tiles * B, 1, generator=g).to(DEV)
    return X, T


def _select(impl, depth=0):
    ext = _ext()
    ext.set_toy_multistep_impl(impl)
    ext.set_toy_multistep_chain_depth(depth)
    return ext


def _run(impl, X, T, B, use_mse=True, depth=0):
    ext = _select(impl, depth)
    p = _params()
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(X, T, p, loss, use_mse, 0, K, LR, B)
    torch.cuda.synchronize()
    return p.view(torch.int32).cpu(), loss.view(torch.int32).cpu()


def _assert_same_bits(got, ref, what):
    pa, la = got
    pb, lb = ref
    assert torch.equal(pa, pb), (
        f"{what}: params differ at {(pa != pb).nonzero().flatten().tolist()}")
    assert torch.equal(la, lb), f"{what}: loss {la.tolist()} vs {lb.tolist()}"


# ---- element placement, both images ----

def _placement_cases(B):
    """(i, k) of the one non-zero element of each launch: every element at
    batch 32; at batch 64 one row per (i mod 16, k) class, the row's upper
    bits varying with the class."""
    if B == 32:
        return [(i, k) for i in range(B) for k in range(K)]
    return [(c + 16 * ((c + k) % 4), k) for c in range(16) for k in range(K)]


def _one_hot_launches(impl, B, X, T):
    """One S = 1 launch per tile of X, each on a param block and a loss word
    of its own, back to back on one stream; one synchronise at the end."""
    n = X.shape[0]
    ext = _select(impl)
    p = _params(n)
    loss = torch.full((n,), -1.0, device=DEV)
    for j in range(n):
        ext.toy_multistep(X[j], T[j], p, loss[j:j + 1], True, j * P,
                          j * P + K, LR, B)
    torch.cuda.synchronize()
    return p.view(torch.int32).cpu().view(n, P), loss.view(torch.int32).cpu()


@pytest.mark.parametrize("B", [32, 64])
def test_every_element_reaches_its_place_in_both_images(B):
    # X is zero except X[i][k]: the forward reads it from the row image
    # (y_i alone moves off the bias), the backward from the transposed one
    # (dw_k alone is non-zero, through dy_i, which the random targets make
    # different for every row). Put elsewhere, dropped (the slot then keeps
    # the launch before's element) or duplicated, it changes bits.
    cases = _placement_cases(B)
    n = len(cases)
    g = torch.Generator().manual_seed(7 + B)
    X = torch.zeros(n, B, K)
    vals = 0.5 + torch.rand(n, generator=g)
    for j, (i, k) in enumerate(cases):
        X[j, i, k] = vals[j]
    X = X.to(DEV)
    T = torch.rand(n, B, 1, generator=g).to(DEV)
    got_p, got_l = _one_hot_launches("chain", B, X, T)
    ref_p, ref_l = _one_hot_launches("mfma", B, X, T)
    untouched = _params(n).view(torch.int32).cpu().view(n, P)
    for j, (i, k) in enumerate(cases):
        # the reference itself must see the element: w_k moves
        assert ref_p[j, k] != untouched[j, k], (i, k)
        assert torch.equal(got_p[j], ref_p[j]), (
            f"B={B} element ({i}, {k}): params "
            f"{got_p[j].tolist()} vs {ref_p[j].tolist()}")
    assert torch.equal(got_l, ref_l)


@pytest.mark.parametrize("B", [32, 64])
def test_all_elements_distinct(B):
    # every element its own integer code: two elements swapped inside an
    # image, or between lanes of the loaders, show in the params
    code = torch.arange(1, B * K + 1, dtype=torch.float32).view(B, K) / 64.0
    X = code.to(DEV)
    T = _pool(B)[1][:B].clone()
    _assert_same_bits(_run("chain", X, T, B), _run("mfma", X, T, B),
                      f"distinct codes B={B}")


# ---- roles and barrier count ----

@functools.lru_cache(maxsize=None)
def _nan_behind(B, S):
    """Tiles 0 .. S - 1 of the pool followed by four NaN tiles, X and T."""
    Xp, Tp = _pool(B)
    X = Xp[:(S + 4) * B].clone()
    T = Tp[:(S + 4) * B].clone()
    X[S * B:] = float("nan")
    T[S * B:] = float("nan")
    return X, T


def _two_launches(impl, B, S, depth):
    """Launch on tiles 24 .. 24 + S of the pool, then on the NaN-backed
    range 0 .. S, same params, nothing between them on the stream."""
    Xp, Tp = _pool(B)
    X, T = _nan_behind(B, S)
    ext = _select(impl, depth)
    p = _params()
    loss = torch.full((1,), -1.0, device=DEV)
    ext.toy_multistep(Xp[24 * B:(24 + S) * B], Tp[24 * B:(24 + S) * B], p,
                      loss, True, 0, K, LR, B)
    ext.toy_multistep(X[:S * B], T[:S * B], p, loss, True, 0, K, LR, B)
    torch.cuda.synchronize()
    return p.view(torch.int32).cpu(), loss.view(torch.int32).cpu()


def _role_cases():
    for B, depth, H in DEPTHS:
        for S in sorted({1, 2, 2 * H - 1, 2 * H, 2 * H + 1, 4 * H + 1,
                         4 * H + 5}):
            yield pytest.param(B, depth, S, id=f"B{B}-H{H}-S{S}")


@pytest.mark.parametrize("B,depth,S", _role_cases())
def test_every_wave_runs_the_same_barriers_and_stays_in_range(B, depth, S):
    # a wave (parked, loader or compute) with one barrier more or fewer than
    # the rest hangs the launch; a tile >= S staged and consumed turns the
    # params NaN; a slot the second launch failed to rewrite holds the first
    # launch's tile
    assert 24 + S <= 48
    got = _two_launches("chain", B, S, depth)
    assert torch.isfinite(got[0].view(torch.float32)).all()
    assert torch.isfinite(got[1].view(torch.float32)).all()
    _assert_same_bits(got, _two_launches("mfma", B, S, 0),
                      f"B={B} depth={depth} S={S}")


# ---- base off 16-byte alignment ----

@pytest.mark.parametrize("B", [32, 64])
def test_tile_base_one_float_off_alignment(B):
    # the loaders' per-lane offsets are in dwords from the tile base: no
    # load may assume more than 4-byte alignment
    S = 5
    Xp, Tp = _pool(B)
    X, T = Xp[:S * B], Tp[:S * B]
    pad = torch.empty(X.numel() + 4, device=DEV)
    Xm = pad[1:1 + X.numel()].view(S * B, K)
    Xm.copy_(X)
    tpad = torch.empty(T.numel() + 4, device=DEV)
    Tm = tpad[1:1 + T.numel()].view(S * B, 1)
    Tm.copy_(T)
    assert Xm.data_ptr() % 16 == 4 and Tm.data_ptr() % 16 == 4
    ref = _run("mfma", X, T, B)
    _assert_same_bits(_run("chain", Xm, Tm, B), ref, f"misaligned B={B}")


# ---- degenerate CE path ----

@pytest.mark.parametrize("B,depth,H", DEPTHS)
@pytest.mark.parametrize("which", ["S3", "S2H+1"])
def test_ce_path_with_nan_and_inf_targets(B, depth, H, which):
    # use_mse = False: dy is exactly 0 whatever d is; the roles and the
    # barrier count are the MSE path's
    S = 3 if which == "S3" else 2 * H + 1
    Xp, Tp = _pool(B)
    X, T = Xp[:S * B], Tp[:S * B].clone()
    T[0::3] = float("nan")
    T[1::7] = float("inf")
    T[2::11] = float("-inf")
    got = _run("chain", X, T, B, use_mse=False, depth=depth)
    assert torch.equal(got[0], _params().view(torch.int32).cpu())
    assert got[1].item() == 0  # +0.0f
    _assert_same_bits(got, _run("mfma", X, T, B, use_mse=False),
                      f"CE B={B} H={H} S={S}")
