"""GPU tests for the class-index cross-entropy kernels (csrc/loss_kernels.hip)
and ops.cross_entropy_index.

Reference: F.cross_entropy in fp64 from the STORED logits and its autograd
gradient. Yardstick: F.cross_entropy in the storage dtype on the device. With
e = max|got - ref| / max|ref| per result, e_ours <= 4 * max(e_torch, eps);
eps = 2^-24 for the f32 loss (either storage) and f32 dlogits, 2^-9 for bf16
dlogits: the bound of tests/test_layer_norm_gpu.py."""

import math

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # sentinel elements on either side; keeps 16-byte alignment
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                                 ids=["f32", "bf16"])
IGNORE = -100
ROW_MAX_C, MIN_SEG, GRID_CAP = 2048, 2048, 512  # loss_kernels.hip's constants
SEG3 = (2, 3 * MIN_SEG + 7)    # three segments, the last one shorter
MANY = (4 * GRID_CAP + 7, 10)  # a wave of the row kernels visits two rows
SHAPES = [(1, 1), (3, 2), (5, 63), (4, 1000), (9, ROW_MAX_C),
          (3, ROW_MAX_C + 1), (2, 4099), SEG3, MANY]
CASES = [(s, "normal", 0.1, "mean") for s in SHAPES] + [
    ((5, 63), "normal", 0.0, "sum"), ((4, 1000), "offset", 0.1, "sum"),
    ((4, 1000), "dominant", 0.0, "none"),
    ((9, ROW_MAX_C), "offset", 0.1, "none"),
    ((3, ROW_MAX_C + 1), "offset", 0.0, "none"),
    ((3, ROW_MAX_C + 1), "dominant", 0.1, "mean"),
    ((2, 4099), "dominant", 0.1, "sum"), (SEG3, "offset", 0.1, "none"),
    (SEG3, "dominant", 0.0, "sum"), (MANY, "normal", 0.0, "none")]


def _err(got, ref):
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


def _guarded(shape, dtype, src=None):
    """A view of `shape` inside a larger NaN-filled allocation."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _pads_intact(*bufs):
    return all(bool(b[:PAD].isnan().all() and b[-PAD:].isnan().all())
               for b in bufs)


def _held(names, ours, torchs, refs, epss):
    bad = []
    for name, o, t, ref, eps in zip(names, ours, torchs, refs, epss):
        e_o, e_t = _err(o, ref), _err(t, ref)
        bound = 4 * max(e_t, eps)
        print(f"{name}: e_ours {e_o:.3e} e_torch {e_t:.3e} "
              f"ratio {e_o / bound:.3f}")
        if not e_o <= bound:  # catches NaN too
            bad.append((name, e_o, bound))
    return bad


def _inputs(B, C, kind, dtype):
    """(logits buffer, logits view, labels with every third row ignored,
    per-row gradient)."""
    g = torch.Generator().manual_seed(10000 * B + C)
    x = 2 * torch.randn(B, C, generator=g)
    if kind == "offset":
        x += 1000 if dtype == torch.float32 else 64
    elif kind == "dominant":
        x *= torch.logspace(-1, 1.3, B).unsqueeze(1)
    labels = torch.randint(0, C, (B,), generator=g)
    labels[1::3] = IGNORE
    buf, view = _guarded((B, C), dtype, x)
    return buf, view, labels.to(DEV), (1 + torch.rand(B, generator=g)).to(DEV)


def _torch(x, labels, smoothing, reduction, grad):
    """(loss, dlogits) of F.cross_entropy in x's dtype; grad is the seed, or
    one value per row for "none"."""
    x = x.detach().clone().requires_grad_(True)
    loss = F.cross_entropy(x, labels, ignore_index=IGNORE,
                           reduction=reduction, label_smoothing=smoothing)
    (loss * grad.to(loss.dtype)).sum().backward()
    return loss.detach(), x.grad


def _kernels(x, labels, smoothing, reduction, grad):
    """(loss, dlogits, buffers) of cei_fwd / cei_bwd on guarded buffers."""
    B, C = x.shape
    bufs, (stats, ws, dx) = zip(
        _guarded((B, 2), torch.float32),
        _guarded((B, ops.ext().cei_plan(B, C)[0], 4), torch.float32),
        _guarded((B, C), x.dtype))
    loss, _, inv = ops.ext().cei_fwd(x, labels, smoothing, IGNORE, reduction,
                                     row_stats=stats, workspace=ws)
    ops.ext().cei_bwd(grad, x, labels, stats, inv, smoothing, IGNORE,
                      reduction, dlogits=dx)
    torch.cuda.synchronize()
    return loss, dx, bufs


def _check(x, labels, smoothing, reduction, grad):
    loss, dx, bufs = _kernels(x, labels, smoothing, reduction, grad)
    ref = _torch(x.double(), labels, smoothing, reduction, grad.double())
    yard = _torch(x, labels, smoothing, reduction, grad)
    bad = _held(("loss", "dlogits"), (loss, dx), yard, ref,
                (EPS[torch.float32], EPS[x.dtype]))
    return loss, dx, bufs, bad


@DTYPES
@pytest.mark.parametrize("shape,kind,smoothing,reduction", CASES)
def test_kernels_against_fp64(shape, kind, smoothing, reduction, dtype):
    S, L = ops.ext().cei_plan(*SEG3)
    assert S >= 3 and SEG3[1] % L and ops.ext().cei_grid_cap() == GRID_CAP
    xbuf, x, labels, grad = _inputs(*shape, kind, dtype)
    if reduction != "none":
        grad = torch.tensor(2.5, device=DEV)
    _, _, bufs, bad = _check(x, labels, smoothing, reduction, grad)
    assert _pads_intact(xbuf, *bufs) and not bad


@DTYPES
@pytest.mark.parametrize("C", [256, 4096], ids=["rows", "segments"])
def test_exact_on_zero_logits(C, dtype):
    """dlogits is torch's fp64 gradient rounded once, and in f32 the exact
    value (2.5 / 4) (1/C - [c == t]). torch's own fp64 gradient is
    exp(log_softmax), an ulp of fp64 away from 1/C, so it is compared after
    the one rounding and the exact value is written out."""
    x = torch.zeros(6, C, dtype=dtype, device=DEV, requires_grad=True)
    labels = torch.tensor([3, IGNORE, C - 1, 0, IGNORE, 7], device=DEV)
    (2.5 * ops.cross_entropy_index(x, labels)).backward()
    _, want = _torch(x.double(), labels, 0.0, "mean", torch.tensor(2.5))
    assert torch.equal(x.grad, want.to(dtype))
    if dtype == torch.float32:
        keep = (labels != IGNORE).double().unsqueeze(1)
        exact = 0.625 * keep * (1 / C - F.one_hot(labels.clamp(min=0), C))
        assert torch.equal(x.grad.double(), exact)


@DTYPES
def test_target_placement(dtype):
    """One-hot-scaled logits: a target fetched from the wrong column moves the
    row's loss by 8."""
    B, C = 4, SEG3[1]
    L = ops.ext().cei_plan(B, C)[1]
    labels = torch.tensor([0, C - 1, L, 2 * L - 1], device=DEV)
    xbuf, x = _guarded((B, C), dtype, 8 * F.one_hot(labels, C))
    _, _, bufs, bad = _check(x, labels, 0.0, "none", torch.ones(B, device=DEV))
    assert _pads_intact(xbuf, *bufs) and not bad


@pytest.mark.parametrize("C", [1000, ROW_MAX_C + 1])
def test_invalid_labels_give_nan_rows(C):
    xbuf, x, labels, grad = _inputs(5, C, "normal", torch.float32)
    labels[labels == IGNORE] = 5
    labels[0], labels[3] = C, -1
    ok = torch.tensor([1, 2, 4], device=DEV)
    valid = labels.clone()
    valid[0] = valid[3] = IGNORE  # for the reference: rows are independent
    loss, dx, bufs, bad = _check(x, valid, 0.1, "none", grad)
    assert not bad
    loss2, dx2, bufs2 = _kernels(x, labels, 0.1, "none", grad)
    assert _pads_intact(xbuf, *bufs2)
    assert loss2[[0, 3]].isnan().all() and dx2[[0, 3]].isnan().all()
    assert torch.equal(loss2[ok], loss[ok]) and torch.equal(dx2[ok], dx[ok])
    mean, _, inv = ops.ext().cei_fwd(x, labels, 0.1, IGNORE, "mean")
    assert mean.isnan() and float(inv) == pytest.approx(0.2)  # 5 rows count


def test_all_rows_ignored():
    x = torch.randn(3, 50, device=DEV, requires_grad=True)
    labels = torch.full((3,), 7, device=DEV)
    assert ops.cross_entropy_index(x, labels, ignore_index=7).isnan()
    loss = ops.cross_entropy_index(x, labels, ignore_index=7, reduction="sum")
    loss.backward()
    assert float(loss) == 0 and not x.grad.any()


def _loss_and_grad(x, labels, reduction="mean"):
    x = x.detach().requires_grad_(True)
    loss = ops.cross_entropy_index(x, labels, 0.1, reduction=reduction)
    (dx,) = torch.autograd.grad((2.5 * loss).sum(), x)
    return loss.detach(), dx


@pytest.mark.parametrize("shape", [SEG3, MANY])
def test_same_bits_run_to_run(shape):
    _, x, labels, _ = _inputs(*shape, "normal", torch.float32)
    runs = [_loss_and_grad(x, labels.int()) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("shape", [(37, 1000), (5, SEG3[1])])
def test_graph_capture_replays_on_new_values(shape):
    _, x, labels, _ = _inputs(*shape, "normal", torch.float32)
    x = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _loss_and_grad(x, labels)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ops.cross_entropy_index(x, labels, 0.1)
        (dx,) = torch.autograd.grad(2.5 * loss, x)
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            x.copy_(3 * torch.randn(shape, generator=g))
            labels.copy_(torch.randint(0, shape[1], shape[:1], generator=g))
            labels[seed::4] = IGNORE
        graph.replay()
        torch.cuda.synchronize()
        want = _loss_and_grad(x, labels)
        assert torch.equal(loss, want[0]) and torch.equal(dx, want[1])


def _z(*shape, dtype=torch.float32, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


GUARDS = {  # name -> (logits, labels, label_smoothing, reduction)
    "f16": lambda: (_z(2, 8, dtype=torch.float16), _z(2).long(), 0.0, "mean"),
    "float labels": lambda: (_z(2, 8), _z(2), 0.0, "mean"),
    "cpu labels": lambda: (_z(2, 8), _z(2, device="cpu").long(), 0.0, "mean"),
    "cpu logits": lambda: (_z(2, 8, device="cpu"), _z(2).long(), 0.0, "mean"),
    "label shape": lambda: (_z(2, 8), _z(3).long(), 0.0, "mean"),
    "strided": lambda: (_z(2, 16)[:, :8], _z(2).long(), 0.0, "mean"),
    "smoothing": lambda: (_z(2, 8), _z(2).long(), 1.5, "mean"),
    "reduction": lambda: (_z(2, 8), _z(2).long(), 0.0, "max"),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    x, labels, smoothing, reduction = GUARDS[name]()
    nan = float("nan")
    stats, ws = torch.full((2, 2), nan, device=DEV), \
        torch.full((2, 1, 4), nan, device=DEV)
    dx = torch.full((2, 8), nan, dtype=x.dtype, device=DEV)
    with pytest.raises(RuntimeError):
        ops.ext().cei_fwd(x, labels, smoothing, IGNORE, reduction,
                          row_stats=stats, workspace=ws)
    with pytest.raises(RuntimeError):
        ops.ext().cei_bwd(None, x, labels, _z(2, 2), _z(1), smoothing, IGNORE,
                          reduction, dlogits=dx)
    if name != "strided":  # the public entry makes the logits contiguous
        with pytest.raises(ValueError):
            ops.cross_entropy_index(x, labels, smoothing, IGNORE, reduction)
    torch.cuda.synchronize()
    assert all(t.isnan().all() for t in (stats, ws, dx))


def test_no_rows_launch_nothing():
    x = _z(0, 3, 8).requires_grad_(True)
    labels = _z(0, 3).long()
    assert ops.cross_entropy_index(x, labels).isnan()
    loss = ops.cross_entropy_index(x, labels, reduction="none")
    assert loss.shape == (0, 3)
    ops.cross_entropy_index(x, labels, reduction="sum").backward()
    assert x.grad.shape == x.shape
