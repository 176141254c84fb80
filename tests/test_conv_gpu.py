"""GPU tests for the implicit-GEMM convolution kernels (csrc/conv_kernels.hip)
and what reaches them: ops.conv2d, HipConv2d, ResNet(conv="hip").

Reference, bounds and shapes: tests/conv_cases.py. x and dy are slices
big[1:1+N] of larger channels-last allocations whose neighbouring images are
NaN, so a gather across an image or tensor boundary shows in the result."""

import pytest
import torch

import conv_cases as cc
from mi355x_ddp import ops
from mi355x_ddp.models import HipConv2d, ResNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _nan_neighbours(t):
    """`t` [N, C, H, W] on the device, channels-last, between two NaN images."""
    big = torch.full((t.shape[0] + 2,) + t.shape[1:], float("nan"),
                     dtype=t.dtype, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    big[1:-1] = t
    return big[1:-1]


def _ours(x, w, dy, stride):
    x = _nan_neighbours(x).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    y = ops.conv2d(x, w, stride)
    assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(_nan_neighbours(dy))
    assert w.grad.is_contiguous() and w.grad.dtype == w.dtype
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad}


def _slices(shape):
    N, H, W, Cin, Cout, k, s = shape
    M = N * cc.out_size(H, k, s) * cc.out_size(W, k, s)
    _, _, GS, L = ops.ext().conv_wgrad_plan(M, Cout, Cin, k * k)
    return M, GS, L


@pytest.mark.parametrize("kind", ["random", "integer"])
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=str)
def test_conv2d_against_fp64(shape, dtype, kind):
    M, GS, L = _slices(shape)
    if shape == cc.MULTI_SLICE:
        assert GS >= 3 and M % L
    x, w, dy = cc.operands(shape, dtype, kind)
    ref, S = cc.reference(x, w, dy, shape[6])
    cc.check(_ours(x, w, dy, shape[6]), shape, dtype, kind, ref, S, GS)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["f32", "bf16"])
def test_weight_gradient_is_reproducible(dtype):
    x, w, dy = cc.operands(cc.MULTI_SLICE, dtype, "random")
    runs = [_ours(x, w, dy, 1)["dw"] for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["f32", "bf16"])
def test_graph_replays_to_the_eager_bits(dtype):
    """ops.conv2d and its autograd backward, captured into one graph.

    Every call of `step` makes leaves of its own and returns nothing that
    holds an autograd graph. A leaf's AccumulateGrad node keeps the stream it
    was made on; one left alive by an earlier call on another stream makes
    the engine synchronise the two streams with a temporary event inside the
    capture; a capture written that way died in hipStreamEndCapture
    (docs/KERNELS.md, "Graphs")."""
    shape = cc.SHAPES[3]
    x, w, dy = (t.to(DEV) for t in cc.operands(shape, dtype, "random"))

    def step():
        xl, wl = (t.detach().requires_grad_(True) for t in (x, w))
        y = ops.conv2d(xl, wl, shape[6])
        return (y.detach(),) + torch.autograd.grad(y, (xl, wl), dy)

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, outs))


GPU_REFUSED = dict(cc.REFUSED, **{
    "f16": ((1, 16, 8, 8), (16, 16, 3, 3), 1, None, torch.float16),
    "misaligned": ((1, 16, 8, 8), (16, 16, 3, 3), 1, None, None)})


@pytest.mark.parametrize("name", GPU_REFUSED)
def test_refused_before_any_launch(name):
    xs, ws, stride, padding, wdtype = GPU_REFUSED[name]
    xdtype = torch.float16 if name == "f16" else torch.float32
    x = torch.zeros(xs, dtype=xdtype, device=DEV)
    if name == "misaligned":
        x = torch.zeros(x.numel() + 1, device=DEV)[1:].view(1, 8, 8, 16) \
            .permute(0, 3, 1, 2)
    w = torch.zeros(ws, dtype=wdtype or xdtype, device=DEV)
    with pytest.raises(ValueError):
        ops.conv2d(x, w, stride, padding)


def test_empty_batch():
    w = torch.zeros(16, 16, 3, 3, device=DEV, requires_grad=True)
    y = ops.conv2d(torch.zeros(0, 16, 5, 5, device=DEV), w, 2)
    assert y.shape == (0, 16, 3, 3)
    y.sum().backward()
    assert torch.equal(w.grad, torch.zeros_like(w))


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("norm", ["torch", "hip"])
def test_small_resnet(norm):
    """Logits and the gradients of the first and the last converted
    convolution of ResNet([1, 1, 1, 1], conv="hip") in f32 against the fp64
    model: e_ours <= 4 * max(e_torch, 2^-24), e = max|got - ref| / max|ref|,
    e_torch from the same model with conv="torch"."""
    torch.manual_seed(11)
    base = ResNet([1, 1, 1, 1], 10, norm=norm).to(DEV)
    ours = ResNet([1, 1, 1, 1], 10, norm=norm, conv="hip").to(DEV)
    ref = ResNet([1, 1, 1, 1], 10).double()  # on the CPU
    ours.load_state_dict(base.state_dict())
    base.load_state_dict(ours.state_dict())
    ref.load_state_dict(base.state_dict())
    names = [n for n, m in ours.named_modules() if isinstance(m, HipConv2d)]
    assert len(names) == 16  # four blocks of three, each with a downsample
    x = torch.rand(2, 3, 64, 64, device=DEV)
    g = torch.randn(2, 10, device=DEV)
    outs = []
    for m, dt in ((ours, None), (base, None), (ref, torch.float64)):
        xin, gin = (x, g) if dt is None else (x.cpu().double(), g.cpu().double())
        logits = m(xin)
        (logits * gin).sum().backward()
        outs.append({"logits": logits.detach(), **{
            n: m.get_submodule(n).weight.grad for n in (names[0], names[-1])}})
    bad = []
    for name, r in outs[2].items():
        e_o, e_t = _err(outs[0][name], r), _err(outs[1][name], r)
        print(f"{norm} {name}: e_ours {e_o:.3e} e_torch {e_t:.3e}")
        if not e_o <= 4 * max(e_t, 2.0 ** -24):
            bad.append(name)
    assert not bad
