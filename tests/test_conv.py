"""CPU tests for ops.conv2d, HipConv2d and resnet50(conv="hip"): the CPU path,
the refusals, the state dicts, and that torch's own fp32 and bf16 convolution
meets the bounds the kernels are held to (tests/conv_cases.py)."""

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_cases as cc
from mi355x_ddp import ops
from mi355x_ddp.models import HipConv2d, ResNet, resnet50


@pytest.mark.parametrize("shape", cc.SHAPES[:7], ids=str)
def test_cpu_path_is_f_conv2d(shape):
    x, w, dy = cc.operands(shape, torch.float32, "random")
    want = cc.conv_all(x, w, dy, shape[6])
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ops.conv2d(x, w, shape[6])
    y.backward(dy)
    assert torch.equal(y, want["y"]) and torch.equal(x.grad, want["dx"]) \
        and torch.equal(w.grad, want["dw"])


@pytest.mark.parametrize("name", cc.REFUSED)
def test_refused(name):
    xs, ws, stride, padding, wdtype = cc.REFUSED[name]
    with pytest.raises(ValueError):
        ops.conv2d(torch.zeros(xs), torch.zeros(ws, dtype=wdtype), stride,
                   padding)


def test_too_many_pixels_refused():
    x = torch.empty(2 ** 17, 16, 2 ** 7, 2 ** 7, device="meta")
    with pytest.raises(ValueError):
        ops.conv2d(x, torch.empty(16, 16, 1, 1, device="meta"))


def test_state_dicts_interchange():
    torch.manual_seed(0)
    ours, theirs = HipConv2d(32, 16, 3, 2), nn.Conv2d(32, 16, 3, 2, 1,
                                                      bias=False)
    assert ours.weight.shape == theirs.weight.shape
    sd = theirs.state_dict()
    ours.load_state_dict(sd)
    theirs.load_state_dict(ours.state_dict())
    x = torch.randn(2, 32, 9, 9)
    assert torch.equal(ours(x), theirs(x))
    with pytest.raises(ValueError):
        HipConv2d(32, 16, 5)


def test_resnet_switch_keeps_names_and_shapes():
    want = {k: v.shape for k, v in resnet50().state_dict().items()}
    for norm in ("torch", "hip"):
        model = resnet50(norm=norm, conv="hip")
        assert {k: v.shape for k, v in model.state_dict().items()} == want
        convs = [m for m in model.modules() if isinstance(m, HipConv2d)]
        assert len(convs) == 52 and isinstance(model.conv1, nn.Conv2d)
        # the init loop reached them: kaiming_normal_, fan_out
        w = model.layer4[2].conv2.weight
        assert abs(float(w.detach().std()) - (2 / (512 * 9)) ** 0.5) < 1e-3
    with pytest.raises(ValueError):
        ResNet([1, 1, 1, 1], conv="miopen")


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=str)
def test_torch_cpu_convolution_meets_the_bounds(shape, dtype):
    x, w, dy = cc.operands(shape, dtype, "random")
    ref, S = cc.reference(x, w, dy, shape[6])
    cc.check(cc.conv_all(x, w, dy, shape[6]), shape, dtype, "random", ref, S,
             GS=1)
