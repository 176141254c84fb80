"""CPU tier of the fused LayerNorm: the plain-torch path behind
`ops.layer_norm` / `ops.add_layer_norm`, `HipLayerNorm`'s interchange with
`nn.LayerNorm`, and the ViT switch."""

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipLayerNorm, vit_tiny


def test_cpu_path_is_layer_norm_and_a_plain_add():
    torch.manual_seed(0)
    x, r = torch.randn(2, 3, 7, 48, dtype=torch.float64).unbind(0)
    w, b = torch.randn(2, 48, dtype=torch.float64).unbind(0)
    assert torch.equal(ops.layer_norm(x, w, b, 1e-6),
                       F.layer_norm(x, (48,), w, b, 1e-6))
    s, y = ops.add_layer_norm(x, r, w, b)
    assert torch.equal(s, x + r)
    assert torch.equal(y, F.layer_norm(x + r, (48,), w, b, 1e-5))


def test_state_dicts_interchange_and_init_matches():
    ln, hip = nn.LayerNorm(32, eps=1e-6), HipLayerNorm(32, eps=1e-6)
    sd_l, sd_h = ln.state_dict(), hip.state_dict()
    assert list(sd_l) == list(sd_h)
    assert all(torch.equal(sd_l[k], sd_h[k]) for k in sd_l)  # same init
    with torch.no_grad():
        for p in ln.parameters():
            p.normal_()
    hip.load_state_dict(ln.state_dict())
    x = torch.randn(2, 5, 32)
    assert torch.equal(hip(x), ln(x))
    s, y = hip(x, residual=x)
    assert torch.equal(s, x + x) and torch.equal(y, ln(x + x))
    back = nn.LayerNorm(32, eps=1e-6)
    back.load_state_dict(hip.state_dict())
    assert all(torch.equal(a, b) for a, b in
               zip(back.state_dict().values(), ln.state_dict().values()))


@pytest.mark.parametrize("attention", ["torch", "hip"])
def test_vit_tiny_hip_norm_has_the_same_census_and_trains_on_cpu(attention):
    torch.manual_seed(1)
    ref = vit_tiny()
    m = vit_tiny(attention=attention, norm="hip")
    assert [(k, v.shape) for k, v in m.state_dict().items()] == \
        [(k, v.shape) for k, v in ref.state_dict().items()]
    m.load_state_dict(ref.state_dict())
    x = torch.rand(2, 3, 64, 64)
    assert torch.allclose(m(x), ref(x), atol=1e-5)
    before = [p.detach().clone() for p in m.parameters()]
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    ops.cross_entropy(m(x), torch.tensor([1, 2])).backward()
    opt.step()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in m.parameters())
    assert any(not torch.equal(a, b)
               for a, b in zip(before, m.parameters()))


def test_unknown_norm_is_refused():
    with pytest.raises(ValueError):
        vit_tiny(norm="bogus")
