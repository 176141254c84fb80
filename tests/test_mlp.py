"""CPU tier of the tiled-GEMM MLP: the plain-torch path behind `ops.mlp` /
`ops.linear_gelu`, `HipMlp`'s interchange with the nn.Sequential it replaces,
and the ViT switch."""

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipMlp, vit_tiny


def test_cpu_path_is_the_torch_formula():
    torch.manual_seed(0)
    x = torch.randn(3, 7, 48, dtype=torch.float64)
    w1, w2 = torch.randn(80, 48).double(), torch.randn(48, 80).double()
    b1, b2 = torch.randn(80).double(), torch.randn(48).double()
    h = F.gelu(F.linear(x, w1, b1))
    assert torch.equal(ops.linear_gelu(x, w1, b1), h)
    assert torch.equal(ops.mlp(x, w1, b1, w2, b2), F.linear(h, w2, b2))


def test_state_dicts_interchange_and_init_matches():
    def plain():
        return nn.Sequential(nn.Linear(32, 64), nn.GELU(), nn.Linear(64, 32))
    torch.manual_seed(3)
    seq = plain()
    torch.manual_seed(3)
    hip = HipMlp(32, 64)
    sd_s, sd_h = seq.state_dict(), hip.state_dict()
    assert list(sd_s) == list(sd_h)
    assert all(torch.equal(sd_s[k], sd_h[k]) for k in sd_s)  # same init
    with torch.no_grad():
        for p in seq.parameters():
            p.normal_()
    hip.load_state_dict(seq.state_dict())
    x = torch.randn(2, 5, 32)
    assert torch.equal(hip(x), seq(x))
    back = plain()
    back.load_state_dict(hip.state_dict())
    assert torch.equal(back(x), seq(x))


@pytest.mark.parametrize("attention", ["torch", "hip"])
@pytest.mark.parametrize("norm", ["torch", "hip"])
def test_vit_tiny_hip_mlp_has_the_same_census_and_trains_on_cpu(attention,
                                                                norm):
    torch.manual_seed(1)
    ref = vit_tiny()
    m = vit_tiny(attention=attention, norm=norm, mlp="hip")
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


def test_unknown_mlp_is_refused():
    with pytest.raises(ValueError):
        vit_tiny(mlp="bogus")
