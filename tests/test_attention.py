"""CPU tier of the fused self-attention: the plain-torch mirror behind
`ops.self_attention`, `HipSelfAttention`'s interchange with
`nn.MultiheadAttention`, and the ViT switch."""

import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipSelfAttention, vit_tiny


def test_cpu_path_is_multihead_attentions_core():
    torch.manual_seed(0)
    mha = nn.MultiheadAttention(48, 3, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_bias.normal_()
    x = torch.randn(2, 7, 48, dtype=torch.float64)
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    y = F.linear(ops.self_attention(qkv, 3), mha.out_proj.weight,
                 mha.out_proj.bias)
    want = mha(x, x, x, need_weights=False)[0]
    assert torch.allclose(y, want, rtol=0, atol=1e-13)


def test_state_dicts_interchange_and_init_matches():
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(32, 2, batch_first=True)
    torch.manual_seed(3)
    hip = HipSelfAttention(32, 2)
    sd_m, sd_h = mha.state_dict(), hip.state_dict()
    assert list(sd_m) == list(sd_h)
    assert all(torch.equal(sd_m[k], sd_h[k]) for k in sd_m)  # same init
    with torch.no_grad():
        for p in mha.parameters():
            p.normal_()
    hip.load_state_dict(mha.state_dict())
    x = torch.randn(2, 5, 32, dtype=torch.float64)
    hip.double(), mha.double()  # exact casts: the state dicts still match
    assert torch.allclose(hip(x), mha(x, x, x, need_weights=False)[0],
                          rtol=0, atol=1e-10)
    back = nn.MultiheadAttention(32, 2, batch_first=True).double()
    back.load_state_dict(hip.state_dict())
    assert all(torch.equal(a, b) for a, b in
               zip(back.state_dict().values(), mha.state_dict().values()))


def test_vit_tiny_hip_has_the_same_census_and_trains_on_cpu():
    torch.manual_seed(1)
    ref = vit_tiny()
    torch.manual_seed(1)
    m = vit_tiny(attention="hip")
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
