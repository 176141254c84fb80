"""CPU tier of the fused BatchNorm: the plain-torch path behind
`ops.batch_norm_act`, `HipBatchNorm2d`'s interchange with `nn.BatchNorm2d`,
and the ResNet switch."""

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipBatchNorm2d, ResNet, resnet50


@pytest.mark.parametrize("act,add", [("none", False), ("relu", False),
                                     ("relu", True)])
@pytest.mark.parametrize("training", [True, False])
def test_cpu_path_is_batch_norm_add_relu(act, add, training):
    torch.manual_seed(0)
    x, r = torch.randn(2, 5, 8, 3, 4, dtype=torch.float64).unbind(0)
    w, b, rm = torch.randn(3, 8, dtype=torch.float64).unbind(0)
    rv = torch.rand(8, dtype=torch.float64) + 0.5
    stats = [rm.clone(), rv.clone(), torch.tensor(3)]
    want_stats = [rm.clone(), rv.clone()]
    got = ops.batch_norm_act(x, w, b, stats[0], stats[1],
                             residual=r if add else None, act=act,
                             training=training, momentum=0.2, eps=1e-3,
                             num_batches_tracked=stats[2])
    want = F.batch_norm(x, *want_stats, w, b, training, 0.2, 1e-3)
    want = want + r if add else want
    assert torch.equal(got, F.relu(want) if act == "relu" else want)
    assert all(torch.equal(a, b) for a, b in zip(stats, want_stats))
    assert int(stats[2]) == (4 if training else 3)
    assert training == (not torch.equal(stats[0], rm))


def test_bad_arguments_are_refused():
    x, v = torch.zeros(2, 8, 3, 3), torch.ones(8)
    with pytest.raises(ValueError):
        ops.batch_norm_act(x, v, v, v, v, act="gelu")
    with pytest.raises(ValueError):
        ops.batch_norm_act(x, v, v, v, v, residual=x, act="none")
    with pytest.raises(ValueError):
        ops.batch_norm_act(x[0], v, v, v, v)


def test_state_dicts_interchange_and_init_matches():
    bn, hip = nn.BatchNorm2d(8, eps=1e-3), HipBatchNorm2d(8, eps=1e-3)
    sd_b, sd_h = bn.state_dict(), hip.state_dict()
    assert list(sd_b) == list(sd_h)
    assert all(torch.equal(sd_b[k], sd_h[k]) and sd_b[k].dtype == sd_h[k].dtype
               for k in sd_b)  # same init
    with torch.no_grad():
        for p in bn.parameters():
            p.normal_()
    x = torch.randn(4, 8, 3, 3)
    bn(x)  # moves the running statistics and the counter
    hip.load_state_dict(bn.state_dict())
    assert torch.equal(hip(x), bn(x))
    back = nn.BatchNorm2d(8, eps=1e-3)
    back.load_state_dict(hip.state_dict())
    assert int(back.num_batches_tracked) == 2
    assert all(torch.equal(a, b) for a, b in
               zip(back.state_dict().values(), bn.state_dict().values()))
    assert torch.equal(back.eval()(x), hip.eval()(x))


def test_resnet_hip_norm_has_the_same_census_and_output_on_cpu():
    ref = resnet50()
    assert [(k, v.shape) for k, v in resnet50(norm="hip").state_dict().items()] \
        == [(k, v.shape) for k, v in ref.state_dict().items()]
    torch.manual_seed(1)
    small, ours = ResNet([1, 1, 1, 1], 10), ResNet([1, 1, 1, 1], 10, "hip")
    ours.load_state_dict(small.state_dict())
    x = torch.rand(2, 3, 64, 64)
    assert torch.allclose(ours(x), small(x), atol=1e-5)
    assert all(torch.allclose(a, b, atol=1e-6) for a, b in
               zip(ours.state_dict().values(), small.state_dict().values()))


def test_unknown_norm_is_refused():
    with pytest.raises(ValueError):
        resnet50(norm="bogus")
