"""CPU tier of ops.cross_entropy_index: F.cross_entropy's numbers and the
argument guard."""

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp import ops


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_cpu_path_is_torch(reduction):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 11, generator=g, requires_grad=True)
    labels = torch.randint(0, 11, (2, 5), generator=g, dtype=torch.int32)
    labels[0, 1::2] = 4
    loss = ops.cross_entropy_index(x, labels, 0.1, 4, reduction)
    want = F.cross_entropy(x.detach().reshape(10, 11), labels.reshape(10).long(),
                           ignore_index=4, reduction=reduction,
                           label_smoothing=0.1)
    assert loss.dtype == torch.float32
    assert torch.equal(loss.detach(), want.reshape(loss.shape))
    (2.5 * loss).sum().backward()
    assert x.grad.shape == x.shape and not x.grad[0, 1::2].any()


@pytest.mark.parametrize("kwargs", [
    dict(logits=torch.zeros(2, 8, dtype=torch.float64)),
    dict(labels=torch.zeros(2)),
    dict(labels=torch.zeros(3, dtype=torch.int64)),
    dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
    dict(reduction="max")],
    ids=["f64", "float labels", "label shape", "smoothing < 0",
         "smoothing > 1", "reduction"])
def test_guard_raises_on_the_cpu_too(kwargs):
    args = dict(logits=torch.zeros(2, 8),
                labels=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.cross_entropy_index(**{**args, **kwargs})
