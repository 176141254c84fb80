"""BatchNorm2d over the fused column kernels.

`HipBatchNorm2d(num_features, eps, momentum, act)` is `nn.BatchNorm2d`
(affine, tracking running statistics) with the same parameter and buffer
names, shapes and initialisation, so state dicts interchange in both
directions. With `act="relu"` the ReLU that follows the normalisation rides in
the same kernels, and given a `residual` the add in front of that ReLU does
too (`ops.batch_norm_act`): a bottleneck's `relu(bn3(conv3(out)) + identity)`
costs no pass of its own, forward or backward. `momentum=None`,
`affine=False` and `track_running_stats=False` are not offered.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops


class HipBatchNorm2d(nn.Module):
    def __init__(self, num_features: int, eps: float = 1e-5,
                 momentum: float = 0.1, act: str = "none"):
        super().__init__()
        if act not in ("relu", "none"):
            raise ValueError(f"HipBatchNorm2d: act must be 'relu' or 'none', "
                             f"got {act!r}")
        self.num_features, self.eps = num_features, eps
        self.momentum, self.act = momentum, act
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked",
                             torch.tensor(0, dtype=torch.long))

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: [N, C, H, W] -> act(bn(x) + residual), channels-last."""
        return ops.batch_norm_act(
            x, self.weight, self.bias, self.running_mean, self.running_var,
            residual=residual, act=self.act, training=self.training,
            momentum=self.momentum, eps=self.eps,
            num_batches_tracked=self.num_batches_tracked)

    def extra_repr(self) -> str:
        return (f"{self.num_features}, eps={self.eps}, "
                f"momentum={self.momentum}, act={self.act!r}")
