"""LayerNorm over the fused row kernels.

`HipLayerNorm(hidden, eps)` is `nn.LayerNorm(hidden, eps)` (affine, one
normalised dimension) with the same parameter names, shapes and
initialisation, so state dicts interchange in both directions. Given a
`residual` it returns `(s, y)` with `s = x + residual` and `y = LN(s)` from
one pass over the rows (`ops.add_layer_norm`): the residual add that precedes
a pre-norm block's second LayerNorm costs no pass of its own.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops


class HipLayerNorm(nn.Module):
    def __init__(self, hidden: int, eps: float = 1e-5):
        super().__init__()
        self.hidden, self.eps = hidden, eps
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))

    def forward(self, x: torch.Tensor,
                residual: Optional[torch.Tensor] = None):
        """x: [..., hidden] -> y, or with a residual (x + residual, y)."""
        if residual is None:
            return ops.layer_norm(x, self.weight, self.bias, self.eps)
        return ops.add_layer_norm(x, residual, self.weight, self.bias,
                                  self.eps)
