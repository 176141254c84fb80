"""The transformer MLP over the tiled MFMA GEMMs.

`HipMlp(hidden, mlp)` is `nn.Sequential(nn.Linear(hidden, mlp), nn.GELU(),
nn.Linear(mlp, hidden))` with the same parameter names (`0.weight`, `0.bias`,
`2.weight`, `2.bias`), shapes and initialisation, so state dicts interchange
in both directions; its forward is one `ops.mlp` call (six GEMM launches
forward and backward, no elementwise kernel).
"""

from __future__ import annotations

import torch
from torch import nn

from .. import ops


class HipMlp(nn.Sequential):
    def __init__(self, hidden: int, mlp: int):
        super().__init__(nn.Linear(hidden, mlp), nn.GELU(),
                         nn.Linear(mlp, hidden))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.mlp(x, self[0].weight, self[0].bias,
                       self[2].weight, self[2].bias)
