"""Conv2d over the implicit-GEMM kernels.

`HipConv2d(cin, cout, kernel_size, stride)` is `nn.Conv2d(cin, cout,
kernel_size, stride, padding=kernel_size // 2, bias=False)` with the same
parameter name, shape and initialisation, so state dicts interchange in both
directions. Kernel size 1 or 3, stride 1 or 2, channels multiples of 16
(`ops.conv2d`); a bias, groups, dilation and other paddings are not offered.
"""

from __future__ import annotations

import math

import torch
from torch import nn

from .. import ops


class HipConv2d(nn.Module):
    def __init__(self, in_channels: int, out_channels: int,
                 kernel_size: int, stride: int = 1):
        super().__init__()
        # the op's own rules, on shapes alone: refuse here, not at the first
        # forward
        ops.conv_check_args(
            torch.empty(1, in_channels, 1, 1, device="meta"),
            torch.empty(out_channels, in_channels, kernel_size, kernel_size,
                        device="meta"), stride, None)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = kernel_size, stride
        self.weight = nn.Parameter(torch.empty(
            out_channels, in_channels, kernel_size, kernel_size))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))  # nn.Conv2d's

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [N, Cin, H, W] -> [N, Cout, Ho, Wo], channels-last."""
        return ops.conv2d(x, self.weight, self.stride)

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, "
                f"kernel_size={self.kernel_size}, stride={self.stride}")
