"""ResNet-50, defined locally (torchvision is not installed in this
environment — SURVEY §7 environment facts).

The profiling entrypoint (reference multigpu_profile.py:14,25 imports
torchvision's resnet50) needs a real convolutional workload whose DDP
gradient payload is ~102 MB across many buckets. By default
conv/BN/pool run through MIOpen via PyTorch-ROCm; the
final FC layer uses the hand-written MFMA linear.

Standard bottleneck architecture (He et al. 2015), v1.5 variant (stride on
the 3x3 conv) to match what torchvision's resnet50 computes.

`norm="hip"` (opt-in; the default "torch" is nn.BatchNorm2d, untouched) puts
`HipBatchNorm2d` in every BatchNorm's place, under the same parameter and
buffer names: the ReLUs after the stem's and a block's first two norms ride in
the norm's kernels, a block's last norm also takes the residual add and the
final ReLU, and the downsample norm runs without activation.

`conv="hip"` (opt-in; the default "torch" is nn.Conv2d, untouched) puts
`HipConv2d` in the place of the 52 1x1 and 3x3 convolutions, under the same
parameter names: one implicit-GEMM MFMA kernel family (`ops.conv2d`) serves
them all, forward and backward, since every one has channels that are
multiples of 64, stride 1 or 2 and padding k//2. The 7x7 stem (3 input
channels) and the two poolings stay with the library. The switch is
independent of `norm`; state dicts interchange between all four combinations.
"""

from __future__ import annotations

import torch
from torch import nn

from .batchnorm import HipBatchNorm2d
from .conv import HipConv2d
from .toy import HipLinear


def _conv(conv: str, cin: int, cout: int, k: int, stride: int) -> nn.Module:
    if conv == "hip":
        return HipConv2d(cin, cout, k, stride)
    if conv == "torch":
        return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2,
                         bias=False)
    raise ValueError(f"conv must be 'torch' or 'hip', got {conv!r}")


def conv3x3(cin: int, cout: int, stride: int = 1,
            conv: str = "torch") -> nn.Module:
    return _conv(conv, cin, cout, 3, stride)


def conv1x1(cin: int, cout: int, stride: int = 1,
            conv: str = "torch") -> nn.Module:
    return _conv(conv, cin, cout, 1, stride)


def _norm(norm: str, channels: int, act: str) -> nn.Module:
    """The BatchNorm of a `norm` model; `act` is fused only under "hip"."""
    if norm == "hip":
        return HipBatchNorm2d(channels, act=act)
    if norm == "torch":
        return nn.BatchNorm2d(channels)
    raise ValueError(f"norm must be 'torch' or 'hip', got {norm!r}")


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin: int, width: int, stride: int = 1,
                 downsample: nn.Module = None, norm: str = "torch",
                 conv: str = "torch"):
        super().__init__()
        self.norm = norm
        self.conv1 = conv1x1(cin, width, conv=conv)
        self.bn1 = _norm(norm, width, "relu")
        self.conv2 = conv3x3(width, width, stride, conv=conv)
        self.bn2 = _norm(norm, width, "relu")
        self.conv3 = conv1x1(width, width * self.expansion, conv=conv)
        self.bn3 = _norm(norm, width * self.expansion, "relu")
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x
        if self.norm == "hip":
            out = self.bn1(self.conv1(x))
            out = self.bn2(self.conv2(out))
            if self.downsample is not None:
                identity = self.downsample(x)
            return self.bn3(self.conv3(out), residual=identity)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, layers, num_classes: int = 1000, norm: str = "torch",
                 conv: str = "torch"):
        super().__init__()
        self.inplanes = 64
        self.norm, self.conv = norm, conv
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(norm, 64, "relu")
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = HipLinear(512 * Bottleneck.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, HipConv2d)):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, width: int, blocks: int, stride: int = 1):
        downsample = None
        cout = width * Bottleneck.expansion
        if stride != 1 or self.inplanes != cout:
            downsample = nn.Sequential(
                conv1x1(self.inplanes, cout, stride, self.conv),
                _norm(self.norm, cout, "none"))
        layers = [Bottleneck(self.inplanes, width, stride, downsample,
                             self.norm, self.conv)]
        self.inplanes = cout
        layers += [Bottleneck(cout, width, norm=self.norm, conv=self.conv)
                   for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.bn1(self.conv1(x))
        x = self.maxpool(x if self.norm == "hip" else self.relu(x))
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet50(num_classes: int = 1000, norm: str = "torch",
             conv: str = "torch") -> ResNet:
    return ResNet([3, 4, 6, 3], num_classes, norm, conv)
