"""ViT-L/32, defined locally (torchvision is not installed here).

The reference profile stage imports `vit_l_32` alongside `resnet50`
(reference multigpu_profile.py:14) but leaves it commented out at :24;
this module completes that capability so the profile entrypoint can run
either workload (`MI355X_PROFILE_MODEL=vit`). Architecture matches
torchvision's `vit_l_32` (ViT-Large, 32x32 patches, 224 input: 24 layers,
hidden 1024, MLP 4096, 16 heads, learned position embeddings, pre-norm
encoder blocks, class token head) so the parameter census and DDP
gradient payload (~305 M params, ~1.2 GB fp32 grads) are the real thing.

The classifier head uses the hand-written MFMA linear. The encoder MLP is
`mlp="torch"` (`nn.Sequential(Linear, GELU, Linear)` through PyTorch-ROCm,
the default) or `mlp="hip"` (`HipMlp`: the tiled MFMA GEMMs with the bias
adds, GELU, GELU' and the bias gradients in their epilogues). LayerNorm
is `norm="torch"` (`nn.LayerNorm`, the default) or `norm="hip"`
(`HipLayerNorm`: the fused row kernels, with the residual add in front of
`ln_2` folded into it). Attention is `attention="torch"`
(`nn.MultiheadAttention`, the default), `attention="hip"`
(`HipSelfAttention`: the fused attention kernels, any N up to 4096 tokens,
heads of 16, 32 or 64, exact-fp32 products) or `attention="hip-bf16"`
(`HipSelfAttention(matrix="bf16")`: the wide bf16 MFMA kernels, for bf16
activations or bf16 autocast, heads of 32 or 64). The three switches are independent, and every
combination has the same parameters under the same names. In
`VisionTransformer` and `EncoderBlock`, where `mlp` already is the MLP's
width, the switch is spelled `mlp_impl`; `vit_l_32`, `vit_b_16` and `vit_tiny`
take it as `mlp`.
"""

from __future__ import annotations

import torch
from torch import nn

from .attention import HipSelfAttention
from .layernorm import HipLayerNorm
from .mlp import HipMlp
from .toy import HipLinear


def _layer_norm(norm: str, hidden: int) -> nn.Module:
    if norm not in ("torch", "hip"):
        raise ValueError(f"norm must be 'torch' or 'hip', got {norm!r}")
    cls = HipLayerNorm if norm == "hip" else nn.LayerNorm
    return cls(hidden, eps=1e-6)


class EncoderBlock(nn.Module):
    def __init__(self, hidden: int, heads: int, mlp: int,
                 attention: str = "torch", norm: str = "torch",
                 mlp_impl: str = "torch"):
        super().__init__()
        if attention not in ("torch", "hip", "hip-bf16"):
            raise ValueError(f"attention must be 'torch', 'hip' or "
                             f"'hip-bf16', got {attention!r}")
        if mlp_impl not in ("torch", "hip"):
            raise ValueError(f"mlp_impl (mlp= of vit_l_32 / vit_tiny) must be "
                             f"'torch' or 'hip', got {mlp_impl!r}")
        self.hip_attention = attention != "torch"
        self.hip_norm = norm == "hip"
        self.ln_1 = _layer_norm(norm, hidden)
        if self.hip_attention:
            self.self_attention = HipSelfAttention(
                hidden, heads, "bf16" if attention == "hip-bf16" else "f32")
        else:
            self.self_attention = nn.MultiheadAttention(hidden, heads,
                                                        batch_first=True)
        self.ln_2 = _layer_norm(norm, hidden)
        if mlp_impl == "hip":
            self.mlp = HipMlp(hidden, mlp)
        else:
            self.mlp = nn.Sequential(
                nn.Linear(hidden, mlp), nn.GELU(), nn.Linear(mlp, hidden))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.ln_1(x)
        if self.hip_attention:
            y = self.self_attention(y)
        else:
            y, _ = self.self_attention(y, y, y, need_weights=False)
        if self.hip_norm:  # x + y and ln_2 of it in one pass
            x, y = self.ln_2(y, residual=x)
            return x + self.mlp(y)
        x = x + y
        return x + self.mlp(self.ln_2(x))


class VisionTransformer(nn.Module):
    def __init__(self, image_size: int = 224, patch: int = 32,
                 layers: int = 24, hidden: int = 1024, heads: int = 16,
                 mlp: int = 4096, num_classes: int = 1000,
                 attention: str = "torch", norm: str = "torch",
                 mlp_impl: str = "torch"):
        super().__init__()
        self.patch = patch
        self.conv_proj = nn.Conv2d(3, hidden, kernel_size=patch, stride=patch)
        n_tokens = (image_size // patch) ** 2 + 1
        self.class_token = nn.Parameter(torch.zeros(1, 1, hidden))
        self.pos_embedding = nn.Parameter(
            torch.empty(1, n_tokens, hidden).normal_(std=0.02))
        self.encoder = nn.ModuleList(
            EncoderBlock(hidden, heads, mlp, attention, norm, mlp_impl)
            for _ in range(layers))
        self.ln = _layer_norm(norm, hidden)
        self.head = HipLinear(hidden, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.conv_proj(x)                       # [B, H, gh, gw]
        x = x.flatten(2).transpose(1, 2)            # [B, tokens, H]
        cls = self.class_token.expand(x.shape[0], -1, -1)
        x = torch.cat([cls, x], dim=1) + self.pos_embedding
        for blk in self.encoder:
            x = blk(x)
        return self.head(self.ln(x[:, 0]))


def vit_l_32(num_classes: int = 1000, attention: str = "torch",
             norm: str = "torch", mlp: str = "torch") -> VisionTransformer:
    return VisionTransformer(num_classes=num_classes, attention=attention,
                             norm=norm, mlp_impl=mlp)


def vit_b_16(num_classes: int = 1000, attention: str = "torch",
             norm: str = "torch", mlp: str = "torch") -> VisionTransformer:
    """torchvision's `vit_b_16`: 197 tokens at 224 px."""
    return VisionTransformer(patch=16, layers=12, hidden=768, heads=12,
                             mlp=3072, num_classes=num_classes,
                             attention=attention, norm=norm, mlp_impl=mlp)


def vit_tiny(num_classes: int = 10, attention: str = "torch",
             norm: str = "torch", mlp: str = "torch") -> VisionTransformer:
    """Small configuration for tests."""
    return VisionTransformer(image_size=64, patch=16, layers=2, hidden=64,
                             heads=4, mlp=128, num_classes=num_classes,
                             attention=attention, norm=norm, mlp_impl=mlp)
