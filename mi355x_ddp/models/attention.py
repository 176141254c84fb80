"""Self-attention block over the fused attention kernels (any N up to 4096:
one workgroup per head up to 64 tokens, the tiled kernels above).

`HipSelfAttention` is `nn.MultiheadAttention(embed_dim, num_heads,
batch_first=True)` restricted to what ViT uses (self-attention, no mask, no
dropout, weights not returned) with the same parameter names, shapes and
initialisation, so state dicts and snapshots interchange in both directions.
Its forward is `ops.linear` -> `ops.self_attention` -> `ops.linear`: the
attention kernel reads the in-projection's packed [B, N, 3E] output where it
lies and writes [B, N, E] for the out-projection, so no per-head copy exists.
`matrix="bf16"` selects the wide bf16 MFMA kernels (`ops.self_attention`'s
argument of that name: bf16 activations or bf16 autocast, heads of 32 or 64);
the default `"f32"` keeps the exact-fp32 products. Parameters do not depend
on it.
"""

from __future__ import annotations

import torch
from torch import nn

from .. import ops


class HipSelfAttention(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, matrix: str = "f32"):
        super().__init__()
        if embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        if matrix not in ("f32", "bf16"):
            raise ValueError(f"matrix must be 'f32' or 'bf16', got {matrix!r}")
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.matrix = matrix
        self.in_proj_weight = nn.Parameter(
            torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        # nn.MultiheadAttention's order of random draws: out_proj at
        # construction, then the in-projection
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.in_proj_bias)
        nn.init.zeros_(self.out_proj.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B, N, E] -> [B, N, E]."""
        qkv = ops.linear(x, self.in_proj_weight, self.in_proj_bias)
        y = ops.self_attention(qkv, self.num_heads, self.matrix)
        return ops.linear(y, self.out_proj.weight, self.out_proj.bias)
