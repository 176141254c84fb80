"""GPU tests for the tiled self-attention kernels (k_attn_tiled_* in
csrc/attention_kernels.hip) and what reaches them: sequences above 64 tokens.

The instruments, the fp64 reference from the STORED operands, the torch
yardstick in the storage dtype and the bound e_ours <= 4 * max(e_torch, eps)
are tests/test_attention_gpu.py's."""

import pytest
import torch

from mi355x_ddp import ops
from mi355x_ddp.models import VisionTransformer
from test_attention_gpu import (DEV, EPS, _guarded, _held, _out_and_grads,
                                _pads_intact, _zeros)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                                 ids=["f32", "bf16"])
NAMES = ("out", "dQ", "dK", "dV")
SHAPES = [(1, 1, 64, 16),    # exactly one block
          (1, 1, 65, 16),    # one key and one query row in the second block
          (2, 3, 81, 16),    # a 17-row tail, batch and head strides
          (1, 2, 128, 32),   # two full blocks
          (1, 2, 129, 32),   # two full blocks plus a one-row tail
          (1, 2, 197, 64),   # the ViT-B/16 token count
          (1, 1, 1, 64)]     # N = 1 through the tiled path


def _tiled(x, dout, H, dtype):
    """(ours, torchs, refs), each (out, dQ, dK, dV): attn_tiled_fwd and
    attn_tiled_bwd on guarded copies of x [B, N, 3, E] and dout, the torch
    yardstick and the fp64 reference from the same stored operands."""
    B, N, _, E = x.shape
    qbuf, qkv = _guarded((B, N, 3 * E), dtype, x.view(B, N, 3 * E))
    dbuf, dout = _guarded((B, N, E), dtype, dout)
    obuf, out = _guarded((B, N, E), dtype)
    sbuf, stats = _guarded((B, H, N, 2), torch.float32)
    gbuf, dqkv = _guarded((B, N, 3 * E), dtype)
    ext = ops.ext()
    ext.attn_tiled_fwd(qkv, H, out=out, row_stats=stats)
    ext.attn_tiled_bwd(dout, qkv, out, stats, H, dqkv=dqkv)
    torch.cuda.synchronize()
    assert _pads_intact(qbuf, dbuf, obuf, sbuf, gbuf)
    refs = _out_and_grads(qkv.double(), dout.double(), H)
    ours = (out, *dqkv.view(B, N, 3, E).unbind(2))
    return ours, _out_and_grads(qkv, dout, H), refs


@DTYPES
@pytest.mark.parametrize("kind", ["normal", "peaked", "offset", "ramp", "fall"])
@pytest.mark.parametrize("B,H,N,D", SHAPES)
def test_kernels_against_fp64(B, H, N, D, kind, dtype):
    E = H * D
    g = torch.Generator().manual_seed(1000 * N + D)
    x = torch.randn(B, N, 3, E, generator=g)
    if kind == "peaked":  # near one-hot softmax; overflows without the max
        x[:, :, :2] *= 6
    elif kind == "offset":  # a big per-row score offset that cancels exactly
        x[:, :, 1] += 16
    elif kind in ("ramp", "fall"):
        # the running max rises in every key block (ramp), or sits in the
        # first with underflow after it (fall): the rescale in both directions
        t = torch.arange(N) / N
        t = (t if kind == "ramp" else 1 - t).view(1, N, 1)
        x[:, :, 0] = x[:, :, 0].abs()
        x[:, :, 1] = x[:, :, 1].abs() * (0.25 + 4 * t)
    results = _tiled(x, torch.randn(B, N, E, generator=g), H, dtype)
    assert not _held(NAMES, *results, EPS[dtype])


@DTYPES
def test_each_backward_kernel_alone(dtype):
    """Small integers, exact in bf16, at N = 129, D = 16: the second key
    block's dK/dV rows and the second query block's dQ rows on their own,
    every other block's inputs nonzero. A dropped or doubled block, or a
    delta from the wrong row, is an O(1) error here."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (1, 129, 3, 16), generator=g).float()
    dout = torch.randint(-2, 3, (1, 129, 16), generator=g).float()
    block = [[t[:, 64:128] for t in result[1:]]
             for result in _tiled(x, dout, 1, dtype)]
    assert not _held(NAMES[1:], *block, EPS[dtype])


@pytest.mark.parametrize("N,fwd,bwd", [(64, "attn_fwd", "attn_bwd"),
                                       (65, "attn_tiled_fwd", "attn_tiled_bwd")])
def test_dispatch_is_bitwise_the_kernels(N, fwd, bwd):
    H, E = 2, 32
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(2, N, 3 * E, generator=g).to(DEV).requires_grad_(True)
    dout = torch.randn(2, N, E, generator=g).to(DEV)
    out = ops.self_attention(qkv, H)
    out.backward(dout)
    ext = ops.ext()
    want, stats = getattr(ext, fwd)(qkv.detach(), H)
    saved = (want, stats) if N > 64 else (stats,)
    dqkv = getattr(ext, bwd)(dout, qkv.detach(), *saved, H)
    assert torch.equal(out, want) and torch.equal(qkv.grad, dqkv)


GUARDS = {  # name -> (qkv, heads, the operand only the backward refuses)
    "N=4097": lambda: (_zeros(1, 4097, 48), 1, None),
    "D=48": lambda: (_zeros(1, 4, 144), 1, None),
    "strided": lambda: (_zeros(2, 4, 192)[:, :, :96], 2, None),
    "out shape": lambda: (_zeros(1, 4, 96), 2, "out"),
    "dout dtype": lambda: (_zeros(1, 4, 96), 2, "dout"),
    "cpu": lambda: (_zeros(1, 4, 96, device="cpu"), 2, None),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    qkv, heads, bwd_only = GUARDS[name]()
    B, N, E3 = qkv.shape
    nan = float("nan")
    out = torch.full((B, N, E3 // 3), nan, device=DEV)
    dqkv = torch.full((B, N, E3), nan, device=DEV)
    ext = ops.ext()
    if bwd_only is None:
        with pytest.raises(RuntimeError):
            ext.attn_tiled_fwd(qkv, heads, out=out)
    dout = _zeros(B, N, E3 // 3, device=qkv.device,
                  dtype=torch.bfloat16 if bwd_only == "dout" else qkv.dtype)
    fwd_out = _zeros(B, N + (bwd_only == "out"), E3 // 3, device=qkv.device)
    with pytest.raises(RuntimeError):
        ext.attn_tiled_bwd(dout, qkv, fwd_out, _zeros(B, heads, N, 2), heads,
                           dqkv=dqkv)
    torch.cuda.synchronize()
    assert out.isnan().all() and dqkv.isnan().all()


def test_vit_with_82_tokens_against_fp64_model():
    def build(attention):
        return VisionTransformer(image_size=144, patch=16, layers=2,
                                 hidden=64, heads=4, mlp=128, num_classes=10,
                                 attention=attention)

    def run(mod, x, dy):
        y = mod(x)
        y.backward(dy)
        return [y.detach().to(DEV)] + [p.grad.to(DEV) for _, p in sorted(
            mod.named_parameters())]

    torch.manual_seed(5)
    base = build("torch").to(DEV)
    ours = build("hip").to(DEV)
    ours.load_state_dict(base.state_dict())
    ref = build("torch").double()  # on the CPU: the head's kernels have no fp64
    ref.load_state_dict(base.state_dict())
    x = torch.rand(2, 3, 144, 144, device=DEV)
    dy = torch.randn(2, 10, device=DEV)
    names = ["out"] + sorted(n for n, _ in base.named_parameters())
    assert not _held(names, run(ours, x, dy), run(base, x, dy),
                     run(ref, x.double().cpu(), dy.double().cpu()),
                     EPS[torch.float32])
