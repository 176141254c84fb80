"""GPU tests for the bf16 wide-MFMA self-attention kernels (k_attn_bf16_* in
csrc/attention_kernels.hip) and what reaches them: `matrix="bf16"` and
`attention="hip-bf16"`.

The instruments, the fp64 reference from the STORED operands, the torch
yardstick in bf16 and the bound e_ours <= 4 * max(e_torch, 2^-9) are
tests/test_attention_gpu.py's."""

import pytest
import torch

from mi355x_ddp import ops
from mi355x_ddp.models import VisionTransformer
from test_attention_gpu import (DEV, EPS, _guarded, _held, _out_and_grads,
                                _pads_intact, _zeros)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAMES = ("out", "dQ", "dK", "dV")
SHAPES = [(1, 1, 1, 32),     # out == V, dS == 0
          (1, 1, 17, 32),    # a 1-row second MFMA tile in a half-filled step
          (2, 3, 48, 32),    # one and a half wide steps, batch/head strides
          (1, 1, 64, 64),    # exactly one block
          (1, 1, 65, 64),    # one key and one query row in the second block
          (1, 2, 129, 32),   # two full blocks plus a one-row tail
          (1, 2, 197, 64)]   # the ViT-B/16 token count


def _wide(x, dout, H):
    """(ours, torchs, refs), each (out, dQ, dK, dV): attn_bf16_fwd and
    attn_bf16_bwd on guarded bf16 copies of x [B, N, 3, E] and dout, the torch
    yardstick and the fp64 reference from the same stored operands."""
    B, N, _, E = x.shape
    qbuf, qkv = _guarded((B, N, 3 * E), BF16, x.view(B, N, 3 * E))
    dbuf, dout = _guarded((B, N, E), BF16, dout)
    obuf, out = _guarded((B, N, E), BF16)
    sbuf, stats = _guarded((B, H, N, 2), torch.float32)
    gbuf, dqkv = _guarded((B, N, 3 * E), BF16)
    ext = ops.ext()
    ext.attn_bf16_fwd(qkv, H, out=out, row_stats=stats)
    ext.attn_bf16_bwd(dout, qkv, out, stats, H, dqkv=dqkv)
    torch.cuda.synchronize()
    assert _pads_intact(qbuf, dbuf, obuf, sbuf, gbuf)
    refs = _out_and_grads(qkv.double(), dout.double(), H)
    ours = (out, *dqkv.view(B, N, 3, E).unbind(2))
    return ours, _out_and_grads(qkv, dout, H), refs


@pytest.mark.parametrize("kind", ["normal", "peaked", "offset", "ramp", "fall"])
@pytest.mark.parametrize("B,H,N,D", SHAPES)
def test_kernels_against_fp64(B, H, N, D, kind):
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
    results = _wide(x, torch.randn(B, N, E, generator=g), H)
    assert not _held(NAMES, *results, EPS[BF16])


@pytest.mark.parametrize("D", [32, 64])
def test_uniform_attention_is_exact(D):
    """Q = 0 makes P = 1/128 in every place, exact in bf16, and small integer
    V and dout make every sum exact in f32: out and dV are the fp64 results
    rounded once, dK is 0. A dropped, doubled or mis-permuted key in a wide
    step, or a transposed image read at the wrong offset, is a multiple of
    1/128 here."""
    H, N = 2, 128
    g = torch.Generator().manual_seed(D)
    x = torch.randn(1, N, 3, H * D, generator=g)
    x[:, :, 0] = 0
    x[:, :, 2] = torch.randint(-2, 3, (1, N, H * D), generator=g).float()
    dout = torch.randint(-2, 3, (1, N, H * D), generator=g).float()
    ours, torchs, refs = _wide(x, dout, H)
    assert torch.equal(ours[0], refs[0].to(BF16))
    assert torch.equal(ours[3], refs[3].to(BF16))
    assert bool((ours[2] == 0).all())
    assert not _held(NAMES[1:2], ours[1:2], torchs[1:2], refs[1:2], EPS[BF16])


def test_each_backward_kernel_alone():
    """Small integers at N = 129, D = 32: the second key block's dK/dV rows
    and the second query block's dQ rows on their own, every other block's
    inputs nonzero."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (1, 129, 3, 32), generator=g).float()
    dout = torch.randint(-2, 3, (1, 129, 32), generator=g).float()
    block = [[t[:, 64:128] for t in result[1:]]
             for result in _wide(x, dout, 1)]
    assert not _held(NAMES[1:], *block, EPS[BF16])


@pytest.mark.parametrize("N", [50, 65])
def test_dispatch_is_bitwise_the_kernels(N):
    H, E = 2, 64
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(2, N, 3 * E, generator=g).to(DEV, BF16)
    qkv.requires_grad_(True)
    dout = torch.randn(2, N, E, generator=g).to(DEV, BF16)
    out = ops.self_attention(qkv, H, matrix="bf16")
    out.backward(dout)
    ext = ops.ext()
    want, stats = ext.attn_bf16_fwd(qkv.detach(), H)
    dqkv = ext.attn_bf16_bwd(dout, qkv.detach(), want, stats, H)
    assert torch.equal(out, want) and torch.equal(qkv.grad, dqkv)
    with pytest.raises(ValueError):
        ops.self_attention(qkv.detach().float(), H, matrix="bf16")


def _z16(*shape):
    return _zeros(*shape, dtype=BF16)


GUARDS = {  # name -> (qkv, heads, the operand only the backward refuses)
    "f32": lambda: (_zeros(1, 4, 192), 2, None),
    "D=16": lambda: (_z16(1, 4, 96), 2, None),
    "D=48": lambda: (_z16(1, 4, 144), 1, None),
    "N=4097": lambda: (_z16(1, 4097, 96), 1, None),
    "strided": lambda: (_z16(2, 4, 384)[:, :, :192], 2, None),
    "out shape": lambda: (_z16(1, 4, 192), 2, "out"),
    "dout dtype": lambda: (_z16(1, 4, 192), 2, "dout"),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    qkv, heads, bwd_only = GUARDS[name]()
    B, N, E3 = qkv.shape
    nan = float("nan")
    out = torch.full((B, N, E3 // 3), nan, device=DEV, dtype=qkv.dtype)
    dqkv = torch.full((B, N, E3), nan, device=DEV, dtype=qkv.dtype)
    ext = ops.ext()
    if bwd_only is None:
        with pytest.raises(RuntimeError):
            ext.attn_bf16_fwd(qkv, heads, out=out)
    dout = _zeros(B, N, E3 // 3,
                  dtype=torch.float32 if bwd_only == "dout" else qkv.dtype)
    fwd_out = _zeros(B, N + (bwd_only == "out"), E3 // 3, dtype=qkv.dtype)
    with pytest.raises(RuntimeError):
        ext.attn_bf16_bwd(dout, qkv, fwd_out, _zeros(B, heads, N, 2), heads,
                          dqkv=dqkv)
    torch.cuda.synchronize()
    assert out.isnan().all() and dqkv.isnan().all()


def test_vit_with_82_tokens_under_autocast_against_fp64_model():
    def build(attention):
        return VisionTransformer(image_size=144, patch=16, layers=2,
                                 hidden=128, heads=4, mlp=128, num_classes=10,
                                 attention=attention)

    def run(mod, x, dy, autocast):
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            y = mod(x)
        y.backward(dy.to(y.dtype))
        return [y.detach().to(DEV)] + [p.grad.to(DEV) for _, p in sorted(
            mod.named_parameters())]

    torch.manual_seed(5)
    base = build("torch").to(DEV)
    ours = build("hip-bf16").to(DEV)
    assert ours.state_dict().keys() == build("hip").state_dict().keys()
    ours.load_state_dict(base.state_dict())
    ref = build("torch").double()  # on the CPU: the head's kernels have no fp64
    ref.load_state_dict(base.state_dict())
    x = torch.rand(2, 3, 144, 144, device=DEV)
    dy = torch.randn(2, 10, device=DEV)
    names = ["out"] + sorted(n for n, _ in base.named_parameters())
    assert not _held(names, run(ours, x, dy, True), run(base, x, dy, True),
                     run(ref, x.double().cpu(), dy.double().cpu(), False),
                     EPS[BF16])
