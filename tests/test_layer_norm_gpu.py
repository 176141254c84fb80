"""GPU tests for the fused LayerNorm kernels (csrc/layernorm_kernels.hip) and
what reaches them.

Reference: F.layer_norm and its autograd gradients in fp64 from the STORED
operands (with a residual, from the stored s the kernel returned). Yardstick:
F.layer_norm in the storage dtype on the device. With
e = max|got - ref| / max|ref| per result, e_ours <= 4 * max(e_torch, eps),
eps = 2^-24 (f32) or 2^-9 (bf16): the bound of tests/test_attention_gpu.py."""

import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipLayerNorm, vit_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # sentinel elements on either side; keeps 16-byte alignment
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                                 ids=["f32", "bf16"])
G = 512  # kLnGridCap, checked against ext().ln_grid_cap() below
SHAPES = [(1, 4), (3, 252), (5, 256), (4, 260), (7, 64), (9, 1024),
          (2, 1284), (6, 2048), (4 * G + 7, 64)]
LN_EPS = 1e-6


def _err(got, ref):
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


def _guarded(shape, dtype, src=None):
    """A view of `shape` inside a larger NaN-filled allocation."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _pads_intact(*bufs):
    return all(bool(b[:PAD].isnan().all() and b[-PAD:].isnan().all())
               for b in bufs)


def _held(names, ours, torchs, refs, eps):
    bad = []
    for name, o, t, ref in zip(names, ours, torchs, refs):
        e_o, e_t = _err(o, ref), _err(t, ref)
        bound = 4 * max(e_t, eps)
        print(f"{name}: e_ours {e_o:.3e} e_torch {e_t:.3e} "
              f"ratio {e_o / bound:.3f}")
        if not e_o <= bound:  # catches NaN too
            bad.append((name, e_o, bound))
    return bad


def _ln_and_grads(x, w, b, dy, ds=None):
    """(y, dx, dgamma, dbeta) of F.layer_norm in the operands' dtype."""
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(x, x.shape[-1:], w, b, LN_EPS)
    y.backward(dy)
    return (y.detach(), x.grad if ds is None else x.grad + ds, w.grad, b.grad)


def _inputs(R, E, kind, dtype):
    """Guarded (x, r, w, b, dy, ds): ([buffers], [views])."""
    assert ops.ext().ln_grid_cap() == G
    g = torch.Generator().manual_seed(10000 * R + E)
    x = torch.randn(R, E, generator=g)
    if kind == "offset":
        x += 1000 if dtype == torch.float32 else 64
    elif kind == "scaled":
        x *= torch.logspace(-3, 3, R).unsqueeze(1)
    srcs = [x, torch.randn(R, E, generator=g),
            1 + 0.5 * torch.randn(E, generator=g), torch.randn(E, generator=g),
            torch.randn(R, E, generator=g), torch.randn(R, E, generator=g)]
    return zip(*(_guarded(s.shape, dtype, s) for s in srcs))


def _outputs(R, E, dtype):
    """Guarded (y, stats, s, dx, dgamma, dbeta): ([buffers], [views])."""
    return zip(*(_guarded(shape, dt) for shape, dt in [
        ((R, E), dtype), ((R, 2), torch.float32), ((R, E), dtype),
        ((R, E), dtype), ((E,), dtype), ((E,), dtype)]))


def _run(ins, outs, residual):
    x, r, w, b, dy, ds = ins
    y, stats, s, dx, dgamma, dbeta = outs
    ext = ops.ext()
    if residual:
        ext.ln_fwd(x, w, b, LN_EPS, residual=r, y=y, row_stats=stats, s=s)
    else:
        ext.ln_fwd(x, w, b, LN_EPS, y=y, row_stats=stats)
    ext.ln_bwd(dy, s if residual else x, stats, w,
               ds=ds if residual else None, dx=dx, dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()


@DTYPES
@pytest.mark.parametrize("kind", ["normal", "offset", "scaled"])
@pytest.mark.parametrize("residual", [False, True], ids=["ln", "add_ln"])
@pytest.mark.parametrize("R,E", SHAPES)
def test_kernels_against_fp64(R, E, residual, kind, dtype):
    ibufs, ins = _inputs(R, E, kind, dtype)
    obufs, outs = _outputs(R, E, dtype)
    _run(ins, outs, residual)
    assert _pads_intact(*ibufs, *obufs)
    x, r, w, b, dy, ds = ins
    y, _, s, dx, dgamma, dbeta = outs
    if residual:
        assert torch.equal(s, (x.float() + r.float()).to(dtype))
    lin, ds = (s, ds) if residual else (x, None)
    refs = _ln_and_grads(*(t.double() for t in (lin, w, b, dy)),
                         None if ds is None else ds.double())
    torchs = _ln_and_grads(lin, w, b, dy, ds)
    assert not _held(("y", "dx", "dgamma", "dbeta"), (y, dx, dgamma, dbeta),
                     torchs, refs, EPS[dtype])


@DTYPES
@pytest.mark.parametrize("R,E", [s for s in SHAPES if s[0] > 1])
def test_dbeta_exact(R, E, dtype):
    _, ins = _inputs(R, E, "normal", dtype)
    _, outs = _outputs(R, E, dtype)
    i, j = torch.arange(R).unsqueeze(1), torch.arange(E).unsqueeze(0)
    ins[4].copy_((7 * i + 3 * j) % 11 - 5)  # every partial sum is exact
    _run(ins, outs, False)
    want = ins[4].double().sum(0)
    assert torch.equal(outs[5], want.to(dtype))
    if dtype == torch.float32:
        assert torch.equal(outs[5].double(), want)


@DTYPES
@pytest.mark.parametrize("R,E", [(4 * G + 7, 64), (9, 1024)])
def test_backward_is_reproducible(R, E, dtype):
    _, ins = _inputs(R, E, "normal", dtype)
    runs = []
    for _ in range(2):
        _, outs = _outputs(R, E, dtype)
        _run(ins, outs, True)
        runs.append(outs[3:])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _zeros(*shape, dtype=torch.float32, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


GUARDS = {  # name -> (x, weight, residual, dy dtype if only the bwd refuses)
    "E=6": lambda: (_zeros(2, 6), _zeros(6), None, None),
    "E=2052": lambda: (_zeros(2, 2052), _zeros(2052), None, None),
    "short weight": lambda: (_zeros(2, 64), _zeros(60), None, None),
    "weight dtype": lambda: (_zeros(2, 64),
                             _zeros(64, dtype=torch.bfloat16), None, None),
    "strided": lambda: (_zeros(4, 128)[:, :64], _zeros(64), None, None),
    "residual shape": lambda: (_zeros(2, 64), _zeros(64), _zeros(1, 64), None),
    "cpu": lambda: (_zeros(2, 64, device="cpu"), _zeros(64, device="cpu"),
                    None, None),
    "dy dtype": lambda: (_zeros(2, 64), _zeros(64), None, torch.bfloat16),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    x, w, r, dy_dtype = GUARDS[name]()
    R, E = x.shape
    nan = float("nan")
    y, s, dx = (torch.full((R, E), nan, device=DEV) for _ in range(3))
    dgamma, dbeta = (torch.full((w.numel(),), nan, dtype=w.dtype, device=DEV)
                     for _ in range(2))
    ext = ops.ext()
    if dy_dtype is None:
        with pytest.raises(RuntimeError):
            ext.ln_fwd(x, w, w, LN_EPS, residual=r, y=y,
                       s=None if r is None else s)
    dy = _zeros(R, E, dtype=dy_dtype or x.dtype, device=x.device)
    with pytest.raises(RuntimeError):
        ext.ln_bwd(dy, x, _zeros(R, 2, device=x.device), w, ds=r, dx=dx,
                   dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    assert all(t.isnan().all() for t in (y, s, dx, dgamma, dbeta))


def test_empty_rows_launch_nothing():
    w, b = (_zeros(64).requires_grad_(True) for _ in range(2))
    x = _zeros(0, 5, 64).requires_grad_(True)
    y = ops.layer_norm(x, w, b)
    s, y2 = ops.add_layer_norm(x, _zeros(0, 5, 64), w, b)
    assert y.shape == s.shape == y2.shape == x.shape
    (y.sum() + s.sum() + y2.sum()).backward()
    assert x.grad.shape == x.shape
    assert w.grad.shape == b.grad.shape == (64,)
    assert not w.grad.any() and not b.grad.any()


def _run_module(mod, x, dy):
    for p in mod.parameters():
        p.grad = None
    y = mod(x)
    y.backward(dy)
    return [y.detach()] + [p.grad for _, p in sorted(mod.named_parameters())]


def test_module_and_vit_tiny():
    torch.manual_seed(5)
    ln = nn.LayerNorm(256, eps=LN_EPS).to(DEV)
    with torch.no_grad():
        ln.weight.normal_(1, 0.5), ln.bias.normal_()
    hip = HipLayerNorm(256, eps=LN_EPS).to(DEV)
    hip.load_state_dict(ln.state_dict())
    x, dy = torch.randn(2, 3, 17, 256, device=DEV).unbind(0)
    ref = nn.LayerNorm(256, eps=LN_EPS).to(DEV).double()
    ref.load_state_dict(ln.state_dict())
    assert not _held(("y", "bias", "weight"), _run_module(hip, x, dy),
                     _run_module(ln, x, dy),
                     _run_module(ref, x.double(), dy.double()),
                     EPS[torch.float32])

    base = vit_tiny().to(DEV)
    ours = vit_tiny(norm="hip").to(DEV)
    ours.load_state_dict(base.state_dict())
    ref = vit_tiny().double()  # on the CPU: the head's kernels have no fp64
    ref.load_state_dict(base.state_dict())
    x = torch.rand(4, 3, 64, 64, device=DEV)
    dy = torch.randn(4, 10, device=DEV)
    refs = _run_module(ref, x.double().cpu(), dy.double().cpu())
    names = ["out"] + sorted(n for n, _ in base.named_parameters())
    assert not _held(names, _run_module(ours, x, dy), _run_module(base, x, dy),
                     [t.to(DEV) for t in refs], EPS[torch.float32])
