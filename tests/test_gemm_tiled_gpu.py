"""GPU tests for the tiled MFMA GEMMs (csrc/gemm_kernels.hip) and what reaches
them: gemm_nt / gemm_nn / gemm_tn, ops.mlp, HipMlp, vit_tiny(mlp="hip").

GEMM outputs: elementwise against the fp64 product of the STORED operands
(tests/kernel_oracle.py: matmul_tol for f32, gemm_bf16_tol for bf16, n_terms
the contraction length), and on integer-coded operands exactly. GELU
epilogues and autograd: e = max|got - ref| / max|ref| against fp64,
e_ours <= 4 * max(e_torch, eps), eps = 2^-24 (f32) or 2^-9 (bf16), torch's
device result of the same formula in the storage dtype as yardstick (the
bound of tests/test_layer_norm_gpu.py). Shapes sit on the edges of the tile
the extension reports."""

import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import kernel_oracle as ko
from mi355x_ddp import ops
from mi355x_ddp.models import HipMlp, vit_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                                 ids=["f32", "bf16"])
BM, BN, BK = ops.ext().gemm_tile_shape() if ops.has_ext() else (128, 128, 32)
# (rows, output columns, contraction) for NT and NN
ROW_CASES = [(1, 16, 16), (BM - 1, BN - 16, BK + 16),
             (BM + 1, BN + 16, 3 * BK - 16), (2 * BM + 3, 16, 3 * BK - 16),
             (BM + 1, BN - 16, 16), (2 * BM + 3, BN + 16, BK + 16)]
# (contraction rows, N, K) for TN: dw is [N, K]
TN_CASES = [(1, 16, 16), (BK - 1, BN - 16, BN + 16), (BK + 1, BN + 16, 16),
            (3 * BK + 5, 16, BN + 16), (3 * BK + 5, BN + 16, BN - 16)]


def _guarded(shape, dtype, src=None):
    """A view of `shape` inside a larger NaN-filled allocation."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _pads_intact(bufs):
    return all(bool(b[:PAD].isnan().all() and b[-PAD:].isnan().all())
               for b in bufs)


def _err(got, ref):
    d = float((got.double().cpu() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


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


def _operands(kind, dtype, a_shape, w_shape, n_bias):
    """Stored CPU operands (a, w, bias) of one kind."""
    if kind == "int":
        return (ko.int_a(*a_shape, dtype), ko.int_w(*w_shape, dtype),
                ko.int_bias(n_bias, dtype))
    scale = 8 if kind == "wide" else 1  # wide: |h| up to about 8
    return (ko.rand_signed(*a_shape, seed=1, dtype=dtype),
            ko.rand_signed(*w_shape, seed=2, dtype=dtype),
            (scale * ko.rand_signed(n_bias, seed=3)).to(dtype))


def _check(got, ref, S, n_terms, dtype, kind, what):
    if kind == "int":
        ko.assert_exact_int(got, ref, S, what)
    else:
        tol = (ko.gemm_bf16_tol(ref, S, n_terms) if dtype == ko.BF16
               else ko.matmul_tol(ref, S, n_terms, dtype))
        print(what, "worst error/tol", ko.assert_within(got, ref, tol, what))


def _gelu_grad64(h):
    return 0.5 * (1 + torch.erf(h / math.sqrt(2))) \
        + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


@DTYPES
@pytest.mark.parametrize("kind", ["real", "wide", "int"])
@pytest.mark.parametrize("M,N,K", ROW_CASES)
def test_nt_and_nn_against_fp64(M, N, K, kind, dtype):
    ext = ops.ext()
    x, w, b = _operands(kind, dtype, (M, K), (N, K), N)
    bufs, (xd, wd, bd, y, h, a) = zip(*(
        _guarded(s.shape, dtype, s) for s in (x, w, b)),
        *(_guarded((M, N), dtype) for _ in range(3)))
    ext.gemm_nt(xd, wd, bias=bd, y=y)
    ext.gemm_nt(xd, wd, bias=bd, gelu=True, y=a, h=h)
    ref, S = ko.linear_fwd_ref(x, w, b)
    _check(y, ref, S, K, dtype, kind, "y")
    _check(h, ref, S, K, dtype, kind, "h")
    assert ko.worst_ratio(h, ko.widen(y), 1.0) == 0  # one GEMM, two epilogues

    # NN: dy [M, K] (contraction K), w2 [K, N]; h has the output's shape
    dy, w2, _ = _operands(kind, dtype, (M, K), (K, N), 16)
    nbufs, (dyd, w2d, dx, dh) = zip(
        *(_guarded(s.shape, dtype, s) for s in (dy, w2)),
        *(_guarded((M, N), dtype) for _ in range(2)))
    ext.gemm_nn(dyd, w2d, dx=dx)
    ext.gemm_nn(dyd, w2d, gelu_grad_of=h, dx=dh)
    torch.cuda.synchronize()
    assert _pads_intact(bufs + nbufs)
    dref, dS = ko.linear_bwd_input_ref(dy, w2)
    _check(dx, dref, dS, K, dtype, kind, "dx")
    if kind != "int":
        h64 = ko.widen(h)
        refs = (F.gelu(h64), dref * _gelu_grad64(h64))
        torchs = (F.gelu(h), torch.ops.aten.gelu_backward(dyd @ w2d, h))
        assert not _held(("a", "dh"), (a, dh), torchs, refs, EPS[dtype])


@DTYPES
@pytest.mark.parametrize("kind", ["real", "int"])
@pytest.mark.parametrize("M,N,K", TN_CASES)
def test_tn_against_fp64_and_reproducible(M, N, K, kind, dtype):
    dy, x, _ = _operands(kind, dtype, (M, N), (M, K), 16)
    ibufs, (dyd, xd) = zip(*(_guarded(s.shape, dtype, s) for s in (dy, x)))
    runs = []
    for _ in range(2):
        obufs, (dw, db) = zip(_guarded((N, K), dtype), _guarded((N,), dtype))
        ops.ext().gemm_tn(dyd, xd, dw=dw, db=db)
        torch.cuda.synchronize()
        assert _pads_intact(ibufs + obufs)
        runs.append((dw, db))
    (wref, wS), (bref, bS) = ko.linear_bwd_weight_ref(x, dy)
    _check(dw, wref, wS, M, dtype, kind, "dw")
    _check(db, bref, bS, M, dtype, kind, "db")
    for first, second in zip(*runs):
        ko.assert_bitwise(first, second, "gemm_tn twice")


def _z(*shape, dtype=torch.float32, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


BF = torch.bfloat16
REFUSALS = {  # outputs o: y, h, dx [4, 16], dw [16, 32], db [16], NaN-filled
    "feature 24": lambda e, o: e.gemm_nt(_z(4, 24), _z(16, 24), gelu=True,
                                         y=o["y"], h=o["h"]),
    "dtypes": lambda e, o: e.gemm_tn(_z(4, 16), _z(4, 32, dtype=BF),
                                     dw=o["dw"], db=o["db"]),
    "strided": lambda e, o: e.gemm_nn(_z(4, 32), _z(32, 32)[:, :16],
                                      dx=o["dx"]),
    "cpu": lambda e, o: e.gemm_nt(_z(4, 32, device="cpu"),
                                  _z(16, 32, device="cpu"), y=o["y"]),
    "bias length": lambda e, o: e.gemm_nt(_z(4, 32), _z(16, 32),
                                          bias=_z(32), y=o["y"]),
    "gelu_grad_of shape": lambda e, o: e.gemm_nn(
        _z(4, 32), _z(32, 16), gelu_grad_of=_z(4, 32), dx=o["dx"]),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_refused_before_any_launch(name):
    shapes = dict(y=(4, 16), h=(4, 16), dx=(4, 16), dw=(16, 32), db=(16,))
    outs = {k: torch.full(s, float("nan"), device=DEV)
            for k, s in shapes.items()}
    with pytest.raises(RuntimeError):
        REFUSALS[name](ops.ext(), outs)
    torch.cuda.synchronize()
    assert all(t.isnan().all() for t in outs.values())


def test_empty_rows_through_mlp():
    w1, b1, w2, b2 = (_z(*s).requires_grad_(True)
                      for s in [(32, 16), (32,), (16, 32), (16,)])
    x = _z(0, 5, 16).requires_grad_(True)
    y = ops.mlp(x, w1, b1, w2, b2)
    assert y.shape == x.shape
    y.sum().backward()
    assert x.grad.shape == x.shape
    for p in (w1, b1, w2, b2):
        assert p.grad.shape == p.shape and not p.grad.any()


def _run_module(mod, x, dy):
    for p in mod.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(x.is_floating_point()
                                          and x.dim() == 3)
    y = mod(x)
    y.backward(dy)
    outs = [y.detach()] + [p.grad for _, p in sorted(mod.named_parameters())]
    return outs + ([x.grad] if x.requires_grad else [])


@DTYPES
def test_mlp_through_autograd(dtype):
    torch.manual_seed(7)
    base = nn.Sequential(nn.Linear(64, 128), nn.GELU(), nn.Linear(128, 64))
    base = base.to(DEV, dtype)
    hip = HipMlp(64, 128).to(DEV, dtype)
    hip.load_state_dict(base.state_dict())
    ref = nn.Sequential(nn.Linear(64, 128), nn.GELU(), nn.Linear(128, 64))
    ref = ref.double()
    ref.load_state_dict(base.state_dict())  # the stored (rounded) parameters
    x, dy = torch.randn(2, 3, 17, 64, device=DEV).to(dtype).unbind(0)
    refs = _run_module(ref, x.double().cpu(), dy.double().cpu())
    names = ["y", "0.bias", "0.weight", "2.bias", "2.weight", "dx"]
    assert not _held(names, _run_module(hip, x, dy), _run_module(base, x, dy),
                     refs, EPS[dtype])
    # ops.mlp itself, on the same parameters: the module adds nothing
    want = _run_module(hip, x, dy)
    p = dict(hip.named_parameters())
    x2 = x.detach().clone().requires_grad_(True)
    y = ops.mlp(x2, p["0.weight"], p["0.bias"], p["2.weight"], p["2.bias"])
    g = torch.autograd.grad(y, [x2] + [p[k] for k in names[1:5]], dy)
    assert all(torch.equal(a, b) for a, b in
               zip([y] + list(g[1:]) + [g[0]], want))


@DTYPES
def test_linear_gelu_through_autograd(dtype):
    torch.manual_seed(9)
    base = nn.Sequential(nn.Linear(64, 128), nn.GELU()).to(DEV, dtype)
    ref = nn.Sequential(nn.Linear(64, 128), nn.GELU()).double()
    ref.load_state_dict(base.state_dict())  # the stored (rounded) parameters
    ours = nn.Linear(64, 128).to(DEV, dtype)  # the same names, sorted alike
    ours.load_state_dict(base[0].state_dict())
    ours.forward = lambda t: ops.linear_gelu(t, ours.weight, ours.bias)
    x = torch.randn(3, 17, 64, device=DEV).to(dtype)
    dy = torch.randn(3, 17, 128, device=DEV).to(dtype)
    refs = _run_module(ref, x.double().cpu(), dy.double().cpu())
    assert not _held(["y", "db", "dw", "dx"], _run_module(ours, x, dy),
                     _run_module(base, x, dy), refs, EPS[dtype])


@pytest.mark.parametrize("switches", [
    dict(mlp="hip"), dict(mlp="hip", attention="hip", norm="hip")],
    ids=["mlp", "all-hip"])
def test_vit_tiny(switches):
    torch.manual_seed(5)
    base = vit_tiny().to(DEV)
    ours = vit_tiny(**switches).to(DEV)
    ours.load_state_dict(base.state_dict())
    ref = vit_tiny().double()  # on the CPU: the head's kernels have no fp64
    ref.load_state_dict(base.state_dict())
    x = torch.rand(4, 3, 64, 64, device=DEV)
    dy = torch.randn(4, 10, device=DEV)
    refs = _run_module(ref, x.double().cpu(), dy.double().cpu())
    names = ["out"] + sorted(n for n, _ in base.named_parameters())
    assert not _held(names, _run_module(ours, x, dy), _run_module(base, x, dy),
                     refs, EPS[torch.float32])
