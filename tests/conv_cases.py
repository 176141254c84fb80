"""Shapes, operands, the fp64 reference and the bounds shared by
tests/test_conv.py (CPU) and tests/test_conv_gpu.py: a plain module.

Reference: F.conv2d and its autograd gradients in fp64 on the CPU from the
STORED operands (kernel_oracle.widen). Bounds: kernel_oracle's matmul bound,
elementwise, with S the same convolution or gradient of the operands'
absolute values and n_terms = k*k*Cin (y), k*k*Cout (dx), M + GS (dw: GS
slices of at most M terms in all, then GS - 1 adds)."""

import torch
import torch.nn.functional as F

import kernel_oracle as ko

# (N, H, W, Cin, Cout, k, stride)
SHAPES = [(1, 1, 1, 16, 16, 3, 1),     # one pixel: eight of nine taps padding
          (1, 5, 7, 16, 32, 3, 1),     # not square, M = 35 inside one tile
          (2, 12, 11, 16, 16, 3, 1),   # M = 264: tiles straddle rows, images
          (2, 9, 9, 48, 16, 3, 2),     # odd size at stride 2, 16-channel tail
          (1, 8, 8, 32, 144, 3, 2),    # even size at stride 2, two column tiles
          (3, 7, 7, 16, 16, 1, 1),     # 1x1
          (2, 7, 7, 32, 16, 1, 2),     # strided 1x1: the zero rows of dx
          (4, 20, 20, 16, 16, 3, 1)]   # M = 1600: seven slices, the last of 64
MULTI_SLICE = SHAPES[-1]
DTYPES = [ko.F32, ko.BF16]
REFUSED = {  # name -> (x shape, weight shape, stride, padding, weight dtype)
    "k=5": ((1, 16, 8, 8), (16, 16, 5, 5), 1, None, None),
    "k=3x1": ((1, 16, 8, 8), (16, 16, 3, 1), 1, None, None),
    "padding": ((1, 16, 8, 8), (16, 16, 3, 3), 1, 0, None),
    "stride 3": ((1, 16, 8, 8), (16, 16, 3, 3), 3, None, None),
    "Cin=24": ((1, 24, 8, 8), (16, 24, 3, 3), 1, None, None),
    "Cout=24": ((1, 16, 8, 8), (24, 16, 1, 1), 1, None, None),
    "groups": ((1, 32, 8, 8), (16, 16, 3, 3), 1, None, None),
    "mixed dtypes": ((1, 16, 8, 8), (16, 16, 3, 3), 1, None, ko.BF16),
    "3-D x": ((16, 8, 8), (16, 16, 3, 3), 1, None, None),
}


def out_size(h, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1


def operands(shape, dtype, kind):
    """(x [N,Cin,H,W], w [Cout,Cin,k,k], dy [N,Cout,Ho,Wo]) on the CPU in
    `dtype`; x and dy are channels-last views of their row matrices. kind:
    "random" (uniform in [-1, 1)) or "integer" (kernel_oracle's coded ones)."""
    N, H, W, Cin, Cout, k, s = shape
    Ho, Wo = out_size(H, k, s), out_size(W, k, s)
    if kind == "integer":
        xr = ko.int_a(N * H * W, Cin, dtype)
        w = ko.int_w(Cout, Cin * k * k, dtype)
        dyr = ko.int_a(N * Ho * Wo, Cout, dtype)
    else:
        seed = 100 * sum(shape)
        xr = ko.rand_signed(N * H * W, Cin, seed=seed, dtype=dtype)
        w = ko.rand_signed(Cout, Cin * k * k, seed=seed + 1, dtype=dtype)
        dyr = ko.rand_signed(N * Ho * Wo, Cout, seed=seed + 2, dtype=dtype)
    return (xr.view(N, H, W, Cin).permute(0, 3, 1, 2),
            w.view(Cout, Cin, k, k),
            dyr.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2))


def conv_all(x, w, dy, stride):
    """(y, dx, dw) of F.conv2d with padding k//2, in the operands' dtype."""
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad}


def reference(x, w, dy, stride):
    """({name: ref}, {name: S}) in fp64 from the stored operands."""
    x, w, dy = ko.widen(x), ko.widen(w), ko.widen(dy)
    return (conv_all(x, w, dy, stride),
            conv_all(x.abs(), w.abs(), dy.abs(), stride))


def n_terms(shape, GS):
    N, H, W, Cin, Cout, k, s = shape
    M = N * out_size(H, k, s) * out_size(W, k, s)
    return {"y": k * k * Cin, "dx": k * k * Cout, "dw": M + GS}


def check(got, shape, dtype, kind, ref, S, GS):
    """Hold y, dx and dw to the bound (random) or to equality (integer)."""
    for name, terms in n_terms(shape, GS).items():
        what = f"{name} {shape} {dtype} {kind}"
        if kind == "integer":
            ko.assert_exact_int(got[name], ref[name], S[name], what)
        else:
            tol = (ko.gemm_bf16_tol(ref[name], S[name], terms)
                   if dtype == ko.BF16
                   else ko.matmul_tol(ref[name], S[name], terms, dtype))
            print(what, "worst error/tol =",
                  ko.assert_within(got[name], ref[name], tol, what))
