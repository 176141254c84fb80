"""fp64 reference of ONE toy training step (csrc/toy_kernels.hip: Linear(K,1)
+ MSE + SGD) with a derived per-element bound for everything the step
stores. A plain module beside tests/kernel_oracle.py, whose units, widening
and comparisons it reuses; tests/test_toy_oracle.py shows on the CPU that a
torch fp32/bf16 emulation of the step meets every bound, and
tests/test_toy_step_oracle_gpu.py holds the five kernel families to it.

`toy_step_ref` works from the STORED operands (bf16 included) widened
exactly to fp64; lr enters as float(float32(lr)), the value the kernels
multiply by. The bound is propagated, not tuned. With u = U32:

  v   = U16 for bf16 storage, else 0 (the one rounding of a stored result)
  vdy = U16 only where dY is rounded to bf16 before the backward:
        k_toy_multistep_bf16w and nothing else
  c   = 4 only where the 32-wide bf16 MFMA sums in unspecified order (the
        same headroom as kernel_oracle.gemm_bf16_tol), else 1:
        v_mfma_f32_16x16x4_f32 and the chain kernel are plain fmaf chains

  A_i  = sum_k |x_ik||w_k| + |b|        e_y  = c (K+2) u A_i
  d    = y - t                           e_d  = e_y + u |d|
  dy   = d * 2/B                         e_dy = (2/B) e_d + (2u + vdy) |dy|
  dw_k = sum_i dy_i x_ik                 e_dw = sum_i e_dy_i |x_ik|
                                                + c (B+2) u sum_i |dy_i||x_ik|
  db   = the same with x = 1
  w'   = w - lr dw                       e_w  = lr e_dw + 2u (|w| + lr |dw|)
                                                + v |w'|
  loss = mean d^2                        e_l  = (2/B) sum |d| e_d
                                                + (B+8) u loss

A gradient written to a bf16 bucket (the lr = 0 path) gets e_dw + v |dw|
(`stored_grad_tol`). The loss word is f32 whatever the storage.

Measured with the CPU emulation of test_toy_oracle.py (nine shapes from
(1,1) to (128,20), uniform, signed and N(0,100^2) inputs, 20 seeds each):
worst error/tol 0.43 for f32 storage, 0.99 for bf16 (0.98 for the dY-in-bf16
step). The bf16 figure is the final bf16 rounding itself (half an ulp is a
relative 2^-8 just above a power of two), not slack another summation order
could use up. (An emulation that keeps the lr = 0 gradients in fp32 and has
no signed kind measures 0.37 and 0.89; this one also rounds those gradients
to bf16 storage, each a fresh half-ulp draw. The storage term is added to
the bound for exactly that rounding, so <= 1 holds by construction.) It is
also why a bound that admits bf16 storage cannot see a small gradient error
at a small lr, and why two sharper instruments stand beside it:

integer-coded cases (`int_case`)  small signed integers, B a power of two,
  lr = 2^-4: every intermediate of one step is exact in fp32 (and dY in
  bf16, |d| < 256), so the result must EQUAL the fp64 one, for bf16 storage
  its single rounding. `assert_step_exact` asserts the exactness condition
  on the reference itself. One dropped row or column is invisible to any
  bound and fails this.
zero-start cases (`inputs("zero", ...)`)  w = b = 0 and lr = 1, so
  w' = -dw rounded once: the bound is then 2^-8 of the gradient itself.
"""

import collections

import numpy as np
import torch

from kernel_oracle import (BF16, F32, U16, U32, assert_bitwise,  # noqa: F401
                           assert_within, widen, worst_ratio)

# (w', b', dw, db, loss): fp64 tensors, w/dw of K elements, the rest 0-dim
Step = collections.namedtuple("Step", "w b dw db loss")


def f32_lr(lr):
    """The learning rate the kernels multiply by: the host's double cast to
    float."""
    return float(np.float32(lr))


def toy_step_ref(x, t, w, b, lr, *, bf16_mfma=False, dy_bf16=False,
                 storage=F32):
    """(ref, tol) of one step, each a `Step`; the module docstring is the
    derivation. x [B,K], t [B] or [B,1], w [K], b one element: stored
    operands of any dtype."""
    assert storage in (F32, BF16)
    x = widen(x)
    B, K = x.shape
    t = widen(t).reshape(B)
    w = widen(w).reshape(K)
    b = widen(b).reshape(())
    lr = f32_lr(lr)
    u = U32
    v = U16 if storage == BF16 else 0.0
    vdy = U16 if dy_bf16 else 0.0
    c = 4.0 if bf16_mfma else 1.0
    ax = x.abs()

    A = ax @ w.abs() + b.abs()
    y = x @ w + b
    e_y = c * (K + 2) * u * A
    d = y - t
    e_d = e_y + u * d.abs()
    dy = d * (2.0 / B)
    e_dy = (2.0 / B) * e_d + (2 * u + vdy) * dy.abs()
    dw = dy @ x
    e_dw = e_dy @ ax + c * (B + 2) * u * (dy.abs() @ ax)
    db = dy.sum()
    e_db = e_dy.sum() + c * (B + 2) * u * dy.abs().sum()
    w1 = w - lr * dw
    e_w = lr * e_dw + 2 * u * (w.abs() + lr * dw.abs()) + v * w1.abs()
    b1 = b - lr * db
    e_b = lr * e_db + 2 * u * (b.abs() + lr * db.abs()) + v * b1.abs()
    loss = (d * d).mean()
    e_l = (2.0 / B) * (d.abs() * e_d).sum() + (B + 8) * u * loss
    return Step(w1, b1, dw, db, loss), Step(e_w, e_b, e_dw, e_db, e_l)


def stored_grad_tol(ref, tol, storage):
    """(e_dw, e_db) of gradients written to a bucket of dtype `storage`."""
    v = U16 if storage == BF16 else 0.0
    return tol.dw + v * ref.dw.abs(), tol.db + v * ref.db.abs()


# ---------------------------------------------------------------------------
# integer-coded exact cases
# ---------------------------------------------------------------------------
INT_LR = 2.0 ** -4


def int_case(B, K, dtype=F32):
    """(x, t, w, b, lr): x = (7i+3j) mod 5 - 2, w = (5j) mod 7 - 3,
    t = (3i) mod 7 - 3, b = 2, lr = 2^-4. B must be a power of two, so that
    2/B and /B are exact."""
    assert B >= 1 and B & (B - 1) == 0, "integer-coded cases need B = 2^n"
    i = torch.arange(B).view(-1, 1)
    j = torch.arange(K).view(1, -1)
    x = ((7 * i + 3 * j) % 5 - 2).to(dtype)
    w = ((5 * j) % 7 - 3).view(-1).to(dtype)
    t = ((3 * i) % 7 - 3).to(dtype)
    b = torch.tensor([2.0]).to(dtype)
    return x, t, w, b, INT_LR


def _survives(v, dtype=F32):
    return torch.equal(v.to(dtype).to(torch.float64), v)


def assert_step_exact(x, t, w, b, lr, *, dy_bf16=False, what=""):
    """The exactness condition of an integer-coded step, asserted on the
    fp64 reference: every intermediate survives a round trip through fp32
    (dY through bf16 where the kernel rounds it so), and every partial sum
    of every summation order is a multiple of a power of two below 2^24 of
    them, so fp32 arithmetic in any order is exact. Returns the reference
    `Step`."""
    ref, _ = toy_step_ref(x, t, w, b, lr)
    x = widen(x)
    B, K = x.shape
    t, w, bb = widen(t).reshape(B), widen(w).reshape(K), widen(b).reshape(())
    lr = f32_lr(lr)
    assert B & (B - 1) == 0, what
    y = x @ w + bb
    d = y - t
    dy = d * (2.0 / B)
    # integer operands: all forward partial sums are integers below 2^24
    for name, val in (("x", x), ("w", w), ("t", t), ("b", bb)):
        assert torch.equal(val, val.round()), f"{what}: {name} not integer"
    assert float((x.abs() @ w.abs() + bb.abs() + t.abs()).max()) < 2 ** 24
    # backward partial sums: integers times 2/B
    assert float((dy.abs() @ x.abs()).max()) * (B / 2) < 2 ** 24, what
    assert float(dy.abs().sum()) * (B / 2) < 2 ** 24, what
    # loss partial sums: integers
    assert float((d * d).sum()) < 2 ** 24, what
    assert float(d.abs().max()) < 256, f"{what}: |d| must stay below 256"
    assert _survives(dy, BF16 if dy_bf16 else F32), f"{what}: dY inexact"
    for name, val in (("y", y), ("d", d), ("d^2", d * d), ("dw", ref.dw),
                      ("db", ref.db), ("lr*dw", lr * ref.dw),
                      ("lr*db", lr * ref.db), ("w'", ref.w), ("b'", ref.b),
                      ("loss", ref.loss)):
        assert _survives(val), f"{what}: {name} is not exact in fp32"
    return ref


def exact_stored(ref64, dtype):
    """The value an exact fp32 computation stores: fp64 -> fp32 is exact
    here (asserted by assert_step_exact), then the single rounding of the
    storage dtype."""
    return ref64.to(torch.float32).to(dtype)


def assert_equal_exact(got, ref64, what=""):
    """`got` equals the exact result's stored value (+0 == -0)."""
    want = exact_stored(ref64, got.dtype).reshape(got.shape)
    assert_bitwise(got.detach().cpu() + 0, want + 0, what)


# ---------------------------------------------------------------------------
# operands of the bound-checked cases
# ---------------------------------------------------------------------------
KINDS = ["uniform", "signed", "normal100", "zero"]


def inputs(kind, rows, K, dtype=F32, seed=0):
    """(x [rows,K], t [rows,1], w [K], b [1], lr), rounded to the storage
    dtype.
      uniform    x, t in [0,1), w in [-.5,.5), b in [0,1), lr 0.05: what the
                 benchmark draws
      signed     everything in [-1,1), lr 0.05
      normal100  x, t ~ N(0, 100^2), w, b in [-1,1), lr 1e-5: cancellation
                 and large magnitudes
      zero       signed x, t; w = b = 0, lr 1: w' = -dw rounded once
    """
    g = torch.Generator().manual_seed(1000003 * seed + 131 * rows + K)
    if kind == "uniform":
        x = torch.rand(rows, K, generator=g)
        t = torch.rand(rows, 1, generator=g)
        w = torch.rand(K, generator=g) - 0.5
        b = torch.rand(1, generator=g)
        lr = 0.05
    elif kind == "normal100":
        x = torch.randn(rows, K, generator=g) * 100.0
        t = torch.randn(rows, 1, generator=g) * 100.0
        w = torch.rand(K, generator=g) * 2 - 1
        b = torch.rand(1, generator=g) * 2 - 1
        lr = 1e-5
    else:
        assert kind in ("signed", "zero"), kind
        x = torch.rand(rows, K, generator=g) * 2 - 1
        t = torch.rand(rows, 1, generator=g) * 2 - 1
        w = torch.rand(K, generator=g) * 2 - 1
        b = torch.rand(1, generator=g) * 2 - 1
        lr = 0.05
        if kind == "zero":
            w, b, lr = torch.zeros(K), torch.zeros(1), 1.0
    return x.to(dtype), t.to(dtype), w.to(dtype), b.to(dtype), lr


# ---------------------------------------------------------------------------
# CPU emulation of the kernels' step: torch fp32 arithmetic on the stored
# operands, the kernels' roundings at the kernels' places. Its summation
# order is torch's, not the kernels'; the bound is order-independent.
# ---------------------------------------------------------------------------
def emulate_step(x, t, w, b, lr, *, dy_bf16=False, storage=F32, mutate=None):
    """Returns (w', b', dw, db, loss): params and gradients in `storage`,
    the loss f32. mutate: None, or a named wrong step for the detection
    tests ("grad_1pct", "drop_row", "drop_col", "no_bias", "half_scale")."""
    B, K = x.shape
    xf = x.float()
    tf = t.float().reshape(B)
    wf = w.float().reshape(K)
    bf = b.float().reshape(())
    lrf = torch.tensor(lr, dtype=F32)
    xfwd = xf
    if mutate == "drop_col":
        xfwd = xf.clone()
        xfwd[:, K - 1] = 0
    y = xfwd @ wf + (0 if mutate == "no_bias" else bf)
    d = y - tf
    scale = torch.tensor((1.0 if mutate == "half_scale" else 2.0) / B,
                         dtype=F32)
    dy = d * scale
    if dy_bf16:
        dy = dy.to(BF16).float()
    dyb = dy
    if mutate == "drop_row":
        dyb = dy.clone()
        dyb[B - 1] = 0
    dw = dyb @ xf
    db = dyb.sum()
    if mutate == "grad_1pct":
        dw, db = dw * 1.01, db * 1.01
    w1 = (wf - lrf * dw).to(storage)
    b1 = (bf - lrf * db).to(storage)
    loss = (d * d).sum() / B
    return Step(w1, b1.reshape(()), dw.to(storage), db.to(storage).reshape(()),
                loss)


def step_ratios(got, ref, tol, storage):
    """Worst error/tol of each stored quantity of `got` (a Step)."""
    e_gw, e_gb = stored_grad_tol(ref, tol, storage)
    return Step(worst_ratio(got.w, ref.w, tol.w),
                worst_ratio(got.b, ref.b, tol.b),
                worst_ratio(got.dw, ref.dw, e_gw),
                worst_ratio(got.db, ref.db, e_gb),
                worst_ratio(got.loss, ref.loss, tol.loss))


def fmt_ratios(r):
    return " ".join(f"{n}={v:.3g}" for n, v in zip(Step._fields, r))

