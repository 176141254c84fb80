"""fp64 references and derived error bounds for the general kernel pack
(csrc/kernels.hip): the linear family, gemm_bf16, CE, MSE and the copies.

A plain module that the tests import; tests/test_kernel_oracle.py shows on
the CPU that torch's own fp32 and bf16 results meet every bound here, so a
bound is known to be satisfiable before a kernel is held to it.

Every reference is computed from the STORED operands (what the device
buffers hold, bf16 included) widened exactly to fp64, and every comparison
is elementwise `|got - ref| <= tol` with a per-element tol — no allclose.

Bounds (u32 = 2^-24 the fp32 unit roundoff, u16 = 2^-8 for bf16 storage):

matmul   tol = (n_terms + 4) * u32 * S        S = |A| @ |B| (+ |bias|)
         the classical dot-product bound, valid for ANY summation order
         (so for the MFMA k-loop, the split form's LDS reduction and
         rocBLAS alike; v_mfma_f32_16x16x4_f32 is an fmaf chain, no hidden
         term). +4: the three LDS adds of the split form and the bias add.
         bf16 storage adds the one output rounding: + u16 * |ref|.
         accumulate=True: ref = ref_new + old, old read back before the
         call; |old| joins S like a bias, the rounding term uses |ref|.
gemm_bf16  4 * (K + 4) * u32 * S + u16 * |ref|: the 32-wide bf16 MFMA's
         inner summation is unspecified; 4 is headroom, not a measurement.
CE       __expf/__logf have no derivable bound: the project's tolerances,
         now against fp64 — loss atol = rtol = 1e-5; grad (and probs, the
         same quantity) atol = 1e-5, rtol = 1e-4, + u16 * |ref| for a bf16
         gradient. tsum is a sum of C terms, ceil(C/64) per lane and a
         6-level wave tree: (ceil(C/64) + 6) * u32 * sum|t|.
MSE      loss: non-negative terms, so relative (2 + 6 + 4 + blocks) * u32
         (per-thread adds, wave tree, block adds, one atomic per block),
         blocks = min(cdiv(n, 256), 2048). grad: (y - t) * s with s formed
         as the kernel forms it, relative 3 * u32 (+ u16 for bf16).
copies   bitwise, compared as integer views so NaN patterns compare.

The matmul bound grows with the contraction length and cannot see ONE
dropped term in 2048, so every matmul shape is also run on integer-coded
operands (int_a/int_w/int_bias): small signed integers, exact in bf16,
every partial sum below 2^24, hence every fp32 summation order exact —
the result must EQUAL the fp64 one (for bf16: its single rounding).
"""

import math

import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8

F32, BF16 = torch.float32, torch.bfloat16


def widen(t):
    """The stored values of `t`, exactly, as a CPU fp64 tensor."""
    return t.detach().cpu().to(torch.float64)


def storage_u(dtype):
    """The output-rounding term's factor: 0 for fp32 (inside the dot-product
    bound already), u16 for bf16."""
    assert dtype in (F32, BF16)
    return U16 if dtype == BF16 else 0.0


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def worst_ratio(got, ref, tol):
    """max over elements of |got - ref| / tol (0/0 counts as 0, x/0 as inf);
    nan in `got` counts as inf."""
    got = widen(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(ratio.max())


def assert_within(got, ref, tol, what=""):
    """Elementwise |got - ref| <= tol. Returns the worst error/tol ratio."""
    r = worst_ratio(got, ref, tol)
    assert r <= 1.0, f"{what}: worst error/tol = {r:.3g}"
    return r


def assert_bitwise(got, want, what=""):
    """Equality of the bit patterns (NaN sentinels compare equal)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[got.element_size()]
    assert torch.equal(got.detach().cpu().contiguous().view(it),
                       want.detach().cpu().contiguous().view(it)), what


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def rand_signed(*shape, seed, dtype=F32):
    """Uniform in [-1, 1), rounded to the storage dtype."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(dtype)


def _coded(rows, cols, a, b, m, dtype):
    i = torch.arange(rows).view(-1, 1)
    j = torch.arange(cols).view(1, -1)
    return ((a * i + b * j) % m - m // 2).to(dtype)


def int_a(rows, cols, dtype=F32):
    """(7i + 3j) mod 11 - 5: the left operand (x, or dy for dX and dW)."""
    return _coded(rows, cols, 7, 3, 11, dtype)


def int_w(rows, cols, dtype=F32):
    """(5i + 2j) mod 13 - 6: the right operand (w, or x for dW)."""
    return _coded(rows, cols, 5, 2, 13, dtype)


def int_bias(n, dtype=F32):
    """Small signed integers, period 7, not symmetric about zero."""
    return ((3 * torch.arange(n)) % 7 - 2).to(dtype)


# ---------------------------------------------------------------------------
# matmul family
# ---------------------------------------------------------------------------
def matmul_ref(a, b, add=None):
    """(ref, S) of a @ b (+ add) in fp64: a [M,K], b [K,N] and add
    (broadcastable to [M,N]: a bias, or the old value under accumulate) are
    stored operands; S = |a| @ |b| (+ |add|)."""
    a, b = widen(a), widen(b)
    ref = a @ b
    S = a.abs() @ b.abs()
    if add is not None:
        add = widen(add)
        ref = ref + add
        S = S + add.abs()
    return ref, S


def matmul_tol(ref, S, n_terms, dtype, factor=1.0):
    return factor * (n_terms + 4) * U32 * S + storage_u(dtype) * ref.abs()


def gemm_bf16_tol(ref, S, K):
    return matmul_tol(ref, S, K, BF16, factor=4.0)


def assert_exact_int(got, ref, S, what=""):
    """The integer-coded check: every partial sum of every order is an
    integer below 2^24 (asserted on S, which bounds them all), so fp32
    arithmetic is exact and the stored result is ref's single rounding."""
    assert float(S.max()) < 2 ** 24 if S.numel() else True, \
        f"{what}: integer operands too large for exact fp32 sums"
    assert torch.equal(ref, ref.round()), f"{what}: reference is not integer"
    want = ref.to(torch.float32).to(got.dtype)  # < 2^24: fp32 step is exact
    assert_bitwise(got.detach().cpu() + 0, want + 0, what)  # +0: -0 == +0


def linear_fwd_ref(x, w, bias=None):
    """y = x @ w^T + bias; n_terms = K."""
    return matmul_ref(x, w.t(), None if bias is None else bias.view(1, -1))


def linear_bwd_input_ref(dy, w):
    """dx = dy @ w; n_terms = N."""
    return matmul_ref(dy, w)


def linear_bwd_weight_ref(x, dy, old_dw=None, old_db=None):
    """((dw_ref, dw_S), (db_ref, db_S)); n_terms = B for both. old_*: the
    tensors read back before an accumulate=True call."""
    dw = matmul_ref(dy.t(), x, old_dw)
    ones = torch.ones(dy.shape[0], 1, dtype=torch.float64)
    db_ref, db_S = matmul_ref(dy.t(), ones,
                              None if old_db is None else old_db.view(-1, 1))
    return dw, (db_ref.view(-1), db_S.view(-1))


# ---------------------------------------------------------------------------
# CE (probability targets) and MSE
# ---------------------------------------------------------------------------
CE_LOSS_ATOL = CE_LOSS_RTOL = 1e-5
CE_GRAD_ATOL, CE_GRAD_RTOL = 1e-5, 1e-4


def ce_ref(y, t, scale=1.0):
    """fp64 (loss, grad, probs, tsum) of mean-reduced CE on stored values;
    grad = (tsum * softmax(y) - t) * scale / B."""
    y, t = widen(y), widen(t)
    B = y.shape[0]
    lsm = torch.log_softmax(y, dim=1)
    loss = -(t * lsm).sum(1).mean()
    probs = torch.softmax(y, dim=1)
    tsum = t.sum(1)
    grad = (tsum.view(-1, 1) * probs - t) * (scale / B)
    return loss, grad, probs, tsum


def ce_loss_tol(ref):
    return CE_LOSS_ATOL + CE_LOSS_RTOL * ref.abs()


def ce_grad_tol(ref, dtype):
    return CE_GRAD_ATOL + (CE_GRAD_RTOL + storage_u(dtype)) * ref.abs()


def ce_probs_tol(ref):
    return ce_grad_tol(ref, F32)  # probs are fp32 whatever the storage


def ce_tsum_tol(t):
    t = widen(t)
    C = t.shape[1]
    return (math.ceil(C / 64) + 6) * U32 * t.abs().sum(1)


# every B in {1, 3, 4, 5} and C in {1, 2, 63, 64, 65, 129}: C straddles the
# 64-lane stride of k_ce_fwd
CE_SHAPES = [(1, 1), (3, 2), (4, 63), (5, 64), (1, 65), (3, 129), (4, 2),
             (5, 129)]
# the +1e4 shift is fp32 only: bf16 steps by 64 there
CE_LOGITS = [("pm30", F32), ("pm30", BF16), ("shift1e4", F32)]
CE_LOGITS_IDS = ["pm30-f32", "pm30-bf16", "shift1e4-f32"]


def ce_inputs(B, C, logits, targets, dtype, seed=0):
    """The CE cases: logits scaled to +-30, or small and shifted
    by +1e4; unnormalised (uniform in [0, 1)) or one-hot targets."""
    y = rand_signed(B, C, seed=seed + 1)
    y = y * 30 if logits == "pm30" else y * 3 + 1e4
    g = torch.Generator().manual_seed(seed + 2)
    if targets == "onehot":
        t = torch.nn.functional.one_hot(torch.randint(0, C, (B,), generator=g), C).float()
    else:
        t = torch.rand(B, C, generator=g)
    return y.to(dtype), t.to(dtype)


def mse_blocks(n):
    return min((n + 255) // 256, 2048)


def mse_loss_ref(y, t):
    y, t = widen(y), widen(t)
    return ((y - t) ** 2).mean()


def mse_loss_tol(ref, n):
    return (2 + 6 + 4 + mse_blocks(n)) * U32 * ref.abs()


def mse_scale(n, grad_scale=1.0, gout=None):
    """The kernel's fp32 factor: float(2 * grad_scale / n), times gout in
    fp32 when autograd's seed is folded in."""
    s = torch.tensor(2.0 * grad_scale / n, dtype=F32)
    if gout is not None:
        s = s * torch.tensor(gout, dtype=F32)
    return s


def mse_grad_ref(y, t, s):
    return (widen(y) - widen(t)) * widen(s)


def mse_grad_tol(ref, dtype):
    return (3 * U32 + storage_u(dtype)) * ref.abs()
