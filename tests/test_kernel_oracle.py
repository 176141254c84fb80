"""CPU check of tests/kernel_oracle.py: torch's own fp32 and bf16 CPU results
meet every bound the GPU edge tests (test_kernel_pack_edges_gpu.py) hold the
kernels to, at the same kinds of shapes, and the integer-coded operands are
exact — so each bound is known to be satisfiable before it reaches a GPU.
A wrong result must also FAIL the bound: one dropped term, a transposed
operand and an ignored scale are checked to be seen."""

import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko
from kernel_oracle import BF16, F32

DTYPES = [F32, BF16]
IDS = ["f32", "bf16"]

# M x K x N: the issue's table plus the two routing-threshold shapes
MATMUL_SHAPES = [(17, 2048, 500), (65, 17, 33), (63, 257, 17), (1, 1, 1),
                 (17, 1024, 1023), (17, 1024, 1024)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,K,N", MATMUL_SHAPES)
def test_matmul_bound_holds_for_torch_cpu(M, K, N, dtype):
    x = ko.rand_signed(M, K, seed=1, dtype=dtype)
    w = ko.rand_signed(N, K, seed=2, dtype=dtype)
    b = ko.rand_signed(N, seed=3, dtype=dtype)
    ref, S = ko.linear_fwd_ref(x, w, b)
    r = ko.assert_within(F.linear(x, w, b), ref,
                         ko.matmul_tol(ref, S, K, dtype), "fwd")
    print(f"fwd {M}x{K}x{N} {dtype}: error/tol {r:.3g}")
    # dX of the same layer: contraction over N
    dy = ko.rand_signed(M, N, seed=4, dtype=dtype)
    ref, S = ko.linear_bwd_input_ref(dy, w)
    ko.assert_within(dy @ w, ref, ko.matmul_tol(ref, S, N, dtype), "dX")
    # the looser gemm_bf16 bound contains the plain one
    if dtype == BF16:
        ref, S = ko.linear_fwd_ref(x, w, b)
        assert (ko.gemm_bf16_tol(ref, S, K)
                >= ko.matmul_tol(ref, S, K, BF16)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,K,N", [(33, 129, 33), (5, 17, 33), (1, 1, 1),
                                   (17, 1024, 1023)])
def test_bwd_weight_bound_holds_for_torch_cpu(B, K, N, dtype):
    x = ko.rand_signed(B, K, seed=5, dtype=dtype)
    dy = ko.rand_signed(B, N, seed=6, dtype=dtype)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(x, dy)
    dw = (dy.float().t() @ x.float()).to(dtype)
    db = dy.float().sum(0).to(dtype)
    ko.assert_within(dw, dw_ref, ko.matmul_tol(dw_ref, dw_S, B, dtype), "dw")
    ko.assert_within(db, db_ref, ko.matmul_tol(db_ref, db_S, B, dtype), "db")
    # accumulate: fp32 add onto the stored old value, one rounding
    old_w = ko.rand_signed(N, K, seed=7, dtype=dtype)
    old_b = ko.rand_signed(N, seed=8, dtype=dtype)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(
        x, dy, old_w, old_b)
    dw = (dy.float().t() @ x.float() + old_w.float()).to(dtype)
    db = (dy.float().sum(0) + old_b.float()).to(dtype)
    ko.assert_within(dw, dw_ref, ko.matmul_tol(dw_ref, dw_S, B, dtype),
                     "dw accumulate")
    ko.assert_within(db, db_ref, ko.matmul_tol(db_ref, db_S, B, dtype),
                     "db accumulate")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,K,N", MATMUL_SHAPES)
def test_integer_operands_are_exact(M, K, N, dtype):
    x, w, b = ko.int_a(M, K, dtype), ko.int_w(N, K, dtype), \
        ko.int_bias(N, dtype)
    # exact in the storage dtype
    assert torch.equal(x.double(), ko.int_a(M, K, torch.float64))
    assert torch.equal(w.double(), ko.int_w(N, K, torch.float64))
    ref, S = ko.linear_fwd_ref(x, w, b)
    got = F.linear(x.float(), w.float(), b.float()).to(dtype)
    ko.assert_exact_int(got, ref, S, "fwd")
    dy = ko.int_a(M, N, dtype)
    ref, S = ko.linear_bwd_input_ref(dy, w)
    ko.assert_exact_int((dy.float() @ w.float()).to(dtype), ref, S, "dX")
    xw = ko.int_w(M, K, dtype)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(xw, dy)
    ko.assert_exact_int((dy.float().t() @ xw.float()).to(dtype), dw_ref,
                        dw_S, "dw")
    ko.assert_exact_int(dy.float().sum(0).to(dtype), db_ref, db_S, "db")


def test_integer_operands_are_asymmetric_and_signed():
    a, w = ko.int_a(12, 14), ko.int_w(12, 14)
    assert a.min() == -5 and a.max() == 5 and w.min() == -6 and w.max() == 6
    assert not torch.equal(a[:12, :12], a[:12, :12].t())
    assert not torch.equal(w[:12, :12], w[:12, :12].t())
    assert len(set(ko.int_bias(7).tolist())) == 7


def test_integer_check_sees_one_dropped_term_in_2048():
    M, K, N = 17, 2048, 500
    x, w, b = ko.int_a(M, K), ko.int_w(N, K), ko.int_bias(N)
    ref, S = ko.linear_fwd_ref(x, w, b)
    got = F.linear(x[:, :-1], w[:, :-1], b)  # the last k never contracted
    with pytest.raises(AssertionError):
        ko.assert_exact_int(got, ref, S)
    # and the random-operand bound sees a transposed operand or a lost bias
    x, w, b = (ko.rand_signed(33, 33, seed=1), ko.rand_signed(33, 33, seed=2),
               ko.rand_signed(33, seed=3))
    ref, S = ko.linear_fwd_ref(x, w, b)
    tol = ko.matmul_tol(ref, S, 33, F32)
    assert ko.worst_ratio(F.linear(x, w.t().contiguous(), b), ref, tol) > 1
    assert ko.worst_ratio(F.linear(x, w), ref, tol) > 1


def test_integer_oracle_rejects_sums_past_2_24():
    x = torch.full((1, 4), 4096.0)
    ref, S = ko.linear_fwd_ref(x, x)
    with pytest.raises(AssertionError, match="too large"):
        ko.assert_exact_int((x @ x.t()), ref, S, "big")


def test_nan_never_passes():
    ref = torch.zeros(3, dtype=torch.float64)
    assert ko.worst_ratio(torch.tensor([0.0, float("nan"), 0.0]), ref,
                          1.0) == float("inf")
    assert ko.worst_ratio(torch.zeros(3), ref, 0.0) == 0.0


# ---------------------------------------------------------------------------
# CE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("targets", ["unnorm", "onehot"])
@pytest.mark.parametrize("logits,dtype", ko.CE_LOGITS, ids=ko.CE_LOGITS_IDS)
@pytest.mark.parametrize("B,C", ko.CE_SHAPES)
def test_ce_bounds_hold_for_torch_cpu(B, C, logits, dtype, targets):
    y, t = ko.ce_inputs(B, C, logits, targets, dtype)
    loss_ref, grad_ref, probs_ref, tsum_ref = ko.ce_ref(y, t, 2.5)
    yf = y.float().requires_grad_(True)  # torch's loss policy: fp32
    loss = F.cross_entropy(yf, t.float())
    (2.5 * loss).backward()
    ko.assert_within(loss, loss_ref, ko.ce_loss_tol(loss_ref), "loss")
    ko.assert_within(yf.grad.to(dtype), grad_ref,
                     ko.ce_grad_tol(grad_ref, dtype), "grad")
    ko.assert_within(torch.softmax(y.float(), 1), probs_ref,
                     ko.ce_probs_tol(probs_ref), "probs")
    ko.assert_within(t.float().sum(1), tsum_ref, ko.ce_tsum_tol(t), "tsum")
    # a gradient that ignored the 2.5 seed is outside the bound
    if grad_ref.abs().max() > 1e-3:
        assert ko.worst_ratio(yf.grad / 2.5, grad_ref,
                              ko.ce_grad_tol(grad_ref, dtype)) > 1


def test_ce_loss_without_max_subtraction_misses_the_bound():
    """Why the shifted case is there: ts * (m + log se) - sum t*y in fp32,
    the form that leaves the row max inside both terms, is off by the fp32
    spacing at 1e4 (1e-3) and fails the loss tolerance."""
    y, t = ko.ce_inputs(3, 129, "shift1e4", "unnorm", F32)
    loss_ref = ko.ce_ref(y, t)[0]
    m = y.max(1).values
    se = torch.exp(y - m.view(-1, 1)).sum(1)
    naive = (t.sum(1) * (m + torch.log(se)) - (t * y).sum(1)).mean()
    assert ko.worst_ratio(naive, loss_ref, ko.ce_loss_tol(loss_ref)) > 1
    stable = (t.sum(1) * torch.log(se) - (t * (y - m.view(-1, 1))).sum(1)
              ).mean()
    ko.assert_within(stable, loss_ref, ko.ce_loss_tol(loss_ref), "stable")


# ---------------------------------------------------------------------------
# MSE
# ---------------------------------------------------------------------------
MSE_SIZES = [1, 255, 256, 257, 2048 * 256 + 257]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_bounds_hold_for_torch_cpu(n, dtype):
    y = ko.rand_signed(n, seed=11, dtype=dtype)
    t = ko.rand_signed(n, seed=12, dtype=dtype)
    loss_ref = ko.mse_loss_ref(y, t)
    loss = F.mse_loss(y.float(), t.float())
    ko.assert_within(loss, loss_ref, ko.mse_loss_tol(loss_ref, n), "loss")
    for grad_scale, gout in ((1.0, 2.5), (0.5, None)):
        s = ko.mse_scale(n, grad_scale, gout)
        ref = ko.mse_grad_ref(y, t, s)
        got = ((y.float() - t.float()) * s).to(dtype)
        ko.assert_within(got, ref, ko.mse_grad_tol(ref, dtype), "grad")
        if n > 1:  # an ignored scale is outside the bound
            wrong = ((y.float() - t.float()) * ko.mse_scale(n)).to(dtype)
            assert ko.worst_ratio(wrong, ref,
                                  ko.mse_grad_tol(ref, dtype)) > 1
    assert ko.mse_blocks(n) == min(-(-n // 256), 2048)


def test_bitwise_compare_sees_nan_payloads():
    a = torch.tensor([0x7FC12345, 0x7FC12345], dtype=torch.int32).view(F32)
    b = a.clone()
    ko.assert_bitwise(a, b)
    b.view(torch.int32)[1] = 0x7FC12346
    with pytest.raises(AssertionError):
        ko.assert_bitwise(a, b)
