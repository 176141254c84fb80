"""The general kernel pack (csrc/kernels.hip, autograd_ops.hip) at its edges,
held to the fp64 references and derived bounds of tests/kernel_oracle.py:
ragged tiles, both forms of k_linear_tile up to the rocBLAS routing
threshold, k_linear_bwd_w across K-blocks and in both modes, gemm_bf16, CE
around the 64-lane stride with wide and shifted logits, the gout/grad_scale
folds, the MSE grid-stride loop, multi-row bucket copies with byte tails,
the epoch shard's cycle walk, and the host-side guards of every launcher.

Every matmul case runs twice: random signed operands against the
dot-product bound, and integer-coded operands that must come out EXACT (one
dropped or doubled k-slice, a wrong slice boundary or a transposed fragment
cannot hide inside a bound that grows with K)."""

import functools

import pytest
import torch

import kernel_oracle as ko
from kernel_oracle import BF16, F32
from mi355x_ddp import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [F32, BF16]
IDS = ["f32", "bf16"]
KINDS = ["rand", "int"]


def _ext():
    return ops.ext()


def _left(kind, rows, cols, dtype, seed):
    return (ko.int_a(rows, cols, dtype) if kind == "int"
            else ko.rand_signed(rows, cols, seed=seed, dtype=dtype))


def _right(kind, rows, cols, dtype, seed):
    return (ko.int_w(rows, cols, dtype) if kind == "int"
            else ko.rand_signed(rows, cols, seed=seed, dtype=dtype))


def _bias(kind, n, dtype, seed):
    return (ko.int_bias(n, dtype) if kind == "int"
            else ko.rand_signed(n, seed=seed, dtype=dtype))


def _check_matmul(kind, got, ref, S, n_terms, dtype, what, factor=1.0):
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), what
    if kind == "int":
        ko.assert_exact_int(got, ref, S, what)
    else:
        ko.assert_within(got, ref,
                         ko.matmul_tol(ref, S, n_terms, dtype, factor), what)


# ---------------------------------------------------------------------------
# k_linear_tile: (M, contraction, output columns). Serial form from M = 64,
# split form below; every listed value appears in each form.
# ---------------------------------------------------------------------------
SERIAL = [(64, 1, 1), (65, 3, 15), (80, 4, 16), (81, 5, 17), (64, 16, 33),
          (65, 17, 1), (80, 17, 33), (81, 16, 15)]
# contraction 13: every wave one iteration, the last ragged; 17: wave 2 one
# element, wave 3 an empty slice; (17, 2048, 500) is the ResNet-FC-like
# forward just under the routing threshold and (17, 500, 2048) its dX
SPLIT = [(1, 1, 1), (15, 3, 15), (16, 4, 16), (17, 5, 17), (63, 13, 33),
         (1, 17, 33), (15, 64, 17), (16, 67, 1), (17, 257, 15),
         (63, 257, 16), (17, 2048, 500), (17, 500, 2048)]
TILE_CASES = ([pytest.param(*c, id="serial-%dx%dx%d" % c) for c in SERIAL]
              + [pytest.param(*c, id="split-%dx%dx%d" % c) for c in SPLIT])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,Kc,Nc", TILE_CASES)
def test_linear_fwd_edges(M, Kc, Nc, dtype, kind):
    x = _left(kind, M, Kc, dtype, 1)
    w = _right(kind, Nc, Kc, dtype, 2)
    b = _bias(kind, Nc, dtype, 3)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref, S = ko.linear_fwd_ref(x, w, b)
    _check_matmul(kind, _ext().linear_fwd(xd, wd, bd), ref, S, Kc, dtype,
                  "fwd+bias")
    ref, S = ko.linear_fwd_ref(x, w)
    _check_matmul(kind, _ext().linear_fwd(xd, wd, None), ref, S, Kc, dtype,
                  "fwd bias=None")
    _check_matmul(kind, _ext().linear_fwd(xd, wd), ref, S, Kc, dtype,
                  "fwd no bias argument")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,Kc,Nc", TILE_CASES)
def test_linear_bwd_input_edges(M, Kc, Nc, dtype, kind):
    dy = _left(kind, M, Kc, dtype, 4)
    w = _right(kind, Kc, Nc, dtype, 5)
    ref, S = ko.linear_bwd_input_ref(dy, w)
    _check_matmul(kind, _ext().linear_bwd_input(dy.to(DEV), w.to(DEV)), ref,
                  S, Kc, dtype, "dX")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M", [17, 65], ids=["split", "serial"])
def test_linear_entry_points_noncontiguous(M, dtype, kind):
    K, N = 21, 19
    xT = _left(kind, K, M, dtype, 6).to(DEV)      # x = xT.t(): [M, K]
    wT = _right(kind, K, N, dtype, 7).to(DEV)     # w = wT.t(): [N, K]
    b = _bias(kind, N, dtype, 8).to(DEV)
    x, w = xT.t(), wT.t()
    assert not x.is_contiguous() and not w.is_contiguous()
    ref, S = ko.linear_fwd_ref(x, w, b)
    _check_matmul(kind, _ext().linear_fwd(x, w, b), ref, S, K, dtype, "fwd")
    dyT = _left(kind, N, M, dtype, 9).to(DEV)     # dy = dyT.t(): [M, N]
    dy = dyT.t()
    ref, S = ko.linear_bwd_input_ref(dy, w)
    _check_matmul(kind, _ext().linear_bwd_input(dy, w), ref, S, N, dtype,
                  "dX")
    dw = torch.full((N, K), float("nan"), dtype=dtype, device=DEV)
    db = torch.full((N,), float("nan"), dtype=dtype, device=DEV)
    _ext().linear_bwd_weight(x, dy, dw, db, False)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(x, dy)
    _check_matmul(kind, dw, dw_ref, dw_S, M, dtype, "dw")
    _check_matmul(kind, db, db_ref, db_S, M, dtype, "db")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,N,library", [(1024, 1023, False),
                                         (1024, 1024, True)],
                         ids=["hand-1024x1023", "rocblas-1024x1024"])
def test_linear_autograd_routing_threshold(K, N, library, kind):
    """ops.linear end to end on either side of K*N >= 2^20: y, dx, dw, db.
    The bound is order-independent, so it holds for rocBLAS too."""
    assert ops._library_gemm_shape(K, N) is library
    assert ops._library_gemm_shape(2048, 500) is False  # the long split case
    B = 17
    x = _left(kind, B, K, F32, 10).to(DEV).requires_grad_(True)
    w = _right(kind, N, K, F32, 11).to(DEV).requires_grad_(True)
    b = _bias(kind, N, F32, 12).to(DEV).requires_grad_(True)
    g = _right(kind, B, N, F32, 13).to(DEV)
    y = ops.linear(x, w, b)
    (y * g).sum().backward()
    ref, S = ko.linear_fwd_ref(x, w, b)
    _check_matmul(kind, y.detach(), ref, S, K, F32, "y")
    ref, S = ko.linear_bwd_input_ref(g, w)
    _check_matmul(kind, x.grad, ref, S, N, F32, "dx")
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(x, g)
    _check_matmul(kind, w.grad, dw_ref, dw_S, B, F32, "dw")
    _check_matmul(kind, b.grad, db_ref, db_S, B, F32, "db")


# ---------------------------------------------------------------------------
# k_linear_bwd_w: (B, K, N); K > 64 reaches blockIdx.x >= 1
# ---------------------------------------------------------------------------
BWD_W = [(1, 1, 1), (3, 15, 16), (4, 16, 17), (5, 17, 33), (33, 63, 1),
         (1, 64, 16), (3, 65, 17), (4, 100, 33), (5, 129, 17), (33, 129, 33)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,K,N", BWD_W)
def test_linear_bwd_weight_edges(B, K, N, dtype, kind):
    x = _right(kind, B, K, dtype, 14)
    dy = _left(kind, B, N, dtype, 15)
    xd, dyd = x.to(DEV), dy.to(DEV)
    # overwrite: nothing of a NaN-prefilled dw/db may survive
    dw = torch.full((N, K), float("nan"), dtype=dtype, device=DEV)
    db = torch.full((N,), float("nan"), dtype=dtype, device=DEV)
    _ext().linear_bwd_weight(xd, dyd, dw, db, False)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(x, dy)
    _check_matmul(kind, dw, dw_ref, dw_S, B, dtype, "dw overwrite")
    _check_matmul(kind, db, db_ref, db_S, B, dtype, "db overwrite")
    # accumulate onto a non-zero dw/db, read back BEFORE the call
    dw = _right(kind, N, K, dtype, 16).to(DEV)
    db = _bias(kind, N, dtype, 17).to(DEV)
    old_w, old_b = dw.cpu().clone(), db.cpu().clone()
    assert old_w.abs().sum() > 0
    _ext().linear_bwd_weight(xd, dyd, dw, db, True)
    (dw_ref, dw_S), (db_ref, db_S) = ko.linear_bwd_weight_ref(
        x, dy, old_w, old_b)
    _check_matmul(kind, dw, dw_ref, dw_S, B, dtype, "dw accumulate")
    _check_matmul(kind, db, db_ref, db_S, B, dtype, "db accumulate")
    # an empty db: the kernel's nullptr branch, dw still right
    dw = torch.full((N, K), float("nan"), dtype=dtype, device=DEV)
    _ext().linear_bwd_weight(xd, dyd, dw,
                             torch.empty(0, dtype=dtype, device=DEV), False)
    (dw_ref, dw_S), _ = ko.linear_bwd_weight_ref(x, dy)
    _check_matmul(kind, dw, dw_ref, dw_S, B, dtype, "dw with empty db")


# ---------------------------------------------------------------------------
# gemm_bf16 (32-wide bf16 MFMA)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K,N", [(32, 32, 16), (64, 100, 48), (16, 20, 1),
                                   (128, 256, 256), (1, 1, 1), (17, 33, 17),
                                   (65, 31, 15)])
def test_gemm_bf16_edges(B, K, N, kind):
    x = _left(kind, B, K, BF16, 18)
    w = _right(kind, N, K, BF16, 19)
    b = _bias(kind, N, BF16, 20)
    xd, wd = x.to(DEV), w.to(DEV)
    ref, S = ko.linear_fwd_ref(x, w, b)
    _check_matmul(kind, _ext().gemm_bf16(xd, wd, b.to(DEV)), ref, S, K, BF16,
                  "gemm_bf16+bias", factor=4.0)
    ref, S = ko.linear_fwd_ref(x, w)
    _check_matmul(kind, _ext().gemm_bf16(xd, wd), ref, S, K, BF16,
                  "gemm_bf16", factor=4.0)


# ---------------------------------------------------------------------------
# CE
# ---------------------------------------------------------------------------
CE_PARAMS = [pytest.mark.parametrize("targets", ["unnorm", "onehot"]),
             pytest.mark.parametrize("logits,dtype", ko.CE_LOGITS,
                                     ids=ko.CE_LOGITS_IDS),
             pytest.mark.parametrize("B,C", ko.CE_SHAPES)]


def _ce_params(f):
    for p in CE_PARAMS:
        f = p(f)
    return f


@_ce_params
def test_ce_autograd_edges(B, C, logits, dtype, targets):
    """ops.cross_entropy with (2.5 * loss).backward(): the seed reaches
    k_ce_bwd through gout, so a kernel ignoring it is off by 2.5x."""
    y, t = ko.ce_inputs(B, C, logits, targets, dtype)
    loss_ref, grad_ref, _, _ = ko.ce_ref(y, t, 2.5)
    yd = y.to(DEV).requires_grad_(True)
    loss = ops.cross_entropy(yd, t.to(DEV))
    (2.5 * loss).backward()
    assert loss.dtype == F32 and yd.grad.dtype == dtype
    ko.assert_within(loss, loss_ref, ko.ce_loss_tol(loss_ref), "loss")
    ko.assert_within(yd.grad, grad_ref, ko.ce_grad_tol(grad_ref, dtype),
                     "grad")


@_ce_params
def test_ce_direct_edges(B, C, logits, dtype, targets):
    """ce_fwd's loss, probs and tsum, then ce_bwd with grad_scale = 0.5 and
    no gout, and with both."""
    y, t = ko.ce_inputs(B, C, logits, targets, dtype)
    loss_ref, grad_ref, probs_ref, tsum_ref = ko.ce_ref(y, t, 0.5)
    td = t.to(DEV)
    loss, probs, tsum = _ext().ce_fwd(y.to(DEV), td)
    assert loss.dtype == probs.dtype == tsum.dtype == F32
    ko.assert_within(loss, loss_ref, ko.ce_loss_tol(loss_ref), "loss")
    ko.assert_within(probs, probs_ref, ko.ce_probs_tol(probs_ref), "probs")
    ko.assert_within(tsum, tsum_ref, ko.ce_tsum_tol(t), "tsum")
    dy = _ext().ce_bwd(probs, td, tsum, 0.5)
    assert dy.dtype == dtype
    ko.assert_within(dy, grad_ref, ko.ce_grad_tol(grad_ref, dtype),
                     "grad, grad_scale=0.5")
    gout = torch.tensor(-3.0, device=DEV)
    dy = _ext().ce_bwd(probs, td, tsum, 0.5, gout)
    ko.assert_within(dy, -3.0 * grad_ref,
                     ko.ce_grad_tol(-3.0 * grad_ref, dtype),
                     "grad, grad_scale=0.5, gout=-3")


# ---------------------------------------------------------------------------
# MSE: 2048*256 + 257 enters k_mse_fwd's grid-stride loop with a ragged
# second pass
# ---------------------------------------------------------------------------
MSE_SIZES = [1, 255, 256, 257, 2048 * 256 + 257]


@functools.lru_cache(maxsize=None)
def _mse_case(n, dtype):
    y = ko.rand_signed(n, seed=21, dtype=dtype)
    t = ko.rand_signed(n, seed=22, dtype=dtype)
    return y, t, ko.mse_loss_ref(y, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_autograd_edges(n, dtype):
    y, t, loss_ref = _mse_case(n, dtype)
    yd = y.to(DEV).requires_grad_(True)
    loss = ops.mse_loss(yd, t.to(DEV))
    (2.5 * loss).backward()
    assert loss.dtype == F32 and yd.grad.dtype == dtype
    ko.assert_within(loss, loss_ref, ko.mse_loss_tol(loss_ref, n), "loss")
    ref = ko.mse_grad_ref(y, t, ko.mse_scale(n, 1.0, 2.5))
    ko.assert_within(yd.grad, ref, ko.mse_grad_tol(ref, dtype), "grad")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_direct_edges(n, dtype):
    y, t, loss_ref = _mse_case(n, dtype)
    yd, td = y.to(DEV), t.to(DEV)
    loss = _ext().mse_fwd(yd, td)
    ko.assert_within(loss, loss_ref, ko.mse_loss_tol(loss_ref, n), "loss")
    dy = _ext().mse_bwd(yd, td, 0.5)
    ref = ko.mse_grad_ref(y, t, ko.mse_scale(n, 0.5))
    ko.assert_within(dy, ref, ko.mse_grad_tol(ref, dtype),
                     "grad, grad_scale=0.5")
    dy = _ext().mse_bwd(yd, td, 0.5, torch.tensor(-3.0, device=DEV))
    ref = ko.mse_grad_ref(y, t, ko.mse_scale(n, 0.5, -3.0))
    ko.assert_within(dy, ref, ko.mse_grad_tol(ref, dtype),
                     "grad, grad_scale=0.5, gout=-3")


# ---------------------------------------------------------------------------
# Bucket copy. Everything is set up and compared as integer bit patterns;
# the sentinels are NaN patterns in the float view.
# ---------------------------------------------------------------------------
_INT = {F32: torch.int32, BF16: torch.int16}
_PARENT_SENTINEL = {F32: 0x7FC0BEEF, BF16: 0x7FC1}
_BUCKET_SENTINEL = {F32: 0x7FC12345, BF16: 0x7FC2}
# fp32: exactly one 8192-byte plan row, one element more, two rows and a
# bit; bf16: odd lengths, so a row ends in a 2- or 6-byte tail
_MEMBERS = {F32: [2048, 2049, 4099], BF16: [1, 3, 4097, 8193]}


def _rand_bits(n, it, seed):
    g = torch.Generator().manual_seed(seed)
    hi = 2 ** 15 - 1 if it == torch.int16 else 2 ** 31 - 1
    return torch.randint(1, hi, (n,), generator=g, dtype=it)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bucket_copy_edges(dtype):
    it, esz = _INT[dtype], 2 if dtype == BF16 else 4
    align = 8 // esz  # members start on 8-byte multiples of the parent
    sizes = _MEMBERS[dtype]
    # members are slices of ONE sentinel-filled parent, guards on both sides
    starts, pos = [], 2 * align
    for n in sizes:
        starts.append(pos)
        pos = -(-(pos + n + align) // align) * align
    parent0 = torch.full((pos + align,), _PARENT_SENTINEL[dtype], dtype=it)
    for i, (s, n) in enumerate(zip(starts, sizes)):
        parent0[s:s + n] = _rand_bits(n, it, 30 + i)
    guard = torch.ones(parent0.numel(), dtype=torch.bool)
    for s, n in zip(starts, sizes):
        guard[s:s + n] = False
    parent = parent0.clone().to(DEV)
    members = [parent.view(dtype)[s:s + n] for s, n in zip(starts, sizes)]
    assert all(m.data_ptr() % 8 == 0 and m.is_contiguous() for m in members)
    # bucket offsets: 4-element aligned, with a padding gap after every member
    offsets, off = [], 4
    for n in sizes:
        offsets.append(off)
        off = ((off + n + 3) & ~3) + 4
    bucket0 = torch.full((off,), _BUCKET_SENTINEL[dtype], dtype=it)
    pad = torch.ones(off, dtype=torch.bool)
    for o, n in zip(offsets, sizes):
        pad[o:o + n] = False
    bucket = bucket0.clone().to(DEV)
    plan = _ext().build_copy_plan(members, offsets, 0)
    rows = sum(-(-n * esz // 8192) for n in sizes)
    assert tuple(plan.shape) == (rows, 3)
    assert int(plan[:, 2].max()) == 8192 and int(plan[:, 2].sum()) == \
        sum(sizes) * esz

    def check_bucket(what):
        got = bucket.cpu()
        for o, s, n in zip(offsets, starts, sizes):
            assert torch.equal(got[o:o + n], parent0[s:s + n]), \
                f"{what}: member of {n} elements"
        assert torch.equal(got[pad], bucket0[pad]), f"{what}: padding touched"

    _ext().flatten_into(bucket.view(dtype), plan, rows, False)
    check_bucket("flatten_into")
    assert torch.equal(parent.cpu(), parent0), "flatten_into wrote its source"

    _ext().flatten_into(bucket.view(dtype), plan, rows, True)
    check_bucket("flatten_into zero_src")
    got = parent.cpu()
    assert torch.equal(got[guard], parent0[guard]), "zero_src: guard touched"
    assert not got[~guard].any(), "zero_src: member not cleared"

    # new contents everywhere in the bucket, scattered back to the members
    new_bucket = _rand_bits(off, it, 40)
    bucket.copy_(new_bucket)
    _ext().unflatten_from(bucket.view(dtype), plan, rows)
    got = parent.cpu()
    for o, s, n in zip(offsets, starts, sizes):
        assert torch.equal(got[s:s + n], new_bucket[o:o + n]), \
            f"unflatten_from: member of {n} elements"
    assert torch.equal(got[guard], parent0[guard]), \
        "unflatten_from: guard touched"
    assert torch.equal(bucket.cpu(), new_bucket), "unflatten_from wrote bucket"


# ---------------------------------------------------------------------------
# Epoch shard: n off the powers of two, so the cycle walk takes further
# turns on the device, and n % world != 0
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _perm(seed, n):
    """The mirror's whole permutation for one epoch; running it first also
    shows that the walk terminates."""
    return [ops.perm_index(seed, p, n) for p in range(n)]


def _shard_data(n, K, dtype):
    """Rows that are all distinct, as bit patterns (NaNs among them)."""
    it = _INT[dtype]
    base = 0x7FC00000 if dtype == F32 else 0
    X = torch.arange(n * K, dtype=torch.int64).view(n, K) + base
    T = torch.arange(n, dtype=torch.int64).view(n, 1) * 3 + 7 + base
    if dtype == BF16:  # wrap into int16
        X = (X + 2 ** 15) % 2 ** 16 - 2 ** 15
        T = (T + 2 ** 15) % 2 ** 16 - 2 ** 15
    return X.to(it), T.to(it)


SHARD_CASES = [(n, world, (1, 20)[(i + j) % 2], (1, 3)[(i + j // 2) % 2])
               for i, n in enumerate([3, 5, 100, 1000, 2047, 2049])
               for j, world in enumerate([1, 3, 8]) if world <= n]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,world,K,epochs", SHARD_CASES)
def test_epoch_shard_edges(n, world, K, epochs, dtype):
    seed0 = 4242 + n
    per = n // world
    perms = [_perm(seed0 + e, n) for e in range(epochs)]  # mirror first
    for perm in perms:
        taken = perm[:per * world]
        assert len(set(taken)) == len(taken) and min(taken) >= 0 \
            and max(taken) < n
        assert sorted(perm) == list(range(n))
    Xi, Ti = _shard_data(n, K, dtype)
    X, T = Xi.view(dtype).to(DEV), Ti.view(dtype).to(DEV)
    for rank in range(world):
        xs, ts = _ext().epoch_shard_multi(X, T, seed0, epochs, rank, world)
        assert tuple(xs.shape) == (epochs * per, K) and xs.dtype == dtype
        assert tuple(ts.shape) == (epochs * per, 1) and ts.dtype == dtype
        idx = torch.tensor([perm[rank + i * world] for perm in perms
                            for i in range(per)])
        ko.assert_bitwise(xs, Xi[idx].view(dtype), f"xs rank {rank}")
        ko.assert_bitwise(ts, Ti[idx].view(dtype), f"ts rank {rank}")
        if epochs == 1:
            xs1, ts1 = _ext().epoch_shard(X, T, seed0, rank, world)
            ko.assert_bitwise(xs1, xs), ko.assert_bitwise(ts1, ts)


def test_shard_cases_cover_the_listed_values():
    assert {c[0] for c in SHARD_CASES} == {3, 5, 100, 1000, 2047, 2049}
    assert {c[1] for c in SHARD_CASES} == {1, 3, 8}
    assert {c[2] for c in SHARD_CASES} == {1, 20}
    assert {c[3] for c in SHARD_CASES} == {1, 3}
    assert any(n % w for n, w, _, _ in SHARD_CASES)
    for cases, ms, ks, ns in (
            (SERIAL, {64, 65, 80, 81}, {1, 3, 4, 5, 16, 17},
             {1, 15, 16, 17, 33}),
            (SPLIT, {1, 15, 16, 17, 63},
             {1, 3, 4, 5, 13, 17, 64, 67, 257}, {1, 15, 16, 17, 33})):
        assert ms <= {c[0] for c in cases}
        assert ks <= {c[1] for c in cases}
        assert ns <= {c[2] for c in cases}
    assert {1, 15, 16, 17, 63, 64, 65, 100, 129} == {c[1] for c in BWD_W}
    assert {1, 16, 17, 33} == {c[2] for c in BWD_W}
    assert {1, 3, 4, 5, 33} == {c[0] for c in BWD_W}
    assert {1, 3, 4, 5} == {c[0] for c in ko.CE_SHAPES}
    assert {1, 2, 63, 64, 65, 129} == {c[1] for c in ko.CE_SHAPES}


# ---------------------------------------------------------------------------
# Host-side guards: each raises (or returns the empty result) BEFORE any
# launch, so none of these hands a mismatched buffer or a zero-block grid
# to the runtime.
# ---------------------------------------------------------------------------
def _d(*shape, dtype=F32, device=DEV):
    return torch.ones(*shape, dtype=dtype, device=device)


def test_guard_linear_tile_bias():
    x, w = _d(4, 8), _d(5, 8)
    with pytest.raises(RuntimeError, match="bias must be"):
        _ext().linear_fwd(x, w, _d(5, dtype=BF16))
    with pytest.raises(RuntimeError, match="bias must be"):
        _ext().linear_fwd(x, w, _d(4))
    with pytest.raises(RuntimeError, match="bias must be"):
        _ext().linear_fwd(x, w, _d(5, 1))
    with pytest.raises(RuntimeError, match="bias must be"):
        _ext().linear_fwd(x, w, _d(5, device="cpu"))
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        _ext().linear_fwd(x, _d(5, 8, dtype=BF16))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        _ext().linear_bwd_input(x, _d(5, 8))
    with pytest.raises(RuntimeError, match="one device"):
        _ext().linear_fwd(x, w.cpu())
    with pytest.raises(RuntimeError, match="one device"):
        _ext().linear_bwd_input(x.cpu(), _d(8, 5))


def test_guard_linear_bwd_weight():
    x, dy, dw, db = _d(4, 8), _d(4, 5), _d(5, 8), _d(5)
    f = _ext().linear_bwd_weight
    for bad in ((x, _d(4, 5, dtype=BF16), dw, db),
                (x, dy, _d(5, 8, dtype=BF16), db),   # 4-byte stores, 2-byte dw
                (x, dy, dw, _d(5, dtype=BF16)),
                (x.bfloat16(), dy, dw, db)):
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(*bad, False)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        f(x, _d(3, 5), dw, db, False)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        f(x, _d(20), dw, db, False)
    with pytest.raises(RuntimeError, match="dw must be"):
        f(x, dy, _d(5, 7), db, False)
    with pytest.raises(RuntimeError, match="dw must be"):
        f(x, dy, _d(8, 5), db, False)
    with pytest.raises(RuntimeError, match="db must be"):
        f(x, dy, dw, _d(4), False)
    with pytest.raises(RuntimeError, match="one device"):
        f(x, dy, _d(5, 8, device="cpu"), db, False)
    with pytest.raises(RuntimeError, match="one device"):
        f(x, dy.cpu(), dw, db, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        f(x, dy, _d(8, 5).t(), db, False)


def test_guard_gemm_bf16():
    x, w, b = _d(4, 8, dtype=BF16), _d(5, 8, dtype=BF16), _d(5, dtype=BF16)
    f = _ext().gemm_bf16
    with pytest.raises(RuntimeError, match="x must be"):
        f(x.float(), w, b)
    with pytest.raises(RuntimeError, match="w must be"):
        f(x, w.float(), b)
    with pytest.raises(RuntimeError, match="w must be"):
        f(x, w.cpu(), b)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        f(x, _d(5, 9, dtype=BF16), b)
    with pytest.raises(RuntimeError, match="bias must be"):
        f(x, w, b.float())
    with pytest.raises(RuntimeError, match="bias must be"):
        f(x, w, _d(4, dtype=BF16))
    with pytest.raises(RuntimeError, match="bias must be"):
        f(x, w, b.cpu())


def test_guard_mse():
    y, t = _d(6), _d(6)
    for f in (_ext().mse_fwd, lambda a, b: _ext().mse_bwd(a, b, 1.0)):
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(y, t.bfloat16())  # would read past the end of t
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(y.bfloat16(), t)
        with pytest.raises(RuntimeError, match="one device"):
            f(y, t.cpu())
        with pytest.raises(RuntimeError, match="shape"):
            f(y, _d(6, 1))
        with pytest.raises(RuntimeError, match="shape"):
            f(y, _d(5))
    with pytest.raises(RuntimeError, match="gout must be"):
        _ext().mse_bwd(y, t, 1.0, torch.tensor(1.0))


def test_guard_ce():
    y, t = _d(3, 5), _d(3, 5)
    probs, tsum = _d(3, 5), _d(3)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        _ext().ce_fwd(y, t.bfloat16())
    with pytest.raises(RuntimeError, match="one device"):
        _ext().ce_fwd(y, t.cpu())
    with pytest.raises(RuntimeError, match=r"must be \[B,C\]"):
        _ext().ce_fwd(_d(15), _d(15))
    with pytest.raises(RuntimeError, match="must match"):
        _ext().ce_fwd(y, _d(3, 4))
    f = _ext().ce_bwd
    with pytest.raises(RuntimeError, match="f32 outputs"):
        f(probs.bfloat16(), t, tsum, 1.0)
    with pytest.raises(RuntimeError, match="f32 outputs"):
        f(probs, t, tsum.bfloat16(), 1.0)
    with pytest.raises(RuntimeError, match="match the targets"):
        f(probs, _d(3, 4), tsum, 1.0)
    with pytest.raises(RuntimeError, match="match the targets"):
        f(_d(5, 3).t(), t, tsum, 1.0)
    with pytest.raises(RuntimeError, match="tsum must be"):
        f(probs, t, _d(4), 1.0)
    with pytest.raises(RuntimeError, match="one device"):
        f(probs, t, tsum.cpu(), 1.0)
    with pytest.raises(RuntimeError, match="gout must be"):
        f(probs, t, tsum, 1.0, torch.tensor([1.0, 2.0], device=DEV))


def test_guard_bucket_copy_plan():
    m = _d(8)
    bucket = torch.zeros(16, device=DEV)
    plan = _ext().build_copy_plan([m], [4], 0)
    for f in (lambda *a: _ext().flatten_into(*a, False),
              _ext().unflatten_from):
        with pytest.raises(RuntimeError, match="outside the plan"):
            f(bucket, plan, 2)
        with pytest.raises(RuntimeError, match="outside the plan"):
            f(bucket, plan, -1)
        with pytest.raises(RuntimeError, match="plan must be"):
            f(bucket, plan.int(), 1)
        with pytest.raises(RuntimeError, match="plan must be"):
            f(bucket, plan.view(-1), 1)
        with pytest.raises(RuntimeError, match="one device"):
            f(bucket, plan.cpu(), 1)
        # empty work is a no-op, not a zero-block launch
        f(bucket, plan, 0)
        f(bucket, torch.empty(0, 3, dtype=torch.int64, device=DEV), 0)
    torch.cuda.synchronize()
    assert not bucket.any() and bool((m == 1).all())


def test_guard_epoch_shard():
    X, T = _d(5, 3), _d(5, 1)
    f = _ext().epoch_shard_multi
    with pytest.raises(RuntimeError, match="exceeds"):
        f(X, T, 1, 1, 0, 6)  # world > n: per_rank == 0
    with pytest.raises(RuntimeError, match="exceeds"):
        _ext().epoch_shard(X, T, 1, 0, 8)
    with pytest.raises(RuntimeError, match="outside world"):
        f(X, T, 1, 1, 3, 3)
    with pytest.raises(RuntimeError, match="outside world"):
        f(X, T, 1, 1, 0, 0)
    with pytest.raises(RuntimeError, match="share a device and a dtype"):
        f(X, T.bfloat16(), 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match=r"\[n,1\]"):
        f(X, _d(5), 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match="epochs out of range"):
        f(X, T, 1, 0, 0, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_work_returns_what_torch_returns(dtype):
    e = _ext()
    w, b = _d(5, 8, dtype=dtype), _d(5, dtype=dtype)
    y = e.linear_fwd(_d(0, 8, dtype=dtype), w, b)
    assert tuple(y.shape) == (0, 5) and y.dtype == dtype
    y = e.linear_fwd(_d(4, 8, dtype=dtype), _d(0, 8, dtype=dtype))
    assert tuple(y.shape) == (4, 0)
    dx = e.linear_bwd_input(_d(0, 5, dtype=dtype), w)
    assert tuple(dx.shape) == (0, 8) and dx.dtype == dtype
    # dW over an empty batch: zeros, or the old value under accumulate
    dw = torch.full((5, 8), float("nan"), dtype=dtype, device=DEV)
    db = torch.full((5,), float("nan"), dtype=dtype, device=DEV)
    e.linear_bwd_weight(_d(0, 8, dtype=dtype), _d(0, 5, dtype=dtype), dw, db,
                        False)
    assert not dw.any() and not db.any()
    dw.fill_(2.0), db.fill_(3.0)
    e.linear_bwd_weight(_d(0, 8, dtype=dtype), _d(0, 5, dtype=dtype), dw, db,
                        True)
    assert bool((dw == 2).all()) and bool((db == 3).all())
    if dtype == BF16:
        y = e.gemm_bf16(_d(0, 8, dtype=BF16), w, b)
        assert tuple(y.shape) == (0, 5) and y.dtype == BF16
    # losses: the mean over nothing is nan, the gradient is empty
    y0 = torch.empty(0, 5, dtype=dtype, device=DEV)
    assert torch.isnan(e.mse_fwd(y0, y0)).item()
    assert tuple(e.mse_bwd(y0, y0, 1.0).shape) == (0, 5)
    loss, probs, tsum = e.ce_fwd(y0, y0)
    assert torch.isnan(loss).item() and loss.dtype == F32
    assert tuple(probs.shape) == (0, 5) and tuple(tsum.shape) == (0,)
    dy = e.ce_bwd(probs, y0, tsum, 1.0)
    assert tuple(dy.shape) == (0, 5) and dy.dtype == dtype
    for fn in (ops.mse_loss, ops.cross_entropy):
        yg = y0.clone().requires_grad_(True)
        loss = fn(yg, y0)
        assert torch.isnan(loss).item()
        loss.backward()
        assert tuple(yg.grad.shape) == (0, 5)
    # ops.linear over an empty batch, through autograd
    x = torch.empty(0, 8, dtype=dtype, device=DEV, requires_grad=True)
    wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.linear(x, wg, bg)
    assert tuple(y.shape) == (0, 5)
    y.sum().backward()
    assert tuple(x.grad.shape) == (0, 8)
    assert not wg.grad.any() and not bg.grad.any()
    torch.cuda.synchronize()
