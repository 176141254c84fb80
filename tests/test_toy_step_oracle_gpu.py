"""The toy training-step kernels (csrc/toy_kernels.hip) held to the fp64 step
oracle of tests/toy_oracle.py: k_toy_fused, the generic k_toy_multistep,
and the three fast paths (k_toy_multistep_spec, k_toy_multistep_chain,
k_toy_multistep_bf16w), plus the argument guards of every entry point.

Every case is one workgroup and at most four steps. Three instruments:
  bound     random operands against the propagated per-element bound
  int       integer-coded operands that must come out EXACT (one dropped
            row or column hides under any bound)
  zero      bf16 from w = b = 0 at lr 1, where the bound is 2^-8 of the
            gradient itself
Multi-step runs compound no tolerance: S launches of one step are each
held to the oracle from the params the previous one STORED (teacher
forcing), and one launch of S steps must equal them bitwise, loss word
included.

Every param, grad and loss buffer is a slice from the middle of a larger
allocation filled with distinct NaN patterns; whatever the kernel was not
asked to write must keep its bits. The guard tests use the same buffers, so
even a missing guard could write only into memory the test owns."""

import collections

import pytest
import torch

import toy_oracle as to
from toy_oracle import BF16, F32
from mi355x_ddp import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [F32, BF16]
IDS = ["f32", "bf16"]
PAD = 64  # sentinel elements on either side of a buffer


def _ext():
    return ops.ext()


# (w_off, b_off) of K weights and a bias
LAYOUTS = {
    "w0": lambda K: (0, K),         # w | b, as the engines lay it out
    "bias-first": lambda K: (1, 0),  # odd w_off
    "gap": lambda K: (4, K + 9),
}


def _sentinels(n, dtype):
    """n distinct-looking NaN patterns of `dtype` (quiet NaNs with a
    payload, so a copied neighbour shows as well as a computed value)."""
    i = torch.arange(n)
    if dtype == F32:
        return (0x7FC00001 + i % 0x3FFFF0).to(torch.int32).view(F32)
    return (0x7FC1 + i % 62).to(torch.int16).view(BF16)


class Bucket:
    """`buf`: the n-element tensor the kernel is given, cut from the middle
    of `whole`. live = the positions the call may write."""

    def __init__(self, dtype, n, live=()):
        self.whole = _sentinels(PAD + n + PAD, dtype).to(DEV)
        self.buf = self.whole[PAD:PAD + n]
        assert self.buf.is_contiguous() and self.buf.numel() == n
        self.keep = torch.ones(self.whole.numel(), dtype=torch.bool)
        for i in live:
            self.keep[PAD + i] = False
        self.before = None

    def arm(self):
        self.before = self.whole.cpu().clone()
        return self

    def _bits(self, t):
        it = torch.int32 if t.element_size() == 4 else torch.int16
        return t.cpu().contiguous().view(it)

    def assert_rest_untouched(self, what):
        now, was = self._bits(self.whole), self._bits(self.before)
        bad = ((now != was) & self.keep).nonzero().flatten().tolist()
        assert not bad, (f"{what}: written outside its slots at whole-buffer "
                         f"index {bad} (buffer starts at {PAD})")

    def assert_untouched(self, what):
        to.assert_bitwise(self.whole, self.before, what)


class Params(Bucket):
    def __init__(self, dtype, K, layout, w=None, b=None):
        self.K = K
        self.w_off, self.b_off = LAYOUTS[layout](K)
        n = max(self.w_off + K, self.b_off + 1) + 3
        live = list(range(self.w_off, self.w_off + K)) + [self.b_off]
        super().__init__(dtype, n, live)
        if w is not None:
            self.buf[self.w_off:self.w_off + K] = w.to(DEV)
            self.buf[self.b_off] = b.to(DEV)[0]
        self.arm()

    @property
    def w(self):
        return self.buf[self.w_off:self.w_off + self.K].cpu()

    @property
    def b(self):
        return self.buf[self.b_off].cpu()


def _loss_word():
    return Bucket(F32, 1, live=[0]).arm()


# worst error/tol per (family, quantity), printed once at the end (-s)
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (family, name), r in sorted(WORST.items()):
        print(f"\nworst error/tol {family:18s} {name:5s} {r:.3g}", end="")
    print()


def _within(family, name, got, ref, tol, what):
    r = to.assert_within(got, ref, tol, f"{what} {name}")
    WORST[family, name] = max(WORST[family, name], r)


@pytest.fixture(autouse=True)
def _restore_impl():
    ext = _ext()
    before = ext.get_toy_multistep_impl()
    yield
    ext.set_toy_multistep_impl(before)
    ext.set_toy_multistep_chain_depth(0)


def _operands(kind, rows, K, dtype, seed, B=None):
    """CPU operands in storage dtype; "int" and "largecol" beside the
    oracle's kinds."""
    if kind == "int":
        assert rows == B
        return to.int_case(B, K, dtype)
    if kind == "clampcol":
        # The fast kernels load X raw with k clamped to K-1, so for k >= K
        # the A operand repeats column K-1; the contract is that the w
        # operand is ZERO there. A pad that repeated w[K-1] as well would add
        # (pad width) * x[m][K-1] * w[K-1] to y: here +-8 * 0.75 per padded
        # k, far outside the bound, while the true term stays moderate.
        x, t, w, b, lr = to.inputs("signed", rows, K, dtype, seed)
        x[:, K - 1] = 8.0 * (1 - 2 * (torch.arange(rows) % 2)).to(dtype)
        w[K - 1] = 0.75
        return x, t, w, b, lr
    if kind == "largecol":
        # large finite values in the last column, against w[K-1] = 0: they
        # contribute nothing to y, and the fast kernels' raw operands
        # clamped to column K-1 for k >= K must contribute nothing either.
        # With w[K-1] = 0 this sees a small non-zero or garbage pad (times
        # 2^100) and Inf/NaN, not a pad that repeats w[K-1]: that is
        # "clampcol" above.
        x, t, w, b, lr = to.inputs("signed", rows, K, dtype, seed)
        x[:, K - 1] = (2.0 ** 100) * (1 - 2 * (torch.arange(rows) % 2)).to(dtype)
        w[K - 1] = 0
        return x, t, w, b, 2.0 ** -110
    return to.inputs(kind, rows, K, dtype, seed)


# ---------------------------------------------------------------------------
# k_toy_fused
# ---------------------------------------------------------------------------
# (32, 20) the flagship; (16, 16), (16, 32) K a multiple of 16 (wave-sum db);
# (33, 32) two K-tiles, ragged last M-tile; (17, 17) db column in the second
# K-tile; (5, 3), (1, 1), (4, 4) one partial tile; (128, 20) the largest
# instantiation; (32, 15), (64, 31) db in lane r = 15 of K-tile 0 / 1;
# (128, 32) both limits; (127, 31) both one short of them
SHAPES = [(32, 20), (48, 12), (16, 16), (33, 32), (17, 17), (5, 3),
          (128, 20), (1, 1), (4, 4), (32, 15), (64, 31), (16, 32), (128, 32),
          (127, 31)]
SHAPE_LAYOUTS = ([(B, K, "w0") for B, K in SHAPES]
                 + [(17, 17, "bias-first"), (17, 17, "gap"),
                    (64, 31, "bias-first")])
GENERIC_MULTI = [c for c in SHAPE_LAYOUTS if c[:2] != (32, 20)]


def _pow2(B):
    return B & (B - 1) == 0


def _kinds(dtype, B):
    kinds = ["uniform", "signed", "normal100"]
    if dtype == BF16:
        kinds.append("zero")
    if _pow2(B):
        kinds.append("int")
    return kinds


def _each_kind(kinds, case):
    """Runs case(kind) for every kind and reports every failing instrument,
    not the first alone: which of them sees a fault is part of the finding."""
    failed = []
    for kind in kinds:
        try:
            case(kind)
        except AssertionError as e:
            failed.append(f"[{kind}] {e}")
    assert not failed, "\n".join(failed)


def _fused_call(dtype, x, t, w, b, layout, lr, use_mse=True):
    B, K = x.shape
    P = Params(dtype, K, layout, w, b)
    G = Params(dtype, K, layout)  # sentinels in the live slots too
    L = _loss_word()
    _ext().toy_fused_fwd_bwd(x.to(DEV), t.to(DEV), P.buf, G.buf, L.buf,
                             use_mse, P.w_off, P.b_off, lr)
    torch.cuda.synchronize()
    return P, G, L


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,K,layout", SHAPE_LAYOUTS)
def test_fused_step(B, K, layout, dtype):
    fam = f"fused-{IDS[DTYPES.index(dtype)]}"

    def case(kind):
        what = f"fused {B}x{K} {layout} {kind}"
        x, t, w, b, lr = _operands(kind, B, K, dtype, seed=1, B=B)
        ref, tol = to.toy_step_ref(x, t, w, b, lr, storage=dtype)
        if kind == "int":
            ref = to.assert_step_exact(x, t, w, b, lr, what=what)
        # lr = 0: gradients and loss, params untouched
        P, G, L = _fused_call(dtype, x, t, w, b, layout, 0.0)
        P.assert_untouched(what + " lr=0 params")
        G.assert_rest_untouched(what + " lr=0 grads")
        L.assert_rest_untouched(what + " lr=0 loss")
        if kind == "int":
            to.assert_equal_exact(G.w, ref.dw, what + " dw")
            to.assert_equal_exact(G.b, ref.db, what + " db")
            to.assert_equal_exact(L.buf[0], ref.loss, what + " loss")
        else:
            e_dw, e_db = to.stored_grad_tol(ref, tol, dtype)
            _within(fam, "dw", G.w, ref.dw, e_dw, what)
            _within(fam, "db", G.b, ref.db, e_db, what)
            _within(fam, "loss", L.buf[0], ref.loss, tol.loss, what)
        # lr > 0: params and loss, grads untouched
        P, G, L = _fused_call(dtype, x, t, w, b, layout, lr)
        G.assert_untouched(what + " lr>0 grads")
        P.assert_rest_untouched(what + " lr>0 params")
        L.assert_rest_untouched(what + " lr>0 loss")
        if kind == "int":
            to.assert_equal_exact(P.w, ref.w, what + " w'")
            to.assert_equal_exact(P.b, ref.b, what + " b'")
            to.assert_equal_exact(L.buf[0], ref.loss, what + " loss")
        else:
            _within(fam, "w", P.w, ref.w, tol.w, what)
            _within(fam, "b", P.b, ref.b, tol.b, what)
            _within(fam, "loss", L.buf[0], ref.loss, tol.loss, what)

    _each_kind(_kinds(dtype, B), case)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,K,layout", [(32, 20, "w0"), (16, 16, "w0"),
                                        (17, 17, "bias-first"),
                                        (128, 32, "gap"), (1, 1, "w0")])
def test_fused_step_degenerate_ce(B, K, layout, dtype):
    """use_mse=False (CE over one logit): loss +0.0, dY = 0."""
    x, t, w, b, lr = _operands("signed", B, K, dtype, seed=2)
    zero_bits = torch.zeros(1, dtype=torch.int32)
    # lr > 0: the params keep their BITS
    P, G, L = _fused_call(dtype, x, t, w, b, layout, lr, use_mse=False)
    P.assert_untouched("CE lr>0 params")
    G.assert_untouched("CE lr>0 grads")
    assert torch.equal(L.buf.view(torch.int32).cpu(), zero_bits)
    # lr = 0: K + 1 gradient words of +0.0
    P, G, L = _fused_call(dtype, x, t, w, b, layout, 0.0, use_mse=False)
    P.assert_untouched("CE lr=0 params")
    G.assert_rest_untouched("CE lr=0 grads")
    to.assert_bitwise(G.w, torch.zeros(K, dtype=dtype), "CE dw")
    to.assert_bitwise(G.b, torch.zeros((), dtype=dtype), "CE db")
    assert torch.equal(L.buf.view(torch.int32).cpu(), zero_bits)


# ---------------------------------------------------------------------------
# toy_multistep: teacher-forced single-step launches, then one launch of S
# ---------------------------------------------------------------------------
def _multistep_case(fam, dtype, B, K, S, kind, layout, *, bf16_mfma=False,
                    dy_bf16=False, use_mse=True, seed=3):
    ext = _ext()
    what = f"{fam} {B}x{K} S={S} {layout} {kind}"
    x, t, w, b, lr = _operands(kind, S * B, K, dtype, seed, B=B)
    xd, td = x.to(DEV), t.to(DEV)
    P = Params(dtype, K, layout, w, b)
    L = _loss_word()
    for s in range(S):
        ws, bs = P.w, P.b.reshape(1)  # what the previous launch STORED
        xs, ts = x[s * B:(s + 1) * B], t[s * B:(s + 1) * B]
        ref, tol = to.toy_step_ref(xs, ts, ws, bs, lr, bf16_mfma=bf16_mfma,
                                   dy_bf16=dy_bf16, storage=dtype)
        if kind == "int":
            ref = to.assert_step_exact(xs, ts, ws, bs, lr, dy_bf16=dy_bf16,
                                       what=what)
        P.arm()
        L.arm()
        ext.toy_multistep(xd[s * B:(s + 1) * B], td[s * B:(s + 1) * B], P.buf,
                          L.buf, use_mse, P.w_off, P.b_off, lr, B)
        torch.cuda.synchronize()
        P.assert_rest_untouched(f"{what} step {s} params")
        L.assert_rest_untouched(f"{what} step {s} loss")
        if not use_mse:
            P.assert_untouched(f"{what} step {s} CE params")
            assert L.buf.view(torch.int32).item() == 0
        elif kind == "int":
            to.assert_equal_exact(P.w, ref.w, what + " w'")
            to.assert_equal_exact(P.b, ref.b, what + " b'")
            to.assert_equal_exact(L.buf[0], ref.loss, what + " loss")
        else:
            _within(fam, "w", P.w, ref.w, tol.w, f"{what} step {s}")
            _within(fam, "b", P.b, ref.b, tol.b, f"{what} step {s}")
            _within(fam, "loss", L.buf[0], ref.loss, tol.loss,
                    f"{what} step {s}")
    # one launch of all S steps: the same bits, sentinels and loss word too
    P1 = Params(dtype, K, layout, w, b)
    L1 = _loss_word()
    ext.toy_multistep(xd, td, P1.buf, L1.buf, use_mse, P1.w_off, P1.b_off,
                      lr, B)
    torch.cuda.synchronize()
    to.assert_bitwise(P1.whole, P.whole, what + ": one launch vs S launches")
    to.assert_bitwise(L1.whole, L.whole, what + ": loss word, one launch")


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,K,layout", GENERIC_MULTI)
def test_generic_multistep(B, K, layout, dtype, S):
    fam = f"generic-multi-{IDS[DTYPES.index(dtype)]}"
    # int and zero are sharp only from their own start
    kinds = [k for k in _kinds(dtype, B) if S == 1 or k not in ("int", "zero")]
    _each_kind(kinds, lambda kind: _multistep_case(fam, dtype, B, K, S, kind,
                                                   layout))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_generic_multistep_degenerate_ce(dtype):
    _multistep_case("generic-ce", dtype, 17, 17, 3, "signed", "bias-first",
                    use_mse=False)


# path -> (dtype, impl, ring depth, oracle flags)
FAST = {
    "mfma": (F32, "mfma", 0, {}),
    "chain-d2": (F32, "chain", 2, {}),
    "chain-d4": (F32, "chain", 4, {}),  # clamped to 2 at batch 64
    "bf16w": (BF16, None, 0, dict(bf16_mfma=True, dy_bf16=True)),
}


def _fast(path):
    dtype, impl, depth, flags = FAST[path]
    if impl is not None:
        _ext().set_toy_multistep_impl(impl)
        _ext().set_toy_multistep_chain_depth(depth)
    return dtype, flags


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("path", list(FAST))
def test_fast_multistep(path, B, S):
    """S in {1, 2, 3, 4}: both operand register sets and the tail."""
    dtype, flags = _fast(path)
    kinds = ["uniform", "signed", "normal100"]
    if S == 1:
        kinds += (["int", "largecol", "clampcol"]
                  + (["zero"] if dtype == BF16 else []))
    _each_kind(kinds, lambda kind: _multistep_case(
        "fast-" + path, dtype, B, 20, S, kind, "w0", **flags))


@pytest.mark.parametrize("layout", ["bias-first", "gap"])
@pytest.mark.parametrize("path", list(FAST))
def test_fast_multistep_layouts(path, layout):
    dtype, flags = _fast(path)
    _multistep_case("fast-" + path, dtype, 32, 20, 3, "signed", layout,
                    **flags)
    _multistep_case("fast-" + path, dtype, 32, 20, 1, "int", layout, **flags)


@pytest.mark.parametrize("path", list(FAST))
def test_fast_multistep_degenerate_ce(path):
    dtype, flags = _fast(path)
    _multistep_case("fast-ce", dtype, 64, 20, 3, "signed", "gap",
                    use_mse=False, **flags)


# ---------------------------------------------------------------------------
# argument guards: RuntimeError before anything is launched, every buffer
# bitwise as it was
# ---------------------------------------------------------------------------
B0, K0 = 32, 20


class Args:
    """A valid call's arguments; a guard case breaks exactly one."""

    def __init__(self, dtype=F32, rows=2 * B0):
        x, t, w, b, lr = to.inputs("signed", rows, K0, dtype, seed=5)
        self.x, self.t = x.to(DEV), t.to(DEV)
        self.P = Params(dtype, K0, "w0", w, b)
        self.G = Params(dtype, K0, "w0")
        self.L = _loss_word()
        self.param, self.grad, self.loss = self.P.buf, self.G.buf, self.L.buf
        self.w_off, self.b_off = self.P.w_off, self.P.b_off
        self.lr, self.batch = lr, B0

    def buckets(self):
        return [("param", self.P), ("grad", self.G), ("loss", self.L)]


def _other(dtype):
    return BF16 if dtype == F32 else F32


def _strided(t):
    big = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    return big[::2]


# name -> (entries it applies to, what it breaks, message fragment)
ALL = ("fused", "fused0", "multistep", "mesh", "shard")
MULTI = ("multistep", "mesh", "shard")
GUARDS = {
    "x_on_cpu": (ALL, lambda a: setattr(a, "x", a.x.cpu()), "x must be on a GPU"),
    "t_on_cpu": (ALL, lambda a: setattr(a, "t", a.t.cpu()), "t must be"),
    "param_on_cpu": (ALL, lambda a: setattr(a, "param", a.param.cpu()),
                     "param"),
    "grad_on_cpu": (("fused", "fused0"),
                    lambda a: setattr(a, "grad", a.grad.cpu()), "grad_flat"),
    "loss_on_cpu": (ALL, lambda a: setattr(a, "loss", a.loss.cpu()),
                    "loss_out"),
    "x_f64": (ALL, lambda a: setattr(a, "x", a.x.double()), "dtype"),
    "x_1d": (ALL, lambda a: setattr(a, "x", a.x.reshape(-1)), "[rows, K]"),
    "x_3d": (ALL, lambda a: setattr(a, "x", a.x.reshape(2, -1, K0)),
             "[rows, K]"),
    "x_not_contiguous": (ALL, lambda a: setattr(
        a, "x", a.x.t().contiguous().t()), "[rows, K]"),
    "t_not_contiguous": (ALL, lambda a: setattr(
        a, "t", _strided(a.t.reshape(-1))), "t must be"),
    "t_short": (ALL, lambda a: setattr(a, "t", a.t[:-1]), "t must be"),
    "t_long": (ALL, lambda a: setattr(a, "t", torch.cat([a.t, a.t])),
               "t must be"),
    "t_other_dtype": (ALL, lambda a: setattr(a, "t", a.t.to(_other(a.t.dtype))),
                      "t must be"),
    "param_other_dtype": (ALL, lambda a: setattr(
        a, "param", a.param.view(torch.int16).view(BF16)
        if a.param.dtype == F32 else a.param.float()), "param"),
    "grad_other_dtype": (("fused", "fused0"), lambda a: setattr(
        a, "grad", a.grad.view(torch.int16).view(BF16)
        if a.grad.dtype == F32 else a.grad.float()), "grad_flat"),
    "param_not_contiguous": (ALL, lambda a: setattr(
        a, "param", _strided(a.param)), "param"),
    "grad_not_contiguous": (("fused", "fused0"), lambda a: setattr(
        a, "grad", _strided(a.grad)), "grad_flat"),
    "batch_0": (MULTI, lambda a: setattr(a, "batch", 0), "batch"),
    "batch_negative": (MULTI, lambda a: setattr(a, "batch", -32), "batch"),
    "batch_129": (ALL, lambda a: (
        setattr(a, "x", torch.zeros(258, K0, dtype=a.x.dtype, device=DEV)),
        setattr(a, "t", torch.zeros(258, 1, dtype=a.x.dtype, device=DEV)),
        setattr(a, "batch", 129)), "batch"),
    "rows_not_multiple": (MULTI, lambda a: (setattr(a, "x", a.x[:-1]),
                                            setattr(a, "t", a.t[:-1])),
                          "multiple of batch"),
    "K_0": (ALL, lambda a: setattr(a, "x", a.x[:, :0].contiguous()),
            "1 <= K <= 32"),
    "K_33": (ALL, lambda a: setattr(
        a, "x", torch.zeros(a.x.shape[0], 33, dtype=a.x.dtype, device=DEV)),
        "1 <= K <= 32"),
    "w_off_negative": (ALL, lambda a: setattr(a, "w_off", -1), "w_off/b_off"),
    "b_off_negative": (ALL, lambda a: setattr(a, "b_off", -1), "w_off/b_off"),
    "w_off_past_end": (ALL, lambda a: (setattr(a, "w_off", a.param.numel() - K0 + 1),
                                       setattr(a, "b_off", 0)), "w_off/b_off"),
    "b_off_past_end": (ALL, lambda a: setattr(a, "b_off", a.param.numel()),
                       "w_off/b_off"),
    "offsets_past_int32": (ALL, lambda a: setattr(a, "w_off", 2 ** 32),
                           "w_off/b_off"),
    "b_off_inside_weights": (ALL, lambda a: setattr(a, "b_off", a.w_off + K0 - 1),
                             "inside the weights"),
    "b_off_is_w_off": (ALL, lambda a: setattr(a, "b_off", a.w_off),
                       "inside the weights"),
    "grad_undefined_lr0": (("fused0",), lambda a: setattr(
        a, "grad", torch.Tensor()), "grad_flat is required"),
    "grad_too_short_lr0": (("fused0",), lambda a: setattr(
        a, "grad", a.grad[:K0]), "grad_flat"),
    "loss_f64": (ALL, lambda a: setattr(
        a, "loss", torch.zeros(1, dtype=torch.float64, device=DEV)),
        "loss_out"),
    "lr_0": (MULTI, lambda a: setattr(a, "lr", 0.0), "lr"),
    "lr_rounds_to_0": (MULTI, lambda a: setattr(a, "lr", 1e-60), "lr"),
}
GUARD_CASES = [pytest.param(e, g, id=f"{g}-{e}")
               for g, (entries, _, _) in GUARDS.items() for e in entries]


@pytest.fixture(scope="module")
def unconnected_mesh():
    """A mesh that was never connected: toy_multistep_mesh refuses it, after
    the tensor guards and before it takes a sequence number or launches."""
    return _ext().P2pMesh(0, 2, 0)


def _invoke(entry, a, mesh):
    ext = _ext()
    if entry in ("fused", "fused0"):
        # the single step takes the whole of x as its batch
        ext.toy_fused_fwd_bwd(a.x, a.t, a.param, a.grad, a.loss, True,
                              a.w_off, a.b_off,
                              a.lr if entry == "fused" else 0.0)
    elif entry == "multistep":
        ext.toy_multistep(a.x, a.t, a.param, a.loss, True, a.w_off, a.b_off,
                          a.lr, a.batch)
    elif entry == "mesh":
        ext.toy_multistep_mesh(a.x, a.t, a.param, a.loss, True, a.w_off,
                               a.b_off, a.lr, a.batch, mesh)
    else:
        run = ext.ToyShardRun(a.param, a.loss, True, a.w_off, a.b_off, a.lr,
                              8, 0, 2.0)
        run.bind_shard(a.x, a.t, a.batch)
        run.step_shard(0)  # pending only: max_defer is 8
        return run


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("entry,guard", GUARD_CASES)
def test_guard(entry, guard, dtype, unconnected_mesh):
    _, breaker, fragment = GUARDS[guard]
    a = Args(dtype, rows=B0 if entry.startswith("fused") else 2 * B0)
    breaker(a)
    with pytest.raises(RuntimeError) as err:
        run = _invoke(entry, a, unconnected_mesh)
        del run
    torch.cuda.synchronize()
    msg = str(err.value)
    assert "not connected" not in msg, msg  # the tensor guard came first
    # the stepper's constructor checks flat_param, loss_out, lr and the
    # offsets' range itself; its wording carries the same fragments
    assert fragment in msg, msg
    for name, bucket in a.buckets():
        bucket.assert_untouched(f"{guard} via {entry}: {name}")


def test_guard_mesh_not_connected(unconnected_mesh):
    a = Args()
    with pytest.raises(RuntimeError, match="not connected"):
        _invoke("mesh", a, unconnected_mesh)
    torch.cuda.synchronize()
    for name, bucket in a.buckets():
        bucket.assert_untouched(f"unconnected mesh: {name}")


def test_guard_mesh_shape_outside_fast_paths(unconnected_mesh):
    a = Args()
    a.batch = 16
    with pytest.raises(RuntimeError, match="fast-path shapes"):
        _invoke("mesh", a, unconnected_mesh)
    a.P.assert_untouched("mesh batch 16")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("entry", ["fused", "fused0", "multistep", "shard"])
def test_zero_rows_launch_nothing(entry, dtype):
    a = Args(dtype)
    a.x, a.t = a.x[:0], a.t[:0]
    if entry == "shard":
        run = _ext().ToyShardRun(a.param, a.loss, True, a.w_off, a.b_off,
                                 a.lr, 8, 0, 2.0)
        run.bind_shard(a.x, a.t, a.batch)
        with pytest.raises(IndexError):
            run.step_shard(0)
        run.flush()
        assert run.launch_count == 0
    else:
        _invoke(entry, a, None)
    torch.cuda.synchronize()
    for name, bucket in a.buckets():
        bucket.assert_untouched(f"zero rows via {entry}: {name}")


def test_valid_call_of_every_entry_passes_the_guards():
    """The Args every guard case starts from is a valid call: it trains."""
    for entry in ("fused", "fused0", "multistep", "shard"):
        a = Args()
        if entry.startswith("fused"):
            a.x, a.t = a.x[:B0], a.t[:B0]
        run = _invoke(entry, a, None)
        if run is not None:
            run.step_shard(1)
            run.flush()
        torch.cuda.synchronize()
        changed = a.G if entry == "fused0" else a.P
        with pytest.raises(AssertionError):
            changed.assert_untouched(entry)
        changed.assert_rest_untouched(entry)


def test_fused_step_without_a_grad_bucket_when_it_applies_sgd():
    """lr > 0 never touches grad_flat, so an empty tensor stands for none."""
    a = Args(rows=B0)
    a.grad = torch.Tensor()
    _invoke("fused", a, None)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        a.P.assert_untouched("trained")
    a.P.assert_rest_untouched("no grad bucket")
    a.G.assert_untouched("no grad bucket")
