"""GPU tests for the fused BatchNorm kernels (csrc/batchnorm_kernels.hip) and
what reaches them.

Reference: F.batch_norm, add, relu and their autograd gradients in fp64 from
the STORED operands. Yardstick: the same in the storage dtype on the device.
With e = max|got - ref| / max|ref| per result, e_ours <= 4 * max(e_torch, eps):
eps = 2^-24 (f32) or 2^-9 (bf16) for z, dx and dresidual; 2^-24 in BOTH
storage dtypes for col_stats, the running statistics, dgamma and dbeta, which
are f32 results of f32 arithmetic on exactly widened operands (so a dropped
row shows under bf16 storage too). The backward's ReLU mask is taken from the
stored z OUR forward returned, as the kernel takes it: reference and yardstick
get dz * (z > 0) as the gradient at the pre-activation."""

import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipBatchNorm2d, ResNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # sentinel elements on either side; keeps 16-byte alignment
F32 = torch.float32
EPS = {F32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
DTYPES = pytest.mark.parametrize("dtype", [F32, torch.bfloat16],
                                 ids=["f32", "bf16"])
FORMS = pytest.mark.parametrize(
    "relu,add", [(False, False), (True, False), (True, True)],
    ids=["bn", "bn_relu", "bn_add_relu"])
# (R, C) with the plan (LC, slabs, GR) each must get; kBnTargetGrid = 1024
SHAPES = {(2, 4): (1, 1, 1),        # 254 row lanes hold empty records
          (3, 64): (16, 1, 1),      # fewer rows than LR
          (257, 12): (4, 1, 2),     # a masked lane; one row past four blocks
          (1030, 64): (16, 1, 17),  # 17 workgroups, ragged last block
          (70, 260): (64, 2, 5),    # second slab holds a single vector
          (37, 2048): (64, 8, 3),   # eight slabs, LR = 4
          (1100, 4096): (64, 16, 64)}  # GR capped: strides twice, ends ragged
BN_EPS, MOM, CONST = 1e-5, 0.1, 3.25
STAT_NAMES = ("mean", "rstd", "running_mean", "running_var", "dgamma", "dbeta")


def _err(got, ref):
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


def _guarded(src, dtype):
    """A copy of `src` as `dtype` inside a larger NaN-filled allocation."""
    buf = torch.full((src.numel() + 2 * PAD,), float("nan"), dtype=dtype,
                     device=DEV)
    view = buf[PAD:PAD + src.numel()].view(src.shape)
    view.copy_(src)
    return buf, view


def _pads_intact(bufs):
    return all(bool(b[:PAD].isnan().all() and b[-PAD:].isnan().all())
               for b in bufs)


def _held(ours, torchs, refs, eps):
    bad = []
    for name, ref in refs.items():
        e_o, e_t = _err(ours[name], ref), _err(torchs[name], ref)
        bound = 4 * max(e_t, 2.0 ** -24 if name in STAT_NAMES else eps)
        print(f"{name}: e_ours {e_o:.3e} e_torch {e_t:.3e} "
              f"ratio {e_o / bound:.3f}")
        if not e_o <= bound:  # catches NaN too
            bad.append((name, e_o, bound))
    return bad


def _inputs(R, C, kind, dtype):
    """Guarded operands: ([buffers], {name: view}). Per-channel ones are f32."""
    g = torch.Generator().manual_seed(10000 * R + C)
    x = torch.randn(R, C, generator=g)
    if kind == "offset":
        x += 1000 if dtype == F32 else 64
    elif kind == "scaled":
        x *= torch.logspace(-3, 3, C)
    elif kind == "constcol":
        x[:, C // 2] = CONST
    srcs = {"x": x, "res": torch.randn(R, C, generator=g),
            "dz": torch.randn(R, C, generator=g),
            "w": 1 + 0.5 * torch.randn(C, generator=g),
            "b": torch.randn(C, generator=g),
            "rm": torch.randn(C, generator=g),
            "rv": torch.rand(C, generator=g) + 0.5}
    pairs = {k: _guarded(s, dtype if s.dim() == 2 else F32)
             for k, s in srcs.items()}
    return [p[0] for p in pairs.values()], {k: p[1] for k, p in pairs.items()}


def _outputs(R, C, dtype):
    """Guarded results, NaN-filled, and the zero batch counter."""
    nan = float("nan")
    pairs = {k: _guarded(torch.full(shape, nan), dt) for k, shape, dt in [
        ("z", (R, C), dtype), ("stats", (2, C), F32), ("dx", (R, C), dtype),
        ("dres", (R, C), dtype), ("dgamma", (C,), F32), ("dbeta", (C,), F32)]}
    outs = {k: p[1] for k, p in pairs.items()}
    outs["nbt"] = torch.zeros((), dtype=torch.long, device=DEV)
    return [p[0] for p in pairs.values()], outs


def _run(t, o, relu, add):
    """Forward and backward on the kernels; the results by name."""
    rm, rv = t["rm"].clone(), t["rv"].clone()
    ext = ops.ext()
    ext.bn_fwd(t["x"], t["w"], t["b"], rm, rv, True, MOM, BN_EPS, relu,
               residual=t["res"] if add else None,
               num_batches_tracked=o["nbt"], z=o["z"], col_stats=o["stats"])
    ext.bn_bwd(t["dz"], t["x"], o["stats"], t["w"], z=o["z"] if relu else None,
               add=add, dx=o["dx"], dresidual=o["dres"] if add else None,
               dgamma=o["dgamma"], dbeta=o["dbeta"])
    torch.cuda.synchronize()
    res = {"z": o["z"], "dx": o["dx"], "mean": o["stats"][0],
           "rstd": o["stats"][1], "running_mean": rm, "running_var": rv,
           "dgamma": o["dgamma"], "dbeta": o["dbeta"]}
    if add:
        res["dres"] = o["dres"]
    return res


def _torch(t, z_ours, relu, add, dt=None):
    """The same results from torch ops in dtype `dt` (None: as stored), the
    ReLU mask taken from z_ours."""
    cast = (lambda v: v.to(dt)) if dt else (lambda v: v)
    x, res, w, b = (cast(t[k]).clone().requires_grad_(True)
                    for k in ("x", "res", "w", "b"))
    rm, rv = cast(t["rm"]).clone(), cast(t["rv"]).clone()
    y = F.batch_norm(x, rm, rv, w, b, True, MOM, BN_EPS)
    if add:
        y = y + res
    dz = cast(t["dz"])
    y.backward(dz * (z_ours > 0) if relu else dz)
    if dt:
        mean = x.detach().mean(0)
        rstd = (x.detach().var(0, unbiased=False) + BN_EPS).rsqrt()
    else:
        mean, rstd = torch.batch_norm_stats(x.detach(), BN_EPS)
    out = {"z": (F.relu(y) if relu else y).detach(), "dx": x.grad,
           "mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv,
           "dgamma": w.grad, "dbeta": b.grad}
    if add:
        out["dres"] = res.grad
    return out


@DTYPES
@pytest.mark.parametrize("kind", ["normal", "offset", "scaled", "constcol"])
@FORMS
@pytest.mark.parametrize("R,C", SHAPES)
def test_kernels_against_fp64(R, C, relu, add, kind, dtype):
    assert tuple(ops.ext().bn_plan(R, C)) == SHAPES[R, C]
    ibufs, t = _inputs(R, C, kind, dtype)
    obufs, o = _outputs(R, C, dtype)
    ours = _run(t, o, relu, add)
    assert _pads_intact(ibufs + obufs) and int(o["nbt"]) == 1
    if not add:
        assert o["dres"].isnan().all()
    assert not _held(ours, _torch(t, o["z"], relu, add),
                     _torch(t, o["z"], relu, add, torch.float64), EPS[dtype])
    if kind == "constcol":  # Welford and the merges keep an exact zero
        want = 1 / math.sqrt(float(torch.tensor(BN_EPS, dtype=F32)))
        assert float(ours["mean"][C // 2]) == CONST
        assert abs(float(ours["rstd"][C // 2]) - want) <= want * 2.0 ** -23


@DTYPES
@pytest.mark.parametrize("R,C", [(1030, 64), (1100, 4096)])
def test_statistics_and_parameter_gradients_are_reproducible(R, C, dtype):
    _, t = _inputs(R, C, "normal", dtype)
    runs = [_run(t, _outputs(R, C, dtype)[1], True, True) for _ in range(2)]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in STAT_NAMES)


@DTYPES
def test_graph_replays_to_the_eager_bits(dtype):
    R, C = 257, 12
    _, t = _inputs(R, C, "normal", dtype)
    (_, eager), (_, o) = _outputs(R, C, dtype), _outputs(R, C, dtype)
    rm0, rv0 = t["rm"].clone(), t["rv"].clone()

    def step(o):
        ext = ops.ext()
        ext.bn_fwd(t["x"], t["w"], t["b"], t["rm"], t["rv"], True, MOM, BN_EPS,
                   True, residual=t["res"], num_batches_tracked=o["nbt"],
                   z=o["z"], col_stats=o["stats"])
        ext.bn_bwd(t["dz"], t["x"], o["stats"], t["w"], z=o["z"], add=True,
                   dx=o["dx"], dresidual=o["dres"], dgamma=o["dgamma"],
                   dbeta=o["dbeta"])

    step(eager), step(eager)
    want = [t["rm"].clone(), t["rv"].clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(o)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(o)
    t["rm"].copy_(rm0), t["rv"].copy_(rv0), o["nbt"].zero_()
    graph.replay(), graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(eager[k], o[k]) for k in eager)  # nbt == 2 too
    assert torch.equal(t["rm"], want[0]) and torch.equal(t["rv"], want[1])


@DTYPES
@FORMS
@pytest.mark.parametrize("R,C", [(1, 260), (257, 12), (70, 260)])
def test_evaluation_forward_against_fp64(R, C, relu, add, dtype):
    # one row is legal in evaluation; 260 channels so that max|ref| is the
    # scale of the operands and not one cancelled sum
    ibufs, t = _inputs(R, C, "normal", dtype)
    obufs, o = _outputs(R, C, dtype)
    rm, rv = t["rm"].clone(), t["rv"].clone()
    ops.ext().bn_fwd(t["x"], t["w"], t["b"], rm, rv, False, MOM, BN_EPS, relu,
                     residual=t["res"] if add else None,
                     num_batches_tracked=o["nbt"], z=o["z"])
    assert _pads_intact(ibufs + obufs) and int(o["nbt"]) == 0
    assert torch.equal(rm, t["rm"]) and torch.equal(rv, t["rv"])

    def want(cast):
        y = F.batch_norm(cast(t["x"]), cast(rm), cast(rv), cast(t["w"]),
                         cast(t["b"]), False, MOM, BN_EPS)
        y = y + cast(t["res"]) if add else y
        return {"z": F.relu(y) if relu else y}

    assert not _held(o, want(lambda v: v), want(torch.Tensor.double),
                     EPS[dtype])


def _bf16(t):
    return t.to(torch.bfloat16)


GUARDS = {  # name -> what it does to the arguments of a valid call
    "cpu": lambda a: a.update(x=a["x"].cpu()),
    "3-D": lambda a: a.update(x=a["x"].view(2, 4, 64)),
    "strided": lambda a: a.update(x=torch.zeros(8, 128, device=DEV)[:, :64]),
    "misaligned": lambda a: a.update(
        x=torch.zeros(8 * 64 + 1, device=DEV)[1:].view(8, 64)),
    "f16": lambda a: a.update(x=a["x"].half()),
    "residual dtype": lambda a: a.update(residual=_bf16(a["x"]), bwd_ok=True),
    "residual shape": lambda a: a.update(residual=a["x"][:4], bwd_ok=True),
    "dz dtype": lambda a: a.update(dz=_bf16(a["x"]), fwd_ok=True),
    "z dtype": lambda a: a.update(zin=_bf16(a["x"]), fwd_ok=True),
    "weight dtype": lambda a: a.update(weight=_bf16(a["weight"])),
    "weight length": lambda a: a.update(weight=a["weight"][:60]),
    "running_var length": lambda a: a.update(rv=a["rv"][:60], bwd_ok=True),
    "C=6": lambda a: a.update(x=a["x"][:, :6].contiguous()),
    "C=4100": lambda a: a.update(x=torch.zeros(8, 4100, device=DEV)),
    "R=1": lambda a: a.update(x=a["x"][:1], residual=None),
    "residual without relu": lambda a: a.update(relu=False),
    "col_stats shape": lambda a: a.update(stats=a["stats"].view(64, 2),
                                          fwd_ok=True),
    "counter dtype": lambda a: a.update(nbt=a["nbt"].int(), bwd_ok=True),
    "momentum": lambda a: a.update(momentum=1.5, bwd_ok=True),
    "eps": lambda a: a.update(eps=-1.0, bwd_ok=True),
    "evaluation with grad": lambda a: a.update(autograd=True),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    x = torch.randn(8, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    a = {"x": x, "residual": x.clone(), "dz": x.clone(), "zin": x.clone(),
         "weight": w, "rv": w.clone(), "stats": torch.ones(2, 64, device=DEV),
         "nbt": torch.zeros((), dtype=torch.long, device=DEV), "relu": True,
         "momentum": MOM, "eps": BN_EPS}
    GUARDS[name](a)
    nan = float("nan")
    z, dx, dres = (torch.full((8, 64), nan, device=DEV) for _ in range(3))
    stats_out = torch.full((2, 64), nan, device=DEV)
    rm, dgamma, dbeta = (torch.full((64,), nan, device=DEV) for _ in range(3))
    rv = a["rv"].fill_(nan)
    ext = ops.ext()
    if a.get("autograd"):
        with pytest.raises(RuntimeError):
            ext.batch_norm_act_autograd(x.requires_grad_(), w, w, rm, rv,
                                        training=False)
    elif not a.get("fwd_ok"):
        with pytest.raises(RuntimeError):
            ext.bn_fwd(a["x"], a["weight"], w, rm, rv, True, a["momentum"],
                       a["eps"], a["relu"], residual=a["residual"],
                       num_batches_tracked=a["nbt"], z=z, col_stats=stats_out)
    if not a.get("bwd_ok") and not a.get("autograd"):
        with pytest.raises(RuntimeError):
            ext.bn_bwd(a["dz"], a["x"], a["stats"], a["weight"],
                       z=a["zin"] if a["relu"] else None,
                       add=a["residual"] is not None, dx=dx, dresidual=dres,
                       dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    assert all(t.isnan().all()
               for t in (z, stats_out, rm, rv, dx, dres, dgamma, dbeta))
    assert int(a["nbt"]) == 0


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _results(mod, x, res, dz, relu, add, z_ours=None):
    """z, the gradients and the running statistics by name, on the [R, C]
    rows: through `mod`, a HipBatchNorm2d, on the 4-D tensors, or (z_ours
    given) from F.batch_norm on the rows with mod's parameters."""
    x, res = (t.detach().clone().requires_grad_(True) for t in (x, res))
    if z_ours is None:
        z = mod(x, residual=res if add else None)
        z.backward(dz)
        assert z.is_contiguous(memory_format=torch.channels_last)
    else:
        y = F.batch_norm(_rows(x), mod.running_mean, mod.running_var,
                         mod.weight, mod.bias, True, MOM, BN_EPS)
        y = y + _rows(res) if add else y
        z = (F.relu(y) if relu else y).view(_rows(dz).shape)
        dz = _rows(dz)
        y.backward(dz * (z_ours > 0) if relu else dz)
        z = z.view(x.shape[0], *x.shape[2:], -1).permute(0, 3, 1, 2)
    out = {"z": _rows(z.detach()), "dx": _rows(x.grad),
           "dgamma": mod.weight.grad, "dbeta": mod.bias.grad,
           "running_mean": mod.running_mean, "running_var": mod.running_var}
    if add:
        out["dres"] = _rows(res.grad)
    return out


@FORMS
@pytest.mark.parametrize("dtype,nhwc", [(torch.bfloat16, True), (F32, False)],
                         ids=["bf16-nhwc", "f32-nchw"])
def test_op_through_autograd_on_4d_input(dtype, nhwc, relu, add):
    torch.manual_seed(3)
    x, res, dz = (t.to(dtype) for t in
                  torch.randn(3, 3, 24, 5, 7, device=DEV).unbind(0))
    if nhwc:
        x, res = (t.contiguous(memory_format=torch.channels_last)
                  for t in (x, res))
    base = nn.BatchNorm2d(24).to(DEV)
    with torch.no_grad():
        base.weight.normal_(1, 0.5), base.bias.normal_()
    mods = [HipBatchNorm2d(24, act="relu" if relu else "none").to(DEV), base,
            nn.BatchNorm2d(24).to(DEV).double()]
    for m in mods:
        m.load_state_dict(base.state_dict())
    ours = _results(mods[0], x, res, dz, relu, add)
    assert int(mods[0].num_batches_tracked) == 1
    assert not _held(
        ours, _results(mods[1], x, res, dz, relu, add, ours["z"]),
        _results(mods[2], x.double(), res.double(), dz.double(), relu, add,
                 ours["z"]), EPS[dtype])


def test_small_resnet_trains():
    """Logits and running statistics of ResNet([1, 1, 1, 1], norm="hip")
    against the fp64 model, the f32 norm="torch" model as yardstick. Parameter
    gradients of the whole network are deliberately NOT held to a bound: two
    roundings of a pre-activation near zero give different ReLU masks, which
    is an error of neither path. They must exist, fit and be finite."""
    torch.manual_seed(7)
    base = ResNet([1, 1, 1, 1], 10).to(DEV)
    ours = ResNet([1, 1, 1, 1], 10, norm="hip").to(DEV)
    ref = ResNet([1, 1, 1, 1], 10).double()  # on the CPU: the fc has no fp64
    ours.load_state_dict(base.state_dict())
    ref.load_state_dict(base.state_dict())
    x = torch.rand(4, 3, 64, 64, device=DEV)
    outs = []
    for m, xin in ((ours, x), (base, x), (ref, x.double().cpu())):
        out = {"logits": m(xin)}
        out.update({k: v for k, v in m.state_dict().items() if "running" in k})
        outs.append({k: v.detach().to(DEV) for k, v in out.items()})
    assert not _held(outs[0], outs[1], outs[2], EPS[F32])
    assert all(int(v) == 1 for k, v in ours.state_dict().items()
               if "num_batches" in k)
    ops.cross_entropy_index(ours(x), torch.tensor([1, 2, 3, 4], device=DEV)) \
        .backward()
    assert all(p.grad is not None and p.grad.shape == p.shape
               and torch.isfinite(p.grad).all() for p in ours.parameters())
