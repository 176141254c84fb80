"""fp32 emulation of the fused BatchNorm formulation (batchnorm_kernels.hip)
on the CPU in plain torch ops, over the cases of tests/test_batch_norm_gpu.py:
per-lane Welford on x - x[0, column] and a plain sum of x in the kernel's row
order, the Chan merges and the additions in the kernel's order (shift-down
tree in the wave, waves 1..3 into wave 0, slices by 16 waves and those in wave
order), the apply and backward formulas. It holds the FORMULATION to the
test's bound before any kernel runs; fused multiply-adds are not modelled, so
it does not give the kernel's bits. Prints the worst e / bound per result,
fp64 as reference and torch's CPU ops in the storage dtype as yardstick.

    python tools/emulate_batch_norm.py
"""
import itertools

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
EPS = {F32: 2.0 ** -24, BF16: 2.0 ** -9}
SHAPES = [(2, 4), (3, 64), (257, 12), (1030, 64), (70, 260), (37, 2048),
          (1100, 4096)]
FORMS = [(False, False), (True, False), (True, True)]
BN_EPS, MOM, TARGET = 1e-5, 0.1, 1024
STATS = ("mean", "rstd", "running_mean", "running_var", "dgamma", "dbeta")


def plan(R, C):
    nvec, LC = C // 4, 1
    while LC < min(nvec, 64):
        LC *= 2
    LR, slabs = 256 // LC, -(-nvec // LC)
    return LC, LR, min(-(-R // (4 * LR)), max(1, TARGET // slabs))


def chan(a, b):
    (na, ma, qa), (nb, mb, qb) = a, b
    n = na + nb
    w = torch.where(n > 0, nb / n, torch.zeros_like(n))
    d = mb - ma
    return n, ma + d * w, (qa + qb) + (d * d) * (na * w)


def add(a, b):
    return tuple(u + v for u, v in zip(a, b))


def walk(cols, valid, LR, GR, update, state):
    """Every thread (g, lr) over its rows in the kernel's order."""
    R = valid.numel()
    iters = -(-R // (4 * LR * GR))
    pad = iters * GR * 4 * LR - R
    cols = [F.pad(c, (0, 0, 0, pad)).view(iters, GR, 4, LR, -1) for c in cols]
    valid = F.pad(valid, (0, pad)).view(iters, GR, 4, LR, 1)
    for it, u in itertools.product(range(iters), range(4)):
        state = update(state, valid[it, :, u], *(c[it, :, u] for c in cols))
    return state


def reduce(rec, LC, GR, counts, merge):
    """Records [GR, LR, C] -> [C]: wave tree, waves in order, then finish."""
    rpw = max(1, 64 // LC)  # row lanes per wave
    rec = tuple(r.reshape(GR, 4, rpw, -1) for r in rec)
    off = rpw // 2
    while off:
        lo = merge(tuple(r[:, :, :off] for r in rec),
                   tuple(r[:, :, off:2 * off] for r in rec))
        rec = tuple(torch.cat([l, r[:, :, off:]], 2) for l, r in zip(lo, rec))
        off //= 2
    rec = tuple(r[:, :, 0] for r in rec)  # [GR, 4 waves, C]
    wg = tuple(r[:, 0] for r in rec)
    for w in range(1, 4):
        wg = merge(wg, tuple(r[:, w] for r in rec))
    if counts is not None:  # the finish kernel takes the counts from the plan
        wg = (counts.view(GR, 1).expand_as(wg[1]),) + wg[1:]
    zero = tuple(torch.zeros_like(r[0]) for r in wg)
    waves = []
    for w in range(16):
        acc = zero
        for k in range(w, GR, 16):
            acc = merge(acc, tuple(r[k] for r in wg))
        waves.append(acc)
    out = waves[0]
    for w in range(1, 16):
        out = merge(out, waves[w])
    return out


def emulate(t, relu, residual, dtype):
    x, res, dz = (t[k].to(dtype).float() for k in ("x", "res", "dz"))
    R, C = x.shape
    LC, LR, GR = plan(R, C)
    valid = torch.ones(R, dtype=torch.bool)

    def welford(s, ok, v):
        n, mean, m2 = s
        n = n + ok.float()
        inv = torch.where(ok, 1 / n.clamp(min=1), torch.zeros_like(n))
        d = torch.where(ok, v - mean, torch.zeros_like(v))
        mean = mean + d * inv
        return n, mean, m2 + d * (v - mean)

    def total(s, ok, v):
        return (s[0] + torch.where(ok, v, torch.zeros_like(v)),)

    z3 = torch.zeros(GR, LR, C)
    # M2 from Welford on x - x[0, column]; the mean from a plain sum of x
    rec = walk([x - x[0]], valid, LR, GR, welford,
               (torch.zeros(GR, LR, 1), z3, z3))
    counts = rec[0].sum((1, 2))
    rec = (rec[0].expand_as(z3),) + rec[1:]
    m2 = reduce(rec, LC, GR, counts, chan)[2]
    rows = torch.tensor(float(R))
    mean = reduce(walk([x], valid, LR, GR, total, (z3,)), LC, GR, None,
                  add)[0] / rows
    rstd = 1 / torch.sqrt(m2 / rows + BN_EPS)
    out = {"mean": mean, "rstd": rstd,
           "running_mean": MOM * mean + (1 - MOM) * t["rm"],
           "running_var": MOM * (m2 / (rows - 1)) + (1 - MOM) * t["rv"]}
    y = ((x - mean) * rstd) * t["w"] + t["b"]
    y = y + res if residual else y
    out["z"] = (y.relu() if relu else y).to(dtype)
    g = dz * (out["z"] > 0) if relu else dz

    def sums(s, ok, v, gg):
        gg = torch.where(ok, gg, torch.zeros_like(gg))
        return s[0] + gg, s[1] + gg * ((v - mean) * rstd)

    dbeta, dgamma = reduce(walk([x, g], valid, LR, GR, sums, (z3, z3)), LC, GR,
                           None, add)
    inv = 1 / rows
    out["dx"] = ((t["w"] * rstd) * ((g - dbeta * inv) - ((x - mean) * rstd)
                                    * (dgamma * inv))).to(dtype)
    out.update(dgamma=dgamma, dbeta=dbeta)
    if residual:
        out["dres"] = g.to(dtype)
    return out


def torch_path(t, z_ours, relu, residual, cast):
    x, res, w, b = (cast(t[k]).clone().requires_grad_(True)
                    for k in ("x", "res", "w", "b"))
    rm, rv = cast(t["rm"]).clone().float(), cast(t["rv"]).clone().float()
    if x.dtype == torch.float64:
        rm, rv = rm.double(), rv.double()
    y = F.batch_norm(x, rm, rv, w, b, True, MOM, BN_EPS)
    y = y + res if residual else y
    dz = cast(t["dz"])
    y.backward(dz * (z_ours > 0) if relu else dz)
    xf = x.detach().double() if x.dtype == torch.float64 else x.detach().float()
    out = {"z": (y.relu() if relu else y).detach(), "dx": x.grad,
           "mean": xf.mean(0),
           "rstd": (xf.var(0, unbiased=False) + BN_EPS).rsqrt(),
           "running_mean": rm, "running_var": rv, "dgamma": w.grad,
           "dbeta": b.grad}
    if residual:
        out["dres"] = res.grad
    return out


def err(got, ref):
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


def main():
    worst = {}
    for (R, C), kind, dtype in itertools.product(
            SHAPES, ("normal", "offset", "scaled", "constcol"), (F32, BF16)):
        g = torch.Generator().manual_seed(10000 * R + C)
        x = torch.randn(R, C, generator=g)
        if kind == "offset":
            x += 1000 if dtype == F32 else 64
        elif kind == "scaled":
            x *= torch.logspace(-3, 3, C)
        elif kind == "constcol":
            x[:, C // 2] = 3.25
        t = {"x": x, "res": torch.randn(R, C, generator=g),
             "dz": torch.randn(R, C, generator=g),
             "w": 1 + 0.5 * torch.randn(C, generator=g),
             "b": torch.randn(C, generator=g),
             "rm": torch.randn(C, generator=g),
             "rv": torch.rand(C, generator=g) + 0.5}
        stored = {k: v.to(dtype) if v.dim() == 2 else v for k, v in t.items()}
        for relu, residual in FORMS:
            ours = emulate(t, relu, residual, dtype)
            yard = torch_path(stored, ours["z"], relu, residual, lambda v: v)
            ref = torch_path(stored, ours["z"], relu, residual,
                             torch.Tensor.double)
            if kind == "constcol":
                assert float(ours["mean"][C // 2]) == 3.25, (R, C, dtype)
            for name in ours:
                eps = 2.0 ** -24 if name in STATS else EPS[dtype]
                e = err(ours[name], ref[name])
                ratio = e / (4 * max(err(yard[name], ref[name]), eps))
                if ratio > worst.get(name, (0, None))[0]:
                    worst[name] = (ratio, (R, C, kind, str(dtype), relu,
                                           residual))
    for name, (ratio, case) in sorted(worst.items()):
        print(f"{name:13s} worst e/bound {ratio:.3f} at {case}")


if __name__ == "__main__":
    main()
