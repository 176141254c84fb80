"""CPU tier of the fused global grad-norm clipping of the flat-bucket
optimizers (`max_grad_norm` of FusedSGD / FusedAdamW): the plain-torch
mirrors of ops.grad_sumsq_flat_ / ops.clip_coef_ and of the `grad_scale` of
the update ops against torch.nn.utils.clip_grad_norm_ + torch.optim, the
interface (errors, state_dict) and a gloo world of 2.

Yardstick of the comparison with torch: test_optim.TRAJECTORY_ULPS under
test_optim.ulps, the project's CPU bound for the same comparison without
clipping, in spacings at the magnitude max(|initial|, |final|) of each
parameter element, as test_attached_optimizer_matches_torch_20_steps takes
it for a trajectory (test_optim's docstring says why an in-place update is
measured against its operands). Not bitwise: torch takes the total norm as
an fp32 norm of per-tensor fp32 norms, the mirror as the square root of an
fp64 sum of squares, and the two coefficients differ in their last ulps
(from step 2 on; fed torch's own coefficient the optimizers are bitwise
equal to torch). Measured over the cases below: at most 3 ulp (AdamW), 1
(SGD). Measured at the final value's magnitude alone (`ulps` without
`before`, as test_optim._agree calls it for runs that come out bitwise)
SGD stays at 1 but the AdamW runs reach 43: Adam walks one element of the
first weight from -2.7e-3 to -4.8e-5, where an absolute difference of
1.6e-10, under one spacing of its initial value, counts 43 spacings of its
final one.

(The Trainer's engine gate has no CPU-runnable form — off the GPU the toy
engines never engage — so its test is in test_clip_gpu.py.)
"""

import copy
import os

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD
from test_optim import (BETAS, EPS, LR_ADAM, LR_SGD, TRAJECTORY_ULPS, _data,
                        _fused_step, _make, _make_torch, _mlp, _wrap, ulps)

# the seeded MLP's gradient norm stays between 0.5 and 3 over these steps;
# every step asserts that the clip was active
MAX_NORM = 0.05
STEPS = 10


class _WithLoose(nn.Module):
    """The MLP plus one parameter that is NOT handed to DDP: the optimizer
    steps it outside the buckets."""

    def __init__(self):
        super().__init__()
        self.mlp = _mlp()
        self.gain = nn.Parameter(torch.full((5,), 1.5))


# ---------------------------------------------------------------------------
# the op mirrors
# ---------------------------------------------------------------------------
def test_sumsq_slots():
    assert ops.sumsq_slots(0) == 1
    assert ops.sumsq_slots(4) == ops.sumsq_slots(1024) == 1
    assert ops.sumsq_slots(1028) == 2
    assert ops.sumsq_slots(4 * 256 * 2048) == 2048
    assert ops.sumsq_slots(4 * 256 * 2048 + 4) == 2048  # the grid cap
    with pytest.raises(ValueError):
        ops.sumsq_slots(6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mirror_norm_and_coefficient(dtype):
    gen = torch.Generator().manual_seed(51)
    g = torch.randn(4 * (256 * 3 + 17), generator=gen).to(dtype)
    slots = ops.sumsq_slots(g.numel())
    partials = torch.full((slots + 2,), float("nan"), dtype=torch.float64)
    ops.grad_sumsq_flat_(g, partials[1:1 + slots])
    assert partials[0].isnan() and partials[-1].isnan()  # guards untouched
    assert float(partials[1]) == float(g.double().square().sum())
    assert not partials[2:1 + slots].any()
    with pytest.raises(ValueError):
        ops.grad_sumsq_flat_(g, partials[:slots + 1])
    with pytest.raises(ValueError):
        ops.grad_sumsq_flat_(g, partials[1:1 + slots].float())

    state = torch.zeros(2)
    for max_norm in (0.5, 1e30):
        ops.clip_coef_(partials[1:1 + slots], state, max_norm)
        norm = g.double().square().sum().sqrt().float()
        assert torch.equal(state[0], norm)
        want = torch.clamp((norm + 1e-6).reciprocal() * max_norm, max=1.0)
        assert torch.equal(state[1], want)
    assert float(state[1]) == 1.0


def test_mirror_nonfinite_norms():
    state = torch.zeros(2)
    ops.clip_coef_(torch.tensor([float("inf"), 1.0], dtype=torch.float64),
                   state, 1.0)
    assert state[0] == float("inf") and state[1] == 0
    ops.clip_coef_(torch.tensor([float("nan"), 1.0], dtype=torch.float64),
                   state, 1.0)
    assert state[0].isnan() and state[1].isnan()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["plain", "sgd", "adamw"])
def test_mirror_grad_scale_equals_scaling_the_gradient_first(kind, dtype):
    def run(p, g, scale):
        m, v = torch.zeros(p.numel()), torch.zeros(p.numel())
        if kind == "plain":
            ops.sgd_flat_(p, g, LR_SGD, zero_grad=False, grad_scale=scale)
        elif kind == "sgd":
            ops.sgd_momentum_flat_(p, g, m, LR_SGD, 0.9, 1e-2, True,
                                   zero_grad=False, grad_scale=scale)
        else:
            ops.adamw_flat_(p, g, m, v, 1, LR_ADAM, *BETAS, EPS, 1e-2,
                            zero_grad=False, grad_scale=scale)
        return p, m, v

    gen = torch.Generator().manual_seed(52)
    p = torch.randn(1028, generator=gen).to(dtype)
    g = torch.randn(1028, generator=gen).to(dtype)
    s = torch.tensor([0.37])
    g0 = g.clone()
    got = run(p.clone(), g, s)
    assert torch.equal(g, g0), "zero_grad=False leaves the gradient UNSCALED"
    g2 = g.clone()
    g2.mul_(s)  # fp32 multiply, rounded to g's dtype on the store
    want = run(p.clone(), g2, None)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # the scale matters (Adam's first step hides it in p, not in exp_avg)
    unscaled = run(p.clone(), g.clone(), None)
    assert not torch.equal(got[0 if kind == "plain" else 1],
                           unscaled[0 if kind == "plain" else 1])


# ---------------------------------------------------------------------------
# the optimizers against clip_grad_norm_ + torch.optim
# ---------------------------------------------------------------------------
def _run_against_torch(kind, mode):
    data = _data(STEPS)
    if mode == "loose":
        a, b = _WithLoose(), _WithLoose()
        eng = DDP(a.mlp, comm=None, bucket_cap_mb=0.0005)
        fwd_a = lambda x: eng(x) * a.gain  # noqa: E731
        fwd_b = lambda x: b.mlp(x) * b.gain  # noqa: E731
    else:
        a, b = _mlp(), _mlp()
        fwd_b = b
        if mode == "attached":
            eng = DDP(a, comm=None, bucket_cap_mb=0.0005)
            fwd_a = eng
        else:
            eng, fwd_a = None, a
    opt = _make(kind, a.parameters(), max_grad_norm=MAX_NORM)
    assert opt.grad_norm is None and opt.clip_coef is None
    if eng is not None:
        assert len(eng.reducer.buckets) >= 2
        opt.attach_reducer(eng.reducer)
    ref = _make_torch(kind, b.parameters())
    init = [p.detach().clone() for p in b.parameters()]
    for x, t in data:
        if eng is None:
            opt.zero_grad()
        elif mode == "loose":
            a.gain.grad = None  # the attached zero_grad covers buckets only
        nn.functional.mse_loss(fwd_a(x), t).backward()
        if eng is not None:
            eng.finalize_backward()
        opt.step()

        ref.zero_grad()
        nn.functional.mse_loss(fwd_b(x), t).backward()
        norm = torch.nn.utils.clip_grad_norm_(b.parameters(), MAX_NORM)
        ref.step()

        assert float(opt.clip_coef) < 1, "the clip must be active"
        assert opt.grad_norm.dim() == 0 \
            and opt.grad_norm.dtype == torch.float32
        assert float(opt.grad_norm) == pytest.approx(float(norm), rel=1e-5)
    worst = max(ulps(pa, pb, p0) for pa, pb, p0 in
                zip(a.parameters(), b.parameters(), init))
    return a, b, opt, worst


@pytest.mark.parametrize("mode", ["unattached", "attached", "loose"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipped_optimizer_matches_torch(kind, mode):
    a, b, opt, worst = _run_against_torch(kind, mode)
    print(f"[clip] {kind} {mode} vs torch, {STEPS} steps: max {worst} ulp")
    assert worst <= TRAJECTORY_ULPS
    if mode == "loose":
        assert id(a.gain) not in opt._bucketed
        assert not torch.equal(a.gain.detach(), torch.full((5,), 1.5))
    # an unclipped run lands elsewhere: the clip was applied
    c = _mlp()
    plain = _make(kind, c.parameters())
    for x, t in _data(STEPS):
        plain.zero_grad()
        nn.functional.mse_loss(c(x), t).backward()
        plain.step()
    if mode != "loose" and kind == "sgd":  # Adam normalises the scale away
        assert max(ulps(pa, pc) for pa, pc in
                   zip(a.parameters(), c.parameters())) > 100


def test_plain_sgd_clipped_matches_torch():
    """momentum == weight_decay == 0 takes the sgd_flat_ path."""
    a, b = _mlp(), _mlp()
    eng, opt = _wrap("sgd", a, momentum=0, weight_decay=0, nesterov=False,
                     max_grad_norm=MAX_NORM)
    ref = torch.optim.SGD(b.parameters(), lr=LR_SGD, foreach=False)
    init = [p.detach().clone() for p in b.parameters()]
    for x, t in _data(STEPS):
        _fused_step(eng, opt, x, t)
        ref.zero_grad()
        nn.functional.mse_loss(b(x), t).backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), MAX_NORM)
        ref.step()
        assert float(opt.clip_coef) < 1
    assert max(ulps(pa, pb, p0) for pa, pb, p0 in
               zip(a.parameters(), b.parameters(), init)) <= TRAJECTORY_ULPS
    assert not opt._flat_state


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clip_that_never_triggers_changes_nothing(kind):
    a, b = _mlp(), _mlp()
    (eng_a, opt_a) = _wrap(kind, a, max_grad_norm=1e30)
    (eng_b, opt_b) = _wrap(kind, b)
    for x, t in _data(STEPS):
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
        assert float(opt_a.clip_coef) == 1.0
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
    for key, bufs in opt_a._flat_state.items():
        for fa, fb in zip(bufs, opt_b._flat_state[key]):
            assert fa.any() and torch.equal(fa, fb)
    assert opt_b.grad_norm is None and opt_b._clip_partials is None


# ---------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan")])
def test_invalid_max_grad_norm_is_rejected(bad):
    p = [nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedSGD(p, lr=0.1, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW(p, max_grad_norm=bad)
    opt = FusedAdamW(p, max_grad_norm=2.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 2.0
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None


def test_max_grad_norm_is_assignable_between_steps():
    a, b = _mlp(), _mlp()
    eng_a, opt_a = _wrap("sgd", a)
    eng_b, opt_b = _wrap("sgd", b, max_grad_norm=MAX_NORM)
    data = _data(4)
    for x, t in data[:2]:
        _fused_step(eng_a, opt_a, x, t)
    opt_b.max_grad_norm = None
    for x, t in data[:2]:
        _fused_step(eng_b, opt_b, x, t)
    assert opt_b.grad_norm is None
    opt_a.max_grad_norm = opt_b.max_grad_norm = MAX_NORM
    for x, t in data[2:]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    assert float(opt_a.clip_coef) < 1
    assert torch.equal(opt_a.grad_norm, opt_b.grad_norm)
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def _keys(sd):
    return (set(sd), [sorted(g) for g in sd["param_groups"]],
            {k: sorted(st) for k, st in sd["state"].items()})


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_ignores_clipping_and_round_trips_through_torch(kind):
    data = _data(6)
    a, b = _mlp(), _mlp()
    eng_a, opt_a = _wrap(kind, a, max_grad_norm=MAX_NORM)
    eng_b, opt_b = _wrap(kind, b)
    for x, t in data[:3]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    assert _keys(opt_a.state_dict()) == _keys(opt_b.state_dict())
    assert "max_grad_norm" not in opt_a.param_groups[0]

    # clipped fused -> torch.optim -> a fresh clipped fused optimizer
    m_t = _mlp()
    m_t.load_state_dict(a.state_dict())
    opt_t = _make_torch(kind, m_t.parameters())
    opt_t.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    c = _mlp()
    c.load_state_dict(a.state_dict())
    eng_c, opt_c = _wrap(kind, c, max_grad_norm=MAX_NORM)
    opt_c.load_state_dict(copy.deepcopy(opt_t.state_dict()))
    assert opt_c.max_grad_norm == MAX_NORM
    # a load into the running optimizer keeps its clip buffers
    partials, state = opt_a._clip_partials, opt_a._clip_state
    opt_a.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    opt_a.attach_reducer(eng_a.reducer)
    assert opt_a._clip_partials is partials and opt_a._clip_state is state

    start = [p.detach().clone() for p in m_t.parameters()]
    for x, t in data[3:]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_c, opt_c, x, t)
        opt_t.zero_grad()
        nn.functional.mse_loss(m_t(x), t).backward()
        torch.nn.utils.clip_grad_norm_(m_t.parameters(), MAX_NORM)
        opt_t.step()
    for pa, pc, pt, p0 in zip(a.parameters(), c.parameters(),
                              m_t.parameters(), start):
        assert torch.equal(pa, pc)
        assert ulps(pa, pt, p0) <= TRAJECTORY_ULPS


# ---------------------------------------------------------------------------
# gloo, world 2
# ---------------------------------------------------------------------------
WORLD = 2


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clip_worker(rank, kind, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        model = _mlp()
        engine = DDP(model, bucket_cap_mb=0.0005)
        opt = _make(kind, model.parameters(), max_grad_norm=MAX_NORM)
        opt.attach_reducer(engine.reducer)
        norms = []
        for x, t in _data(4):  # 6 rows a batch: 3 per rank
            xs, ts = x[rank * 3:(rank + 1) * 3], t[rank * 3:(rank + 1) * 3]
            nn.functional.mse_loss(engine(xs), ts).backward()
            engine.finalize_backward()
            opt.step()
            norms.append(opt.grad_norm.clone())
            assert float(opt.clip_coef) < 1
        torch.save({"params": [p.detach().clone()
                               for p in model.parameters()],
                    "norms": torch.stack(norms)},
                   os.path.join(out_dir, f"clip{rank}.pt"))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_gloo_world2_ranks_clip_alike(kind, tmp_path):
    """Every rank computes the norm from the same averaged buckets, so no
    collective is needed for the ranks to stay bitwise together."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_clip_worker,
                         args=(r, kind, port, str(tmp_path)))
             for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    got = [torch.load(tmp_path / f"clip{r}.pt", weights_only=True)
           for r in range(WORLD)]
    assert torch.equal(got[0]["norms"], got[1]["norms"])
    assert bool((got[0]["norms"] > MAX_NORM).all())
    for a, b in zip(got[0]["params"], got[1]["params"]):
        assert torch.equal(a, b)
    # and they trained: the full-batch single-process clipped run agrees
    model = _mlp()
    opt = _make(kind, model.parameters(), max_grad_norm=MAX_NORM)
    for x, t in _data(4):
        opt.zero_grad()
        nn.functional.mse_loss(model(x), t).backward()
        opt.step()
    for a, w in zip(got[0]["params"], model.parameters()):
        assert torch.allclose(a, w, atol=1e-6), (a - w).abs().max()
