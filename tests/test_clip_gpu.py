"""GPU tier of the fused global grad-norm clipping: k_sumsq_flat and
k_clip_coef against fp64 host values, the SCALED form of the three update
kernels against scaling the gradient first (bitwise), the attached
optimizers with `max_grad_norm` against torch's clip_grad_norm_ +
torch.optim on the device, non-finite gradients and the Trainer's engine
gate.

(The whole-step graph-capture tests are in test_graph_clip_gpu.py: they
must run BEFORE test_graphed_generic_gpu.py.)

Bound on the total norm, NORM_REL = 2^-20 relative, derived, not measured:
with the grid capped at 2048 blocks of 256 lanes, a lane of k_sumsq_flat
adds at most TERMS_PER_LANE = 8 positive fp32 squares at the sizes below
(two float4 at the largest), each product rounded once and each fp32
addition once; everything after the lane is double, then come one sqrt and
one rounding to fp32. That is under 16 half-ulp roundings of 2^-24 with no
cancellation: 16 * 2^-24 = 2^-20. (With another grid cap the bound scales
as (terms per lane + 4) * 2^-24; test_terms_per_lane_matches_the_grid holds
the 8.)
"""

import functools

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD
from test_optim import BETAS, EPS, LR_ADAM, LR_SGD, seeded
from test_optim_gpu import SIZES, WD, _batches, _mlp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NORM_REL = 2.0 ** -20
TERMS_PER_LANE = 8
DTYPES = [torch.float32, torch.bfloat16]


def _host_coef(norm, max_norm):
    """torch's clip_grad_norm_ formula on the host, in fp32."""
    norm = norm.detach().cpu().reshape(())
    assert norm.dtype == torch.float32
    return torch.clamp((norm + 1e-6).reciprocal() * max_norm, max=1.0)


@functools.lru_cache(maxsize=None)
def _grad(dtype, n, seed=61):
    """-> (the gradient on the host, its fp64 L2 norm)."""
    g = seeded(n, seed, 1)[1].to(dtype)
    return g, float(g.double().square().sum().sqrt())


# ---------------------------------------------------------------------------
# k_sumsq_flat + k_clip_coef
# ---------------------------------------------------------------------------
def test_terms_per_lane_matches_the_grid():
    assert ops.ext().sumsq_slots(max(SIZES)) == 2048
    lanes = 2048 * 256
    assert 4 * -(-(max(SIZES) // 4) // lanes) == TERMS_PER_LANE
    for n in SIZES + [0, 8, 4 * 256 * 2048]:
        assert ops.sumsq_slots(n) == ops.ext().sumsq_slots(n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_and_coefficient(dtype, n):
    g_host, want = _grad(dtype, n)
    g = g_host.to(DEV)
    slots = ops.sumsq_slots(n)
    runs = []
    for _ in range(2):  # every slot is rewritten: NaN in, nothing added up
        buf = torch.full((slots + 2,), float("nan"), dtype=torch.float64,
                         device=DEV)
        state = torch.full((2,), float("nan"), device=DEV)
        seg = buf[1:1 + slots]
        ops.grad_sumsq_flat_(g, seg)
        ops.grad_sumsq_flat_(g, seg)  # a second call into the same slots
        ops.clip_coef_(seg, state, 0.5)
        torch.cuda.synchronize()
        assert buf[0].isnan() and buf[-1].isnan(), "guard slots written"
        assert bool(torch.isfinite(seg).all())
        runs.append((seg.clone(), state.clone()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    seg, state = runs[0]
    assert torch.equal(g, g_host.to(DEV)), "the gradient is only read"

    norm = float(state[0])
    rel = abs(norm - want) / want
    print(f"[clip] {dtype} n={n}: norm {norm!r} fp64 {want!r} "
          f"rel {rel:.3e} (bound {NORM_REL:.3e}), coef {float(state[1])!r}")
    assert rel <= NORM_REL
    assert want > 0.5  # max_norm 0.5 clips
    assert torch.equal(state[1].cpu(), _host_coef(state[0], 0.5))
    assert 0 < float(state[1]) < 1
    # a clip that does not trigger clamps to exactly 1
    ops.clip_coef_(seg, state, 1e30)
    assert float(state[1]) == 1.0 and float(state[0]) == norm
    ops.clip_coef_(seg, state, 3.0 * want)
    assert float(state[1]) == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_buckets_share_one_partials_buffer(dtype):
    n1, n2 = 1028, 4 * (256 * 3 + 17)
    (g1, _), (g2, _) = _grad(dtype, n1, 62), _grad(dtype, n2, 63)
    s1, s2 = ops.sumsq_slots(n1), ops.sumsq_slots(n2)
    buf = torch.full((s1 + s2 + 2,), float("nan"), dtype=torch.float64,
                     device=DEV)
    ops.grad_sumsq_flat_(g1.to(DEV), buf[1:1 + s1])
    assert buf[1 + s1:].isnan().all(), "wrote past its segment"
    ops.grad_sumsq_flat_(g2.to(DEV), buf[1 + s1:1 + s1 + s2])
    state = torch.zeros(2, device=DEV)
    ops.clip_coef_(buf[1:1 + s1 + s2], state, 0.5)
    torch.cuda.synchronize()
    assert buf[0].isnan() and buf[-1].isnan()
    want = float(torch.cat([g1, g2]).double().square().sum().sqrt())
    assert abs(float(state[0]) - want) / want <= NORM_REL
    assert torch.equal(state[1].cpu(), _host_coef(state[0], 0.5))


def test_clip_ops_reject_wrong_buffers():
    g = torch.ones(1028, device=DEV)
    slots = ops.sumsq_slots(1028)
    with pytest.raises((ValueError, RuntimeError)):
        ops.grad_sumsq_flat_(g, torch.zeros(slots - 1, dtype=torch.float64,
                                            device=DEV))
    with pytest.raises(RuntimeError, match="sumsq_slots"):
        ops.ext().grad_sumsq_flat(g, torch.zeros(slots + 1,
                                                 dtype=torch.float64,
                                                 device=DEV))
    with pytest.raises(RuntimeError, match="f64"):
        ops.ext().grad_sumsq_flat(g, torch.zeros(slots, device=DEV))
    with pytest.raises(RuntimeError, match="aligned"):
        ops.ext().grad_sumsq_flat(
            torch.ones(1032, device=DEV)[1:1029],
            torch.zeros(slots, dtype=torch.float64, device=DEV))
    part = torch.zeros(slots, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="clip_state"):
        ops.ext().clip_coef(part, torch.zeros(1, device=DEV), 1.0)
    p = torch.ones(1028, device=DEV)
    for bad in (torch.ones(2, device=DEV), torch.ones(1),
                torch.ones(1, dtype=torch.float64, device=DEV)):
        with pytest.raises(RuntimeError, match="grad_scale"):
            ops.ext().sgd_flat(p, g, 0.5, True, bad)
    torch.cuda.synchronize()
    assert bool((p == 1).all()) and bool((g == 1).all())  # nothing ran


# ---------------------------------------------------------------------------
# the scale folded into the update kernels: bitwise
# ---------------------------------------------------------------------------
SCALES = [0.37, 1.0, 2.0 ** -130]  # active, identity, subnormal products


def _update(op, p, g, m, v, zero, scale):
    """One update on clones of the inputs -> (p, g, state...) after it."""
    p, g, m, v = p.clone(), g.clone(), m.clone(), v.clone()
    if op == "plain":
        ops.sgd_flat_(p, g, LR_SGD, zero_grad=zero, grad_scale=scale)
        return p, g
    if op == "sgd":
        ops.sgd_momentum_flat_(p, g, m, LR_SGD, 0.9, WD, True,
                               zero_grad=zero, grad_scale=scale)
        return p, g, m
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=DEV)
    ops.adamw_tick_(state, LR_ADAM, *BETAS)  # -> t = 2
    ops.adamw_flat_(p, g, m, v, state, LR_ADAM, *BETAS, EPS, WD, None,
                    zero_grad=zero, grad_scale=scale)
    return p, g, m, v


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["plain", "sgd", "adamw"])
def test_folded_scale_equals_scaling_the_gradient_first(op, dtype, n):
    p, g, m, v = (x.to(DEV) for x in seeded(n, 64, 2))
    p, g = p.to(dtype), g.to(dtype)
    for s in SCALES:
        scale = torch.tensor([s], dtype=torch.float32, device=DEV)
        assert float(scale) != 0
        g2 = g.clone()
        # grad.mul_(coef) with the fp32 coefficient: one fp32 multiply,
        # for bf16 rounded on the store. (A 0-dim coefficient would be
        # cast to bf16 FIRST by torch's type promotion.)
        g2.mul_(scale)
        if s == 1.0:
            assert torch.equal(g2, g)
        elif s < 1e-30 and dtype == torch.float32:
            assert g2.any() and bool((g2.abs() < 2.0 ** -126).all())
        for zero in (True, False):
            got = _update(op, p, g, m, v, zero, scale)
            want = _update(op, p, g2, m, v, zero, None)
            names = ("p", "g", "m", "v")
            for name, a, b in zip(names, got, want):
                if name == "g":
                    continue
                assert torch.equal(a, b), (op, s, zero, name,
                                           (a.float() - b.float()).abs().max())
            if zero:
                assert not got[1].any(), "zero_grad must clear the gradient"
            else:
                assert torch.equal(got[1], g), \
                    "zero_grad=False leaves the gradient UNSCALED"
            if s == 1.0:  # the SCALED kernel at 1 is the unscaled kernel
                plain = _update(op, p, g, m, v, zero, None)
                assert all(torch.equal(a, b) for a, b in zip(got, plain))
            elif s == 0.37:
                plain = _update(op, p, g, m, v, zero, None)
                moved = got[0] if op == "plain" else got[2]
                assert not torch.equal(moved,
                                       plain[0] if op == "plain" else plain[2])


# ---------------------------------------------------------------------------
# attached optimizers vs clip_grad_norm_ + torch.optim on the device
# ---------------------------------------------------------------------------
STEPS = 20
# the MLP's gradient norm stays above 0.2 over the 20 steps (asserted)
MAX_NORM = 0.05


def _fused(kind, model, **kw):
    eng = DDP(model, comm=None, bucket_cap_mb=0.05)
    assert len(eng.reducer.buckets) >= 3
    if kind == "sgd":
        opt = FusedSGD(model.parameters(), lr=LR_SGD, momentum=0.9,
                       weight_decay=WD, nesterov=True, **kw)
    else:
        opt = FusedAdamW(model.parameters(), lr=LR_ADAM, betas=BETAS, eps=EPS,
                         weight_decay=WD, **kw)
    opt.attach_reducer(eng.reducer)
    return eng, opt


def _torch_opt(kind, params):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=LR_SGD, momentum=0.9,
                               weight_decay=WD, nesterov=True, foreach=False)
    return torch.optim.AdamW(params, lr=LR_ADAM, betas=BETAS, eps=EPS,
                             weight_decay=WD, foreach=False)


def _fused_step(eng, opt, x, t):
    nn.functional.mse_loss(eng(x), t).backward()
    eng.finalize_backward()
    opt.step()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_attached_clipped_optimizer_matches_torch_20_steps(kind):
    """Oracle: clip_grad_norm_ + torch.optim on the device in fp32, and the
    same in fp64. Not bitwise — the two fp32 total norms differ in their
    last ulps — so both fp32 runs are held against the fp64 trajectory:
    max|ours - fp64| <= 2 * max|torch_fp32 - fp64| over all parameters.
    Measured on MI355X (profiles/README.md §r06a): max|ours - fp64| and
    max|torch_fp32 - fp64| are both 6.900e-08 for SGD and both 2.078e-06
    for AdamW (on these inputs the two fp32 norms round alike, and the
    runs coincide); step-1 `grad_norm` is 1.03e-08 relative from fp64."""
    m_a, m_b, m_c = _mlp(), _mlp(), _mlp().double()
    eng, opt = _fused(kind, m_a, max_grad_norm=MAX_NORM)
    assert opt.grad_norm is None
    ref32, ref64 = _torch_opt(kind, m_b.parameters()), \
        _torch_opt(kind, m_c.parameters())
    for step, (x, t) in enumerate(_batches(STEPS)):
        _fused_step(eng, opt, x, t)
        norms = []
        for mod, ref, cast in ((m_b, ref32, torch.float32),
                               (m_c, ref64, torch.float64)):
            ref.zero_grad()
            nn.functional.mse_loss(mod(x.to(cast)), t.to(cast)).backward()
            norms.append(torch.nn.utils.clip_grad_norm_(
                mod.parameters(), MAX_NORM, foreach=False))
            ref.step()
        assert float(opt.clip_coef) < 1, "the clip must be active"
        assert float(norms[0]) > MAX_NORM and float(norms[1]) > MAX_NORM
        if step == 0:  # the trajectories have not diverged yet
            assert opt.grad_norm.dtype == torch.float32 \
                and opt.grad_norm.dim() == 0
            rel = abs(float(opt.grad_norm) - float(norms[1])) \
                / float(norms[1])
            print(f"[clip] {kind} step-1 grad_norm rel to fp64: {rel:.3e}")
            assert rel <= NORM_REL
    torch.cuda.synchronize()
    ours = max(float((a.double() - c).abs().max())
               for a, c in zip(m_a.parameters(), m_c.parameters()))
    theirs = max(float((b.double() - c).abs().max())
                 for b, c in zip(m_b.parameters(), m_c.parameters()))
    print(f"[clip] attached {kind}, {STEPS} clipped steps: max|ours-fp64| "
          f"{ours:.3e}, max|torch_fp32-fp64| {theirs:.3e}")
    assert ours <= 2 * theirs
    assert all(not fg.any() for _, fg in opt._flat_pairs)
    # the clip was applied: an unclipped run is orders of magnitude away
    if kind == "sgd":
        m_d = _mlp()
        eng_d, opt_d = _fused(kind, m_d)
        for x, t in _batches(STEPS):
            _fused_step(eng_d, opt_d, x, t)
        away = max(float((d.double() - c).abs().max())
                   for d, c in zip(m_d.parameters(), m_c.parameters()))
        assert away > 1000 * max(theirs, 1e-9)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_never_active_clip_changes_nothing_20_steps(kind):
    m_a, m_b = _mlp(), _mlp()
    eng_a, opt_a = _fused(kind, m_a, max_grad_norm=1e30)
    eng_b, opt_b = _fused(kind, m_b)
    for x, t in _batches(STEPS):
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    torch.cuda.synchronize()
    assert float(opt_a.clip_coef) == 1.0 and float(opt_a.grad_norm) > 0
    assert opt_b.grad_norm is None and opt_b._clip_partials is None
    for a, b in zip(m_a.parameters(), m_b.parameters()):
        assert torch.equal(a, b)
    assert opt_a._flat_state.keys() == opt_b._flat_state.keys()
    for key, bufs in opt_a._flat_state.items():
        for a, b in zip(bufs, opt_b._flat_state[key]):
            assert a.any() and torch.equal(a, b)
    if kind == "adamw":
        assert int(opt_a._step_state[0]) == int(opt_b._step_state[0]) == STEPS


@pytest.mark.parametrize("bad", ["inf", "nan"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_nonfinite_gradient_behaves_as_torch(kind, bad):
    m = _mlp()
    eng, opt = _fused(kind, m, max_grad_norm=1.0)
    x, t = _batches(1)[0]
    nn.functional.mse_loss(eng(x), t).backward()
    eng.finalize_backward()
    opt._flat_pairs[1][1][5] = float(bad)  # one element of one bucket
    opt.step()
    torch.cuda.synchronize()
    if bad == "inf":
        assert float(opt.grad_norm) == float("inf")
        assert float(opt.clip_coef) == 0.0
        # inf * 0 = NaN at the offending element and nowhere else
        nans = sum(int(fp.isnan().sum()) for fp, _ in opt._flat_pairs)
        assert nans == 1 and bool(opt._flat_pairs[1][0][5].isnan())
    else:
        assert bool(opt.grad_norm.isnan()) and bool(opt.clip_coef.isnan())


def test_clip_buffers_survive_reattach_and_load_state_dict():
    import copy
    m = _mlp()
    eng, opt = _fused("adamw", m, max_grad_norm=MAX_NORM)
    x, t = _batches(1)[0]
    _fused_step(eng, opt, x, t)
    partials, state = opt._clip_partials, opt._clip_state
    assert partials.dtype == torch.float64 and partials.numel() == 1 + sum(
        ops.sumsq_slots(fg.numel()) for _, fg in opt._flat_pairs)
    assert float(partials[-1]) == 0.0  # no loose parameter
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    opt.attach_reducer(eng.reducer)
    _fused_step(eng, opt, x, t)
    assert opt._clip_partials is partials and opt._clip_state is state
    assert opt.grad_norm.data_ptr() == state.data_ptr()


def test_trainer_keeps_clipped_sgd_off_the_toy_engines(tmp_path):
    """engine="auto" must not hand a clipping optimizer to the toy kernels
    (they apply p -= lr*g only). 5 steps then match clip_grad_norm_ +
    torch.optim.SGD on an identical nn.Linear.

    Tolerance: HipLinear's forward differs from nn.Linear's by fp32
    accumulation order, |dy| <= K*eps*|x||w| with K = 20, |x|,|w| < 1, so a
    gradient element (2/B * sum dy*x) is off by d <= 2*K*eps ~ 4.8e-6. A
    clipped element is c_i = g_i * max_norm / |g| with |g| >= max_norm
    (asserted), so its error is at most d * max_norm/|g| <= d from g_i plus
    (|g_i|/|g|) * (max_norm/|g|) * |delta |g|| <= sqrt(21) * d from the norm
    of the 21 gradient elements. 5 steps of lr = 1e-3:
    atol = 1e-3 * 5 * (1 + sqrt(21)) * 4.8e-6 = 1.3e-7."""
    from mi355x_ddp.data import ToyDataset, prepare_dataloader
    from mi355x_ddp.models import toy_model
    from mi355x_ddp.trainer import Trainer

    lr, max_norm = 1e-3, 0.1
    torch.manual_seed(4)
    model = toy_model(20, 1)
    twin = nn.Linear(20, 1)
    twin.load_state_dict(model.state_dict())
    twin.to(DEV)
    plain = nn.Linear(20, 1).to(DEV)
    plain.load_state_dict(twin.state_dict())
    ds = ToyDataset(160, seed=6)
    loader = prepare_dataloader(ds, 32, shuffle=False)
    tr = Trainer(model, loader,
                 FusedSGD(model.parameters(), lr, max_grad_norm=max_norm),
                 gpu_id=0, save_every=10 ** 9, loss_fn="mse", engine="auto",
                 checkpoint_path=str(tmp_path / "c.pt"))
    assert tr._engine is None, "a clipping optimizer must stay on hooks"
    tr.train(1)
    assert float(tr.optimizer.clip_coef) < 1

    ref = torch.optim.SGD(twin.parameters(), lr=lr)
    ref_plain = torch.optim.SGD(plain.parameters(), lr=lr)
    for i in range(5):
        x = ds.inputs[i * 32:(i + 1) * 32].to(DEV)
        t = ds.targets[i * 32:(i + 1) * 32].to(DEV)
        for mod, o, clip in ((twin, ref, True), (plain, ref_plain, False)):
            o.zero_grad()
            nn.functional.mse_loss(mod(x), t).backward()
            if clip:
                norm = torch.nn.utils.clip_grad_norm_(mod.parameters(),
                                                      max_norm)
                assert float(norm) > max_norm
            o.step()
    torch.cuda.synchronize()
    atol = lr * 5 * (1 + 21 ** 0.5) * (2 * 20 * 2.0 ** -23)
    got = tr._unwrapped()
    assert torch.allclose(got.weight, twin.weight, rtol=0, atol=atol)
    assert torch.allclose(got.bias, twin.bias, rtol=0, atol=atol)
    # unclipped SGD lands visibly elsewhere: the clip was applied
    assert (got.weight - plain.weight).abs().max() > 100 * atol

    # the unclipped optimizer still qualifies for the toy engine
    m2 = toy_model(20, 1)
    tr2 = Trainer(m2, loader, FusedSGD(m2.parameters(), lr), gpu_id=0,
                  save_every=10 ** 9, loss_fn="mse", engine="auto",
                  checkpoint_path=str(tmp_path / "c2.pt"))
    assert tr2._engine is not None
