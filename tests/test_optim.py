"""CPU tier of the flat-bucket optimizers (FusedSGD with momentum /
weight decay / nesterov, FusedAdamW): the plain-torch mirrors in
mi355x_ddp.ops against torch.optim, state_dict interchange with torch.optim,
the no-decay mask, bucket padding, constructor errors and Trainer snapshots.

How differences are measured (`ulps`): in units of the fp32 spacing at the
element's magnitude. Every output checked here is an in-place update
x_new = x_old + delta, so the element's magnitude is taken as
max(|x_old|, |x_new|): where x_old and delta cancel, |x_new| alone can be
orders of magnitude below both operands, and a difference of ONE rounding
in delta — which any two correct implementations may have — is then an
unbounded number of spacings of |x_new|. Measured against the operands it
is what the bounds below mean it to be: a count of roundings.

Bounds (from the issue that introduced these optimizers): <= 2 ulp for one
step from identical state, <= 8 ulp after a 200-step trajectory. The mirrors
issue torch's own operation sequence, so on one machine they come out
bitwise equal to torch.optim; the bounds leave room for a torch build whose
foreach=False path orders an operation differently.
"""

import copy
import os

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.parallel import DDP, FlatBucketOptimizer, FusedAdamW, FusedSGD

ONE_STEP_ULPS = 2
TRAJECTORY_ULPS = 8
LR_ADAM, LR_SGD = 1e-3, 1e-2
BETAS, EPS = (0.9, 0.999), 1e-8


def ulps(got, ref, before=None, mant_bits=23):
    """max |got - ref| in spacings (mant_bits of mantissa: 23 fp32, 7 bf16)
    at the element's magnitude max(|ref|, |before|) — see the module
    docstring. Magnitudes below the smallest normal count as that."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    mag = ref.abs()
    if before is not None:
        mag = torch.maximum(mag, before.detach().double().cpu().abs())
    mag = mag.clamp_min(2.0 ** -126)
    _, e = torch.frexp(mag)  # mag = m * 2^e, m in [0.5, 1)
    spacing = torch.ldexp(torch.ones_like(mag), e - 1 - mant_bits)
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / spacing).max())


def ulps_strict(got, ref, before, mant_bits=23):
    """The literal yardstick — spacings at the OUTPUT's own magnitude |ref|
    — over the elements where the update did not cancel: |ref| >=
    |before| / 2. There it is a fair scale (at most a factor 2 from the
    operands'), so the same bounds are asserted under it."""
    keep = ref.detach().double().cpu().abs() >= \
        before.detach().double().cpu().abs() / 2
    return ulps(got.detach().cpu()[keep], ref.detach().cpu()[keep],
                mant_bits=mant_bits)


def seeded(n, seed, t):
    """p, g ~ N(0,1); the state a run would have before step t: zero at
    t == 1, otherwise a first moment ~ N(0, 0.1) and a positive second."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    if t == 1:
        m.zero_()
        v.zero_()
    return p, g, m, v


def torch_param(p, g):
    q = nn.Parameter(p.clone())
    q.grad = g.clone()
    return q


# ---------------------------------------------------------------------------
# mirror vs torch.optim (foreach=False)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, 100003])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_mirror_one_step_matches_torch(n, t, wd, nesterov):
    p, g, buf, _ = seeded(n, 11, t)
    q = torch_param(p, g)
    ref = torch.optim.SGD([q], lr=LR_SGD, momentum=0.9, weight_decay=wd,
                          nesterov=nesterov, foreach=False)
    if t > 1:
        ref.state[q]["momentum_buffer"] = buf.clone()
    ref.step()

    p0, g0 = p.clone(), g.clone()
    ops.sgd_momentum_flat_(p, g, buf, LR_SGD, 0.9, wd, nesterov,
                           zero_grad=False)
    assert torch.equal(g, g0)
    assert ulps(p, q, p0) <= ONE_STEP_ULPS
    assert ulps_strict(p, q, p0) <= ONE_STEP_ULPS
    assert ulps(buf, ref.state[q]["momentum_buffer"]) <= ONE_STEP_ULPS


@pytest.mark.parametrize("n", [4, 1028, 100003])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-2, 0.1])
def test_adamw_mirror_one_step_matches_torch(n, t, wd):
    p, g, m, v = seeded(n, 12, t)
    q = torch_param(p, g)
    ref = torch.optim.AdamW([q], lr=LR_ADAM, betas=BETAS, eps=EPS,
                            weight_decay=wd, foreach=False)
    ref.state[q] = {"step": torch.tensor(float(t - 1)),
                    "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    ref.step()

    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    ops.adamw_flat_(p, g, m, v, t, LR_ADAM, *BETAS, EPS, wd, zero_grad=True)
    assert not g.any()
    assert ulps(p, q, p0) <= ONE_STEP_ULPS
    assert ulps_strict(p, q, p0) <= ONE_STEP_ULPS
    assert ulps(m, ref.state[q]["exp_avg"], m0) <= ONE_STEP_ULPS
    assert ulps(v, ref.state[q]["exp_avg_sq"], v0) <= ONE_STEP_ULPS


@pytest.mark.parametrize("n", [4, 1028, 100003])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_mirror_200_step_trajectory_matches_torch(n, kind):
    p, _, m, v = seeded(n, 13, 1)
    q = nn.Parameter(p.clone())
    if kind == "sgd":
        ref = torch.optim.SGD([q], lr=LR_SGD, momentum=0.9,
                              weight_decay=1e-2, nesterov=True, foreach=False)
    else:
        ref = torch.optim.AdamW([q], lr=LR_ADAM, betas=BETAS, eps=EPS,
                                weight_decay=1e-2, foreach=False)
    gen = torch.Generator().manual_seed(14)
    worst = 0.0
    for t in range(1, 201):
        g = torch.randn(n, generator=gen)
        q.grad = g.clone()
        before = q.detach().clone()
        ref.step()
        if kind == "sgd":
            ops.sgd_momentum_flat_(p, g, m, LR_SGD, 0.9, 1e-2, True)
        else:
            ops.adamw_flat_(p, g, m, v, t, LR_ADAM, *BETAS, EPS, 1e-2)
        worst = max(worst, ulps(p, q, before))
    assert worst <= TRAJECTORY_ULPS


def test_mirror_bf16_rounds_once_and_keeps_fp32_state():
    p, g, m, v = seeded(1028, 15, 2)
    pb, gb = p.bfloat16(), g.bfloat16()
    want_p, want_m, want_v = pb.float(), m.clone(), v.clone()
    ops.adamw_flat_(want_p, gb.float(), want_m, want_v, 2, LR_ADAM, *BETAS,
                    EPS, 1e-2, zero_grad=False)
    ops.adamw_flat_(pb, gb, m, v, 2, LR_ADAM, *BETAS, EPS, 1e-2)
    assert pb.dtype == torch.bfloat16 and m.dtype == v.dtype == torch.float32
    assert torch.equal(pb, want_p.bfloat16())
    assert torch.equal(m, want_m) and torch.equal(v, want_v)
    assert not gb.any()


# ---------------------------------------------------------------------------
# the optimizers over DDP's flat buckets
# ---------------------------------------------------------------------------
def _mlp(seed=0):
    # no size is a multiple of 4: every parameter is followed by padding
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(7, 33), nn.ReLU(), nn.Linear(33, 13),
                         nn.ReLU(), nn.Linear(13, 5))


def _data(k, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(6, 7, generator=gen), torch.randn(6, 5, generator=gen))
            for _ in range(k)]


def _make(kind, params, **over):
    if kind == "sgd":
        kw = dict(lr=LR_SGD, momentum=0.9, weight_decay=1e-2, nesterov=True)
        kw.update(over)
        return FusedSGD(params, **kw)
    kw = dict(lr=LR_ADAM, betas=BETAS, eps=EPS, weight_decay=1e-2)
    kw.update(over)
    return FusedAdamW(params, **kw)


def _make_torch(kind, params):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=LR_SGD, momentum=0.9,
                               weight_decay=1e-2, nesterov=True,
                               foreach=False)
    return torch.optim.AdamW(params, lr=LR_ADAM, betas=BETAS, eps=EPS,
                             weight_decay=1e-2, foreach=False)


def _wrap(kind, model, **over):
    eng = DDP(model, comm=None, bucket_cap_mb=0.0005)
    assert len(eng.reducer.buckets) >= 2
    opt = _make(kind, model.parameters(), **over)
    opt.attach_reducer(eng.reducer)
    return eng, opt


def _fused_step(eng, opt, x, t):
    nn.functional.mse_loss(eng(x), t).backward()
    eng.finalize_backward()
    opt.step()


def _torch_step(model, opt, x, t):
    opt.zero_grad()
    nn.functional.mse_loss(model(x), t).backward()
    opt.step()


def _agree(a, b, bound=TRAJECTORY_ULPS):
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert ulps(pa, pb) <= bound


def _inside(view, flat):
    lo = flat.data_ptr()
    return lo <= view.data_ptr() < lo + flat.numel() * flat.element_size()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_attached_optimizer_matches_torch(kind):
    m_a, m_b = _mlp(), _mlp()
    eng, opt = _wrap(kind, m_a)
    ref = _make_torch(kind, m_b.parameters())
    for x, t in _data(6):
        _fused_step(eng, opt, x, t)
        _torch_step(m_b, ref, x, t)
    _agree(m_a, m_b)
    assert isinstance(opt, FlatBucketOptimizer)
    assert all(not fg.any() for _, fg in opt._flat_pairs)  # zeroing folded


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_interchanges_with_torch(kind):
    key = "momentum_buffer" if kind == "sgd" else "exp_avg"
    data = _data(6)
    m_a = _mlp()
    eng_a, opt_a = _wrap(kind, m_a)
    for x, t in data[:3]:
        _fused_step(eng_a, opt_a, x, t)

    # fused -> torch.optim
    m_b = _mlp()
    m_b.load_state_dict(m_a.state_dict())
    opt_b = _make_torch(kind, m_b.parameters())
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    # torch.optim -> a fresh fused optimizer ("and back")
    m_c = _mlp()
    m_c.load_state_dict(m_a.state_dict())
    eng_c, opt_c = _wrap(kind, m_c, lr=0.5)  # hyper-parameters load too
    opt_c.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    # fused -> fused round trip, in place
    opt_a.load_state_dict(copy.deepcopy(opt_a.state_dict()))

    for opt in (opt_a, opt_c):
        flats = opt._flat_state[key]
        for p in opt.param_groups[0]["params"]:
            st = opt.state[p][key]
            assert st.dtype == torch.float32
            assert any(_inside(st, f) for f in flats), \
                "load_state_dict detached the state from the flat buffer"
    if kind == "adamw":
        assert int(opt_a._step_state[0]) == int(opt_c._step_state[0]) == 3
        p0 = opt_c.param_groups[0]["params"][0]
        assert int(opt_c.state[p0]["step"]) == 3
        assert float(opt_a.state_dict()["state"][0]["step"]) == 3.0

    for x, t in data[3:]:
        _fused_step(eng_a, opt_a, x, t)
        _torch_step(m_b, opt_b, x, t)
        _fused_step(eng_c, opt_c, x, t)
    _agree(m_a, m_b)
    _agree(m_c, m_b)


def test_state_loaded_before_attach_moves_into_the_flat_buffers():
    # the Trainer restores a snapshot BEFORE the DDP wrap
    data = _data(4)
    m_a = _mlp()
    eng_a, opt_a = _wrap("adamw", m_a)
    for x, t in data[:2]:
        _fused_step(eng_a, opt_a, x, t)
    m_b = _mlp()
    m_b.load_state_dict(m_a.state_dict())
    opt_b = _make("adamw", m_b.parameters())
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    eng_b = DDP(m_b, comm=None, bucket_cap_mb=0.0005)
    opt_b.attach_reducer(eng_b.reducer)
    for x, t in data[2:]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    for pa, pb in zip(m_a.parameters(), m_b.parameters()):
        assert torch.equal(pa, pb)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_bf16_state_dict_round_trip_keeps_fp32_state(kind):
    """torch's loader casts state to the parameter dtype; for bf16
    parameters that would round the fp32 state to bf16. A round trip must
    return every state tensor bit for bit, in the SAME flat buffers (a
    captured graph updates those), and training must go on as if nothing
    had happened."""
    data = [(x.bfloat16(), t.bfloat16()) for x, t in _data(5)]
    m_a, m_b = _mlp().bfloat16(), _mlp().bfloat16()
    (eng_a, opt_a), (eng_b, opt_b) = _wrap(kind, m_a), _wrap(kind, m_b)
    for x, t in data[:3]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    before = {k: [f.clone() for f in fs] for k, fs in opt_a._flat_state.items()}
    ptrs = {k: [f.data_ptr() for f in fs] for k, fs in opt_a._flat_state.items()}
    assert any((f != f.bfloat16().float()).any()
               for fs in before.values() for f in fs), \
        "state must hold more than bf16 precision or the check shows nothing"
    opt_a.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    for k, fs in opt_a._flat_state.items():
        assert [f.data_ptr() for f in fs] == ptrs[k], "flat buffers replaced"
        for f, f0 in zip(fs, before[k]):
            assert f.dtype == torch.float32 and torch.equal(f, f0)
    for p in opt_a.param_groups[0]["params"]:
        for k in opt_a._state_keys:
            assert any(_inside(opt_a.state[p][k], f)
                       for f in opt_a._flat_state[k])
    for x, t in data[3:]:
        _fused_step(eng_a, opt_a, x, t)
        _fused_step(eng_b, opt_b, x, t)
    for pa, pb in zip(m_a.parameters(), m_b.parameters()):
        assert pa.dtype == torch.bfloat16 and torch.equal(pa, pb)
    # a torch.optim state (bf16 there) loads too, widened to fp32
    m_c = _mlp().bfloat16()
    ref = _make_torch(kind, m_c.parameters())
    for x, t in data[:2]:
        _torch_step(m_c, ref, x, t)
    opt_b.load_state_dict(ref.state_dict())
    key = opt_b._state_keys[0]
    for p, q in zip(opt_b.param_groups[0]["params"], m_c.parameters()):
        assert opt_b.state[p][key].dtype == torch.float32
        assert torch.equal(opt_b.state[p][key], ref.state[q][key].float())


def test_momentum_raised_after_attach_gets_its_buffers():
    m_a, m_b = _mlp(), _mlp()
    eng, opt = _wrap("sgd", m_a, momentum=0, nesterov=False)
    ref = torch.optim.SGD(m_b.parameters(), lr=LR_SGD, weight_decay=1e-2,
                          foreach=False)
    data = _data(4)
    for x, t in data[:2]:
        _fused_step(eng, opt, x, t)
        _torch_step(m_b, ref, x, t)
    opt.param_groups[0]["momentum"] = 0.9
    ref.param_groups[0]["momentum"] = 0.9
    for x, t in data[2:]:
        _fused_step(eng, opt, x, t)
        _torch_step(m_b, ref, x, t)
    _agree(m_a, m_b)
    assert len(opt.state_dict()["state"]) == 6


def test_default_fused_sgd_is_stateless():
    m = _mlp()
    eng = DDP(m, comm=None, bucket_cap_mb=0.0005)
    opt = FusedSGD(m.parameters(), lr=1e-2)
    opt.attach_reducer(eng.reducer)
    for x, t in _data(2):
        _fused_step(eng, opt, x, t)
    assert opt.state_dict()["state"] == {}
    assert not opt._flat_state and len(opt.state) == 0


def test_weight_decay_alone_allocates_no_buffer():
    m_a, m_b = _mlp(), _mlp()
    eng, opt = _wrap("sgd", m_a, momentum=0, nesterov=False)
    ref = torch.optim.SGD(m_b.parameters(), lr=LR_SGD, weight_decay=1e-2,
                          foreach=False)
    for x, t in _data(3):
        _fused_step(eng, opt, x, t)
        _torch_step(m_b, ref, x, t)
    _agree(m_a, m_b)
    assert opt.state_dict()["state"] == {}


def test_constructor_errors():
    p = [nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="dampening"):
        FusedSGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedSGD(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):  # as torch does
        torch.optim.SGD(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=-1.0)
    with pytest.raises(ValueError):
        FusedAdamW(p, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="eps"):  # 0/0 in the zero padding
        FusedAdamW(p, eps=0.0)
    two = FusedAdamW([{"params": [p[0]]},
                      {"params": [nn.Parameter(torch.zeros(4))]}])
    m = _mlp()
    with pytest.raises(ValueError, match="single"):
        two.attach_reducer(DDP(m, comm=None).reducer)
    # a torch state_dict with dampening does not load
    q = [nn.Parameter(torch.zeros(4))]
    damp = torch.optim.SGD(q, lr=0.1, momentum=0.9, dampening=0.5)
    with pytest.raises(ValueError, match="dampening"):
        FusedSGD(q, lr=0.1, momentum=0.9).load_state_dict(damp.state_dict())


def test_no_decay_params_mask():
    wd = 0.1
    m_a, m_b = _mlp(), _mlp()
    biases = [p for n, p in m_a.named_parameters() if n.endswith("bias")]
    eng, opt = _wrap("adamw", m_a, weight_decay=wd, no_decay_params=biases)
    assert opt._decay_masks is not None
    assert all(mk.dtype == torch.uint8 and mk.numel() * 4 == fp.numel()
               for mk, (fp, _) in zip(opt._decay_masks, opt._flat_pairs))
    ref = torch.optim.AdamW(
        [{"params": [p for n, p in m_b.named_parameters()
                     if not n.endswith("bias")], "weight_decay": wd},
         {"params": [p for n, p in m_b.named_parameters()
                     if n.endswith("bias")], "weight_decay": 0.0}],
        lr=LR_ADAM, betas=BETAS, eps=EPS, foreach=False)
    # a run that decays everything must differ, or the check shows nothing
    m_c = _mlp()
    eng_c, opt_c = _wrap("adamw", m_c, weight_decay=wd)
    for x, t in _data(4):
        _fused_step(eng, opt, x, t)
        _torch_step(m_b, ref, x, t)
        _fused_step(eng_c, opt_c, x, t)
    _agree(m_a, m_b)
    assert not torch.equal(m_a[0].bias, m_c[0].bias)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_padding_stays_zero(kind):
    m = _mlp()
    eng, opt = _wrap(kind, m)
    for x, t in _data(5):
        _fused_step(eng, opt, x, t)
    padded = 0
    for bi, b in enumerate(eng.reducer.buckets):
        pad = torch.ones(b.numel, dtype=torch.bool)
        for off, p in zip(b.offsets, b.params):
            pad[off:off + p.numel()] = False
        padded += int(pad.sum())
        flats = [b.flat_param, b.flat_grad] + \
            [bufs[bi] for bufs in opt._flat_state.values()]
        assert len(flats) == (3 if kind == "sgd" else 4)
        for f in flats:
            assert not f[pad].any()
            assert f.dtype == torch.float32
    assert padded > 0


def test_unattached_optimizers_match_torch():
    for kind in ("sgd", "adamw"):
        m_a, m_b = _mlp(), _mlp()
        opt, ref = _make(kind, m_a.parameters()), \
            _make_torch(kind, m_b.parameters())
        for x, t in _data(4):
            _torch_step(m_a, opt, x, t)
            _torch_step(m_b, ref, x, t)
        _agree(m_a, m_b)


# ---------------------------------------------------------------------------
# Trainer snapshots
# ---------------------------------------------------------------------------
@pytest.fixture
def world1():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29791")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _trainer(make_opt, snapshot_path, wrap):
    from mi355x_ddp.data import ToyDataset, prepare_dataloader
    from mi355x_ddp.trainer import Trainer
    torch.manual_seed(5)
    model = nn.Sequential(nn.Linear(20, 9), nn.ReLU(), nn.Linear(9, 1))
    loader = prepare_dataloader(ToyDataset(96, seed=2), 32, shuffle=False)
    return Trainer(model, loader, make_opt(model.parameters()), "cpu", 1,
                   snapshot_path=snapshot_path, loss_fn="mse", wrap_ddp=wrap,
                   bucket_cap_mb=0.0005,
                   checkpoint_path=os.path.join(
                       os.path.dirname(snapshot_path), "ckpt.pt"))


@pytest.mark.parametrize("wrap", [True, False])
def test_trainer_snapshot_resume_equals_uninterrupted(tmp_path, world1, wrap):
    """The snapshot written after epoch k carries EPOCHS_RUN = k and the
    resume loop starts AT that epoch (the reference's convention), so a run
    of k+1 epochs resumed to max_epochs N trains (k+1) + (N-k) = N+1 epochs
    in all. Every epoch sees the same batches (shuffle=False), so that
    equals an uninterrupted N+1-epoch run exactly — provided the Adam
    moments and the step count came back with the snapshot."""
    def make(params):
        return FusedAdamW(params, lr=1e-2, weight_decay=1e-2)

    k, N = 1, 3
    snap = str(tmp_path / "snapshot.pt")
    first = _trainer(make, snap, wrap)
    assert (first.optimizer._flat_pairs is not None) == wrap
    first.train(k + 1)
    payload = torch.load(snap, weights_only=True)
    assert set(payload) == {"MODEL_STATE", "EPOCHS_RUN", "OPTIMIZER_STATE"}
    assert payload["EPOCHS_RUN"] == k

    resumed = _trainer(make, snap, wrap)
    assert resumed.epochs_run == k
    assert int(resumed.optimizer._step_state[0]) == 3 * (k + 1)
    resumed.train(N)

    whole = _trainer(make, str(tmp_path / "other.pt"), wrap)
    whole.train(N + 1)
    for a, b in zip(resumed._unwrapped().parameters(),
                    whole._unwrapped().parameters()):
        assert torch.equal(a, b)
    # without the optimizer state the resumed run would NOT match
    lost = _trainer(make, str(tmp_path / "none.pt"), wrap)
    lost._unwrapped().load_state_dict(payload["MODEL_STATE"])
    lost.epochs_run = k
    lost.train(N)
    assert not all(torch.equal(a, b) for a, b in zip(
        lost._unwrapped().parameters(), whole._unwrapped().parameters()))


def test_trainer_snapshot_of_stateless_optimizer_keeps_two_keys(tmp_path,
                                                                world1):
    snap = str(tmp_path / "snapshot.pt")
    tr = _trainer(lambda ps: FusedSGD(ps, lr=1e-2), snap, True)
    tr.train(2)
    payload = torch.load(snap, weights_only=True)
    assert set(payload) == {"MODEL_STATE", "EPOCHS_RUN"}
    # ... and a momentum FusedSGD does carry its buffers
    snap2 = str(tmp_path / "snapshot2.pt")
    tr2 = _trainer(lambda ps: FusedSGD(ps, lr=1e-2, momentum=0.9), snap2,
                   True)
    assert not tr2._needs_zero  # grad zeroing stays folded into the step
    tr2.train(2)
    payload2 = torch.load(snap2, weights_only=True)
    assert "OPTIMIZER_STATE" in payload2
    assert len(payload2["OPTIMIZER_STATE"]["state"]) == 4
