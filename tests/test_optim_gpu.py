"""GPU tier of the flat-bucket optimizers: k_sgd_momentum_flat / k_adamw_flat
(+ k_adamw_tick) against the plain-torch mirrors in mi355x_ddp.ops, the
attached optimizers against torch.optim on the device, the Trainer's engine
gate and the unfenced-step assertion.

(The whole-step graph-capture tests of these optimizers live in
test_graph_optim_gpu.py: they must run BEFORE test_graphed_generic_gpu.py,
whose last test poisons stream capture for the rest of the process.)

Differences are measured with test_optim.ulps: spacings at the element's
magnitude max(|before|, |after|) — see that module's docstring for why an
in-place update is measured against its operands.

fp32: momentum SGD is one operation sequence on the host and the device,
and the kernel reproduces it bit for bit. For AdamW the kernel follows
torch's DEVICE kernels (bitwise: the 20-step test below), which place three
roundings differently from the CPU ops the mirror is made of — v's
(1-b2)*g*g product, the division by sqrt(bc2) done as a multiplication by
its reciprocal, and the final p + step*(m/denom) — and torch's CPU sqrt is
within 1 ulp but not correctly rounded. Measured on MI355X over the seeded
inputs below (profiles/README.md, "Flat-bucket optimizers"): max
FP32_MEASURED_ULPS over every output (7.0, AdamW's parameter at the
2-million-element size; <= 3 at the small sizes; the fp32 state of the
bf16 runs within 1; 0 for all of momentum SGD). The bound asserted is 2x
that, and never above the 16 ulp at which the formula, not the tolerance,
is wrong. The literal yardstick — spacings at the output's own magnitude —
is asserted as well, over the elements whose update did not cancel
(|after| >= |before|/2): measured FP32_STRICT_MEASURED_ULPS (9.0, same
case), bound 2x that under the same cap, i.e. 16.

bf16: the mirror computes in fp32 and rounds once, as the kernel does, so a
parameter may differ by at most 1 bf16 ulp, and only where the two fp32
results straddle a rounding boundary. Measured share of differing
elements: BF16_MEASURED_SHARE — none of the 25 million parameter updates
below (a difference needs an fp32 mismatch, itself of a few fp32 ulps at
most, to straddle a bf16 rounding boundary 2^16 ulps apart); asserted 2x
that, and never above 1%.
"""

import functools
import os

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD
from test_optim import (BETAS, EPS, LR_ADAM, LR_SGD, TRAJECTORY_ULPS, seeded,
                        ulps, ulps_strict)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

FP32_MEASURED_ULPS = 7.0
FP32_BOUND_ULPS = min(2 * FP32_MEASURED_ULPS, 16.0)
# the literal yardstick (spacings at the output's own magnitude) over the
# elements whose update did not cancel — test_optim.ulps_strict
FP32_STRICT_MEASURED_ULPS = 9.0
FP32_STRICT_BOUND_ULPS = min(2 * FP32_STRICT_MEASURED_ULPS, 16.0)
BF16_MEASURED_SHARE = 0.0
BF16_BOUND_SHARE = min(2 * BF16_MEASURED_SHARE, 0.01)

SIZES = [
    4,                       # one lane
    1024,                    # exactly one 256-lane block of float4
    1028,                    # one block plus one lane
    4 * (256 * 3 + 17),      # ragged multi-block
    4 * 256 * 2048 + 4,      # past the grid cap: the grid-stride loop iterates
]
MASK_N = 4 * (256 * 3 + 17)
WD = 1e-2


def _inputs(kind, dtype, n, t):
    p, g, m, v = seeded(n, 21 if kind == "sgd" else 22, t)
    if dtype == torch.bfloat16:
        p, g = p.bfloat16(), g.bfloat16()
    return p, g, m, v


def _mask(n):
    gen = torch.Generator().manual_seed(23)
    mask = (torch.rand(n // 4, generator=gen) < 0.5).to(torch.uint8)
    assert 0 < int(mask.sum()) < mask.numel()  # mixes both kinds of group
    return mask


@functools.lru_cache(maxsize=None)
def _mirror(kind, dtype, n, t, masked=False):
    """One mirror step on the CPU, computed once per case and shared by the
    zero_grad on/off runs (it does not depend on the flag)."""
    p, g, m, v = _inputs(kind, dtype, n, t)
    if kind == "sgd":
        ops.sgd_momentum_flat_(p, g, m, LR_SGD, 0.9, WD, True,
                               zero_grad=False)
        return p, m, None
    ops.adamw_flat_(p, g, m, v, t, LR_ADAM, *BETAS, EPS, WD,
                    _mask(n) if masked else None, zero_grad=False)
    return p, m, v


def _kernel(kind, dtype, n, t, zero, masked=False):
    p, g, m, v = (x.to(DEV) for x in _inputs(kind, dtype, n, t))
    g0 = g.clone()
    if kind == "sgd":
        ops.sgd_momentum_flat_(p, g, m, LR_SGD, 0.9, WD, True, zero_grad=zero)
        v = None
    else:
        state = torch.zeros(4, dtype=torch.int32, device=DEV)
        state[0] = t - 1
        ops.adamw_tick_(state, LR_ADAM, *BETAS)
        ops.adamw_flat_(p, g, m, v, state, LR_ADAM, *BETAS, EPS, WD,
                        _mask(n).to(DEV) if masked else None, zero_grad=zero)
        assert int(state[0]) == t
    torch.cuda.synchronize()
    if zero:
        assert not g.any(), "zero_grad must clear the gradient"
    else:
        assert torch.equal(g, g0), "zero_grad=False must leave the gradient"
    return p, m, v


STRICT_SEEN = [0.0]  # running max of the strict figure, printed per test


def _compare(kind, dtype, n, t, zero, masked=False):
    """-> (worst fp32 ulps over the fp32 outputs, differing bf16 params);
    the strict figure of the same outputs is asserted here."""
    p0, _, m0, v0 = _inputs(kind, dtype, n, t)
    got = _kernel(kind, dtype, n, t, zero, masked)
    want = _mirror(kind, dtype, n, t, masked)
    worst, flips = 0.0, 0
    for name, g_, w_, before in (("p", got[0], want[0], p0),
                                 ("m", got[1], want[1], m0),
                                 ("v", got[2], want[2], v0)):
        if g_ is None:
            continue
        assert g_.dtype == w_.dtype, name
        if name != "p":
            assert g_.dtype == torch.float32, "optimizer state stays fp32"
        if g_.dtype == torch.bfloat16:
            assert ulps(g_.float(), w_.float(), before.float(),
                        mant_bits=7) <= 1.0
            flips += int((g_.cpu() != w_).sum())
        else:
            worst = max(worst, ulps(g_, w_, before))
            strict = ulps_strict(g_, w_, before)
            STRICT_SEEN[0] = max(STRICT_SEEN[0], strict)
            assert strict <= FP32_STRICT_BOUND_ULPS, (name, strict)
    return worst, flips


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fp32_kernel_matches_mirror(kind, n):
    worst = 0.0
    for t in (1, 2, 1000):
        for zero in (True, False):
            worst = max(worst, _compare(kind, torch.float32, n, t, zero)[0])
    print(f"[optim] fp32 {kind} n={n}: max {worst:.3f} ulp "
          f"(strict, running max: {STRICT_SEEN[0]:.3f})")
    assert worst <= FP32_BOUND_ULPS


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_bf16_kernel_matches_mirror(kind, n):
    worst, flips, total = 0.0, 0, 0
    for t in (1, 2, 1000):
        for zero in (True, False):
            w, f = _compare(kind, torch.bfloat16, n, t, zero)
            worst, flips, total = max(worst, w), flips + f, total + n
    print(f"[optim] bf16 {kind} n={n}: state max {worst:.3f} ulp, "
          f"{flips}/{total} params differ (share {flips / total:.2e})")
    assert worst <= FP32_BOUND_ULPS      # the fp32 state
    assert flips / total <= BF16_BOUND_SHARE


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adamw_decay_mask(dtype):
    worst, flips = 0.0, 0
    for t in (1, 1000):
        w, f = _compare("adamw", dtype, MASK_N, t, True, masked=True)
        worst, flips = max(worst, w), flips + f
    print(f"[optim] masked adamw {dtype}: max {worst:.3f} ulp, "
          f"{flips} bf16 params differ")
    assert worst <= FP32_BOUND_ULPS
    assert flips / (2 * MASK_N) <= BF16_BOUND_SHARE
    # the mask must matter: masked groups equal a weight_decay=0 step and
    # differ from the decayed one
    if dtype == torch.float32:
        p, g, m, v = (x.to(DEV) for x in _inputs("adamw", dtype, MASK_N, 2))
        state = torch.tensor([2, 0, 0, 0], dtype=torch.int32, device=DEV)
        ops.adamw_tick_(state, LR_ADAM, *BETAS)  # -> t = 3
        plain = p.clone()
        ops.adamw_flat_(plain, g.clone(), m.clone(), v.clone(), state,
                        LR_ADAM, *BETAS, EPS, 0.0, None, zero_grad=False)
        ops.adamw_flat_(p, g, m, v, state, LR_ADAM, *BETAS, EPS, 0.5,
                        _mask(MASK_N).to(DEV), zero_grad=False)
        keep = ops._expand_mask(_mask(MASK_N), MASK_N).to(DEV)
        assert torch.equal(p[~keep], plain[~keep])
        assert not torch.equal(p[keep], plain[keep])


def test_weight_decay_only_sgd_needs_no_buffer():
    p, g, _, _ = (x.to(DEV) for x in _inputs("sgd", torch.float32, 1028, 1))
    want_p, want_g, _, _ = _inputs("sgd", torch.float32, 1028, 1)
    p0 = want_p.clone()
    ops.sgd_momentum_flat_(want_p, want_g, None, LR_SGD, 0.0, WD, False)
    ops.sgd_momentum_flat_(p, g, None, LR_SGD, 0.0, WD, False)
    assert ulps(p, want_p, p0) <= FP32_BOUND_ULPS and not g.any()
    with pytest.raises((ValueError, RuntimeError)):
        ops.sgd_momentum_flat_(p, g, None, LR_SGD, 0.9, WD, False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_sgd_equals_momentum_kernel_bitwise(dtype):
    """k_sgd_flat is the one fma of k_sgd_momentum_flat without momentum or
    decay (which is itself held bitwise to torch.optim above)."""
    p, g, _, _ = (x.to(DEV) for x in _inputs("sgd", dtype, 1024, 1))
    p2, g2 = p.clone(), g.clone()
    ops.ext().sgd_flat(p, g, LR_SGD, True)
    ops.ext().sgd_momentum_flat(p2, g2, None, LR_SGD, 0, 0, False, True)
    assert not torch.equal(p, _inputs("sgd", dtype, 1024, 1)[0].to(DEV))
    assert torch.equal(p, p2)
    assert not g.any() and not g2.any()


def test_plain_sgd_rejects_mismatched_and_misaligned_buffers():
    base = torch.ones(1032, device=DEV)
    g = torch.ones(1024, device=DEV)
    with pytest.raises(RuntimeError, match="length"):
        ops.ext().sgd_flat(base[:1028], g, 0.5, True)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.ext().sgd_flat(base[1:1025], g, 0.5, True)  # 4 B past 16 B
    torch.cuda.synchronize()
    assert bool((base == 1).all()) and bool((g == 1).all())  # nothing ran


# ---------------------------------------------------------------------------
# attached optimizers vs torch.optim on the device
# ---------------------------------------------------------------------------
def _mlp(seed=0):
    # 31*67, 67, 67*129, 129, 129*131, 131, 1310, 10: no size is a
    # multiple of 4, and 129*131 elements overflow a 0.05 MB bucket
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(31, 67), nn.ReLU(), nn.Linear(67, 129),
                         nn.ReLU(), nn.Linear(129, 131), nn.ReLU(),
                         nn.Linear(131, 10)).to(DEV)


def _batches(k, seed=31):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(16, 31, generator=gen).to(DEV),
             torch.randn(16, 10, generator=gen).to(DEV)) for _ in range(k)]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_attached_optimizer_matches_torch_20_steps(kind):
    """Tolerance: the CPU tier allows TRAJECTORY_ULPS (8) for a trajectory
    whose single step is held to 1 rounding-level bound; a kernel step is
    held to FP32_BOUND_ULPS instead, so the trajectory bound scales by that
    factor: 8 * max(1, FP32_BOUND_ULPS) ulp, at the magnitude
    max(|initial|, |final|) of each parameter. Measured: 0 ulp for both —
    the kernels round as torch's device optimizers do — and exact equality
    is asserted besides. (An AdamW kernel
    rounding as torch's CPU ops do measured 110 ulp here: Adam's
    normalisation amplifies a 1-ulp seed through the network.)"""
    m_a, m_b = _mlp(), _mlp()
    init = [p.detach().clone() for p in m_b.parameters()]
    eng = DDP(m_a, comm=None, bucket_cap_mb=0.05)
    assert len(eng.reducer.buckets) >= 3
    if kind == "sgd":
        opt = FusedSGD(m_a.parameters(), lr=LR_SGD, momentum=0.9,
                       weight_decay=WD, nesterov=True)
        ref = torch.optim.SGD(m_b.parameters(), lr=LR_SGD, momentum=0.9,
                              weight_decay=WD, nesterov=True, foreach=False)
    else:
        opt = FusedAdamW(m_a.parameters(), lr=LR_ADAM, betas=BETAS, eps=EPS,
                         weight_decay=WD)
        ref = torch.optim.AdamW(m_b.parameters(), lr=LR_ADAM, betas=BETAS,
                                eps=EPS, weight_decay=WD, foreach=False)
    opt.attach_reducer(eng.reducer)
    for x, t in _batches(20):
        nn.functional.mse_loss(eng(x), t).backward()
        eng.finalize_backward()
        opt.step()
        ref.zero_grad()
        nn.functional.mse_loss(m_b(x), t).backward()
        ref.step()
    torch.cuda.synchronize()
    bound = TRAJECTORY_ULPS * max(1.0, FP32_BOUND_ULPS)
    worst = max(ulps(a, b, p0) for a, b, p0 in
                zip(m_a.parameters(), m_b.parameters(), init))
    print(f"[optim] attached {kind} vs torch.optim, 20 steps: "
          f"max {worst:.3f} ulp (bound {bound})")
    assert worst <= bound
    # Stronger, and what the documentation claims for these inputs: the
    # kernels issue the very rounding sequence of torch's device ops, so
    # the two runs see identical parameters, hence identical gradients,
    # at every step. Anything else is a kernel that rounds differently.
    for a, b in zip(m_a.parameters(), m_b.parameters()):
        assert torch.equal(a, b), (a - b).abs().max()
    assert all(not fg.any() for _, fg in opt._flat_pairs)
    if kind == "adamw":
        assert int(opt._step_state[0]) == 20


def test_trainer_keeps_momentum_sgd_off_the_toy_engines(tmp_path):
    """engine="auto" must not hand a momentum optimizer to the toy kernels
    (they apply p -= lr*g only). 5 steps then match torch.optim.SGD with
    momentum on an identical nn.Linear.

    Tolerance: HipLinear's forward differs from nn.Linear's by fp32
    accumulation order, |dy| <= K*eps*|x||w| with K = 20, |x|,|w| < 1, so a
    gradient element (2/B * sum dy*x) is off by <= 2*K*eps ~ 4.8e-6; the
    momentum sum weighs it by <= 1/(1-0.9) = 10 and 5 steps of lr = 1e-3
    add up: atol = 1e-3 * 5 * 10 * 4.8e-6 = 2.4e-7."""
    from mi355x_ddp.data import ToyDataset, prepare_dataloader
    from mi355x_ddp.models import toy_model
    from mi355x_ddp.trainer import Trainer

    lr = 1e-3
    torch.manual_seed(4)
    model = toy_model(20, 1)
    twin = nn.Linear(20, 1)
    twin.load_state_dict(model.state_dict())
    twin.to(DEV)
    ds = ToyDataset(160, seed=6)
    loader = prepare_dataloader(ds, 32, shuffle=False)
    tr = Trainer(model, loader, FusedSGD(model.parameters(), lr, momentum=0.9),
                 gpu_id=0, save_every=10 ** 9, loss_fn="mse", engine="auto",
                 checkpoint_path=str(tmp_path / "c.pt"))
    assert tr._engine is None, "a stateful optimizer must stay on hooks"
    tr.train(1)

    ref = torch.optim.SGD(twin.parameters(), lr=lr, momentum=0.9)
    plain = nn.Linear(20, 1).to(DEV)
    plain.load_state_dict(twin.state_dict())
    ref_plain = torch.optim.SGD(plain.parameters(), lr=lr)
    for i in range(5):
        x = ds.inputs[i * 32:(i + 1) * 32].to(DEV)
        t = ds.targets[i * 32:(i + 1) * 32].to(DEV)
        for mod, o in ((twin, ref), (plain, ref_plain)):
            o.zero_grad()
            nn.functional.mse_loss(mod(x), t).backward()
            o.step()
    torch.cuda.synchronize()
    atol = lr * 5 * 10 * (2 * 20 * 2.0 ** -23)
    got = tr._unwrapped()
    assert torch.allclose(got.weight, twin.weight, rtol=0, atol=atol)
    assert torch.allclose(got.bias, twin.bias, rtol=0, atol=atol)
    # momentum-less SGD lands visibly elsewhere: the momentum was applied
    assert (got.weight - plain.weight).abs().max() > 100 * atol

    # the plain optimizer still qualifies for the toy engine
    m2 = toy_model(20, 1)
    tr2 = Trainer(m2, loader, FusedSGD(m2.parameters(), lr), gpu_id=0,
                  save_every=10 ** 9, loss_fn="mse", engine="auto",
                  checkpoint_path=str(tmp_path / "c2.pt"))
    assert tr2._engine is not None


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_debug_sync_catches_unfenced_step(kind, monkeypatch):
    monkeypatch.setenv("MI355X_DEBUG_SYNC", "1")
    m = _mlp(3)
    eng = DDP(m, comm=None, cpp_hooks=False)
    opt = (FusedSGD(m.parameters(), lr=LR_SGD, momentum=0.9) if kind == "sgd"
           else FusedAdamW(m.parameters()))
    opt.attach_reducer(eng.reducer)
    x, t = _batches(1)[0]
    nn.functional.mse_loss(eng(x), t).backward()
    eng.reducer._unfenced = True  # collectives launched, finalize() skipped
    with pytest.raises(RuntimeError, match="unfenced"):
        opt.step()
    eng.finalize_backward()
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in m.parameters())
