"""GPU tests for the fused short-sequence self-attention kernels
(csrc/attention_kernels.hip) and what reaches them.

Reference: softmax(Q K^T / sqrt(D)) V and its autograd gradients in fp64 from
the STORED operands. Yardstick: the same formula in plain torch ops in the
storage dtype on the device. With e = max|got - ref| / max|ref| per result,
e_ours <= 4 * max(e_torch, eps), eps = 2^-24 (f32) or 2^-9 (bf16): one
storage rounding of the largest element, times 4 for another summation order
and the fast exponential."""

import math

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.models import HipSelfAttention, vit_tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # sentinel elements on either side; keeps 16-byte alignment
EPS = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}
SHAPES = [(1, 1, 1, 16), (1, 1, 16, 16), (2, 3, 17, 16), (1, 2, 15, 32),
          (1, 1, 33, 32), (2, 2, 50, 64), (1, 2, 63, 64), (1, 1, 64, 64)]


def _formula(qkv, heads):
    B, N, E3 = qkv.shape
    D = E3 // (3 * heads)
    q, k, v = qkv.view(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, N, heads * D)


def _out_and_grads(qkv, dout, heads):
    """(out, dQ, dK, dV) of the plain formula in qkv's dtype."""
    x = qkv.detach().clone().requires_grad_(True)
    out = _formula(x, heads)
    out.backward(dout)
    return (out.detach(), *x.grad.view(*x.shape[:2], 3, -1).unbind(2))


def _err(got, ref):
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()) if d else 0.0


def _guarded(shape, dtype, src=None):
    """A view of `shape` inside a larger NaN-filled allocation."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _pads_intact(*bufs):
    return all(bool(b[:PAD].isnan().all() and b[-PAD:].isnan().all())
               for b in bufs)


def _held(names, ours, torchs, refs, eps):
    bad = []
    for name, o, t, ref in zip(names, ours, torchs, refs):
        e_o, e_t = _err(o, ref), _err(t, ref)
        bound = 4 * max(e_t, eps)
        print(f"{name}: e_ours {e_o:.3e} e_torch {e_t:.3e} "
              f"ratio {e_o / bound:.3f}")
        if not e_o <= bound:  # catches NaN too
            bad.append((name, e_o, bound))
    return bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["normal", "peaked", "offset"])
@pytest.mark.parametrize("B,H,N,D", SHAPES)
def test_kernels_against_fp64(B, H, N, D, kind, dtype):
    E = H * D
    g = torch.Generator().manual_seed(1000 * N + D)
    x = torch.randn(B, N, 3, E, generator=g)
    if kind == "peaked":  # near one-hot softmax; overflows without the max
        x[:, :, :2] *= 6
    elif kind == "offset":  # a big per-row score offset that cancels exactly
        x[:, :, 1] += 16
    qbuf, qkv = _guarded((B, N, 3 * E), dtype, x.view(B, N, 3 * E))
    dbuf, dout = _guarded((B, N, E), dtype,
                          torch.randn(B, N, E, generator=g))
    obuf, out = _guarded((B, N, E), dtype)
    sbuf, stats = _guarded((B, H, N, 2), torch.float32)
    gbuf, dqkv = _guarded((B, N, 3 * E), dtype)

    ext = ops.ext()
    ext.attn_fwd(qkv, H, out=out, row_stats=stats)
    ext.attn_bwd(dout, qkv, stats, H, dqkv=dqkv)
    torch.cuda.synchronize()
    assert _pads_intact(qbuf, dbuf, obuf, sbuf, gbuf)

    refs = _out_and_grads(qkv.double(), dout.double(), H)
    torchs = _out_and_grads(qkv, dout, H)
    ours = (out, *dqkv.view(B, N, 3, E).unbind(2))
    assert not _held(("out", "dQ", "dK", "dV"), ours, torchs, refs,
                     EPS[dtype])


def _zeros(*shape, dtype=torch.float32, device=DEV):
    return torch.zeros(*shape, dtype=dtype, device=device)


GUARDS = {  # name -> (qkv, heads, dout dtype when only the backward refuses)
    "N=65": lambda: (_zeros(1, 65, 48), 1, None),
    "D=48": lambda: (_zeros(1, 4, 144), 1, None),
    "heads": lambda: (_zeros(1, 4, 96), 5, None),
    "strided": lambda: (_zeros(2, 4, 192)[:, :, :96], 2, None),
    "dout dtype": lambda: (_zeros(1, 4, 96), 2, torch.bfloat16),
    "cpu": lambda: (_zeros(1, 4, 96, device="cpu"), 2, None),
}


@pytest.mark.parametrize("name", GUARDS)
def test_refused_before_any_launch(name):
    qkv, heads, dout_dtype = GUARDS[name]()
    B, N, E3 = qkv.shape
    nan = float("nan")
    out = torch.full((B, N, E3 // 3), nan, device=DEV)
    dqkv = torch.full((B, N, E3), nan, device=DEV)
    ext = ops.ext()
    if dout_dtype is None:
        with pytest.raises(RuntimeError):
            ext.attn_fwd(qkv, heads, out=out)
    dout = _zeros(B, N, E3 // 3, dtype=dout_dtype or qkv.dtype,
                  device=qkv.device)
    with pytest.raises(RuntimeError):
        ext.attn_bwd(dout, qkv, _zeros(B, heads, N, 2), heads, dqkv=dqkv)
    torch.cuda.synchronize()
    assert out.isnan().all() and dqkv.isnan().all()


def test_empty_batch_launches_nothing():
    qkv = _zeros(0, 5, 96).requires_grad_(True)
    out = ops.self_attention(qkv, 2)
    assert out.shape == (0, 5, 32)
    out.sum().backward()
    assert qkv.grad.shape == qkv.shape


def test_module_against_fp64_module():
    E, H, N = 64, 4, 17
    torch.manual_seed(5)
    mha = nn.MultiheadAttention(E, H, batch_first=True).to(DEV)
    with torch.no_grad():
        mha.in_proj_bias.normal_()
        mha.out_proj.bias.normal_()
    hip = HipSelfAttention(E, H).to(DEV)
    hip.load_state_dict(mha.state_dict())
    ref = nn.MultiheadAttention(E, H, batch_first=True).to(DEV).double()
    ref.load_state_dict(mha.state_dict())
    x = torch.randn(2, N, E, device=DEV)
    dy = torch.randn(2, N, E, device=DEV)

    def run(mod, x, dy, call):
        y = call(mod, x)
        y.backward(dy)
        return [y.detach()] + [p.grad for _, p in sorted(
            mod.named_parameters())]

    def torch_call(m, x):
        return m(x, x, x, need_weights=False)[0]

    ours = run(hip, x, dy, lambda m, x: m(x))
    torchs = run(mha, x, dy, torch_call)
    refs = run(ref, x.double(), dy.double(), torch_call)
    names = ["out"] + sorted(n for n, _ in hip.named_parameters())
    assert not _held(names, ours, torchs, refs, EPS[torch.float32])


@pytest.fixture
def deterministic_torch():
    # torch's own LayerNorm/conv backward kernels are not reproducible run to
    # run by default (the default vit_tiny differs eager against eager too);
    # the attention kernels are, having no atomics
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(False)


def test_graphed_vit_tiny_matches_eager_bitwise(deterministic_torch):
    from mi355x_ddp.engine import GraphedAutogradStep
    from mi355x_ddp.parallel import DDP, FusedSGD

    W = 3
    g = torch.Generator().manual_seed(8)
    data = [(torch.rand(4, 3, 64, 64, generator=g).to(DEV),
             torch.rand(4, 10, generator=g).softmax(-1).to(DEV))
            for _ in range(4)]

    def build():
        torch.manual_seed(0)
        m = vit_tiny(attention="hip").to(DEV)
        eng = DDP(m, comm=None, cpp_hooks=False)
        opt = FusedSGD(m.parameters(), lr=0.01)
        opt.attach_reducer(eng.reducer)
        return m, eng, opt

    m_g, eng_g, opt_g = build()
    gs = GraphedAutogradStep(eng_g, ops.cross_entropy, opt_g,
                             finalize=eng_g.finalize_backward, warmup_steps=W)
    for x, t in data:
        gs.step(x, t)
    torch.cuda.synchronize()
    assert not gs._broken and 1 in gs._graphs, "the step must capture"

    m_e, eng_e, opt_e = build()
    for x, t in [data[0]] * (W + 1) + data[1:]:
        ops.cross_entropy(eng_e(x), t).backward()
        eng_e.finalize_backward()
        opt_e.step()
    torch.cuda.synchronize()
    for a, b in zip(m_g.parameters(), m_e.parameters()):
        assert torch.equal(a, b), (a - b).abs().max()
