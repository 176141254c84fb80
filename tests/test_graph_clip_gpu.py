"""Whole-step hipGraph capture of the flat-bucket optimizers WITH global
grad-norm clipping (`max_grad_norm`), through GraphedAutogradStep, world 1.

The point: the norm, the coefficient and the scaling all stay on the
device — k_sumsq_flat per bucket, one k_clip_coef, the coefficient read by
the update kernels — so the captured step recomputes them on every replay.
A coefficient read back to the host would be baked in at its capture-time
value.

Oracle, as in test_graph_optim_gpu.py (same model, data and method): the
same optimizer class run eager from the same init and data, with the
capture call's warmup steps replicated; parameters, optimizer state, step
count and `grad_norm` must be torch.equal.

This file sorts before test_graphed_generic_gpu.py on purpose: that file's
last test invalidates a capture, after which no engine in the process
captures again (engine._CAPTURE_POISONED).
"""

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.engine import GraphedAutogradStep
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD
from test_graph_optim_gpu import B, DEV, _assert_same, _eager, _shard

pytestmark = pytest.mark.gpu

# the model's gradient norm stays above 0.2 on this data (asserted per step)
MAX_NORM = 0.05


def _build(kind, seed):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(31, 67), nn.ReLU(), nn.Linear(67, 129),
                      nn.ReLU(), nn.Linear(129, 131), nn.ReLU(),
                      nn.Linear(131, 10)).to(DEV)
    # capture needs Python hooks (reducer.py); several buckets
    eng = DDP(m, comm=None, bucket_cap_mb=0.05, cpp_hooks=False)
    assert len(eng.reducer.buckets) >= 3
    if kind == "adamw":
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2,
                         no_decay_params=[p for n, p in m.named_parameters()
                                          if n.endswith("bias")],
                         max_grad_norm=MAX_NORM)
    else:
        opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9,
                       weight_decay=1e-2, nesterov=True,
                       max_grad_norm=MAX_NORM)
    opt.attach_reducer(eng.reducer)
    return m, eng, opt


def _assert_same_clip(opt_g, opt_e):
    assert opt_g.grad_norm is not None
    assert torch.equal(opt_g.grad_norm, opt_e.grad_norm)
    assert torch.equal(opt_g.clip_coef, opt_e.clip_coef)
    assert 0 < float(opt_g.clip_coef) < 1


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_graphed_clipped_single_step_replay_matches_eager_bitwise(kind):
    xs, ts = _shard(6, 41)
    m_g, eng_g, opt_g = _build(kind, 0)
    gs = GraphedAutogradStep(eng_g, ops.mse_loss, opt_g,
                             finalize=eng_g.finalize_backward)
    norms_g = []
    for i in range(6):
        gs.step(xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
        norms_g.append(opt_g.grad_norm.clone())
    torch.cuda.synchronize()
    assert not gs._broken and 1 in gs._graphs

    m_e, eng_e, opt_e = _build(kind, 0)
    for _ in range(gs.warmup_steps):
        _eager(eng_e, opt_e, xs[:B], ts[:B])
    norms_e = []
    for i in range(6):
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
        norms_e.append(opt_e.grad_norm.clone())
        assert float(opt_e.clip_coef) < 1, "the clip must be active"
    torch.cuda.synchronize()
    _assert_same(kind, m_g, opt_g, m_e, opt_e, gs.warmup_steps + 6)
    _assert_same_clip(opt_g, opt_e)
    # the norm is recomputed on the device by every replay, not baked in:
    # replays on different batches leave different norms, each the eager one
    assert torch.equal(torch.stack(norms_g), torch.stack(norms_e))
    assert all(float(a) != float(b) for a, b in zip(norms_g, norms_g[1:]))


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_graphed_clipped_chunks_match_eager_bitwise(kind):
    # 73 steps over the default chunk_sizes (64, 8, 1): one replay of each
    S = 64 + 8 + 1
    xs, ts = _shard(S, 43)
    m_g, eng_g, opt_g = _build(kind, 1)
    gs = GraphedAutogradStep(eng_g, ops.mse_loss, opt_g,
                             finalize=eng_g.finalize_backward,
                             chunk_sizes=(64, 8, 1))
    gs.bind_shard(xs, ts, B)
    for i in range(S):
        gs.step_shard(i)
    gs.flush()
    torch.cuda.synchronize()
    assert not gs._broken and set(gs._graphs) == {64, 8, 1}

    m_e, eng_e, opt_e = _build(kind, 1)
    for _ in range(gs.warmup_steps):
        _eager(eng_e, opt_e, xs[:B], ts[:B])
    for i in range(S):
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
        if i % 8 == 0:
            assert float(opt_e.clip_coef) < 1, "the clip must be active"
    torch.cuda.synchronize()
    _assert_same(kind, m_g, opt_g, m_e, opt_e, gs.warmup_steps + S)
    _assert_same_clip(opt_g, opt_e)
