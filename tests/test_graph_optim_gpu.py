"""Whole-step hipGraph capture of the stateful flat-bucket optimizers
(FusedAdamW, momentum FusedSGD) through GraphedAutogradStep, world 1.

The point is the step count: a captured graph bakes host scalars in, so
Adam's bias corrections must come from a count that the graph itself
advances on the device (k_adamw_tick). A host-side count would freeze at
its capture-time value and, at t <= 9, move every update by tens of
percent — nowhere near the bitwise equality asserted here.

Oracle: the same optimizer class run eager from the same init and data,
with the capture call's warmup steps replicated; parameters AND optimizer
state must be torch.equal.

This file sorts before test_graphed_generic_gpu.py on purpose: that file's
last test invalidates a capture, after which no engine in the process
captures again (engine._CAPTURE_POISONED).
"""

import copy

import pytest
import torch
from torch import nn

from mi355x_ddp import ops
from mi355x_ddp.engine import GraphedAutogradStep
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 16


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
                                          if n.endswith("bias")])
    else:
        opt = FusedSGD(m.parameters(), lr=1e-2, momentum=0.9,
                       weight_decay=1e-2, nesterov=True)
    opt.attach_reducer(eng.reducer)
    return m, eng, opt


def _shard(steps, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(steps * B, 31, generator=gen).to(DEV),
            torch.randn(steps * B, 10, generator=gen).to(DEV))


def _eager(eng, opt, x, t):
    ops.mse_loss(eng(x), t).backward()
    eng.finalize_backward()
    opt.step()


def _assert_same(kind, m_g, opt_g, m_e, opt_e, steps):
    for a, b in zip(m_g.parameters(), m_e.parameters()):
        assert torch.equal(a, b), (a - b).abs().max()
    assert opt_g._flat_state.keys() == opt_e._flat_state.keys()
    for key, bufs in opt_g._flat_state.items():
        for a, b in zip(bufs, opt_e._flat_state[key]):
            assert a.dtype == torch.float32 and a.any()
            assert torch.equal(a, b), (key, (a - b).abs().max())
    if kind == "adamw":
        assert int(opt_g._step_state[0]) == int(opt_e._step_state[0]) == steps


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_graphed_single_step_replay_matches_eager_bitwise(kind):
    xs, ts = _shard(6, 41)
    m_g, eng_g, opt_g = _build(kind, 0)
    gs = GraphedAutogradStep(eng_g, ops.mse_loss, opt_g,
                             finalize=eng_g.finalize_backward)
    for i in range(6):
        gs.step(xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    assert not gs._broken and 1 in gs._graphs

    # eager arm: the warmup trains warmup_steps times on batch 0, then the
    # 6 batches in order
    m_e, eng_e, opt_e = _build(kind, 0)
    for _ in range(gs.warmup_steps):
        _eager(eng_e, opt_e, xs[:B], ts[:B])
    for i in range(6):
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    _assert_same(kind, m_g, opt_g, m_e, opt_e, gs.warmup_steps + 6)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_graphed_multi_step_chunks_match_eager_bitwise(kind):
    # 7 steps over chunk_sizes (4, 1): one 4-step graph, three 1-step replays
    S = 7
    xs, ts = _shard(S, 43)
    m_g, eng_g, opt_g = _build(kind, 1)
    gs = GraphedAutogradStep(eng_g, ops.mse_loss, opt_g,
                             finalize=eng_g.finalize_backward,
                             chunk_sizes=(4, 1))
    gs.bind_shard(xs, ts, B)
    for i in range(S):
        gs.step_shard(i)
    gs.flush()
    torch.cuda.synchronize()
    assert not gs._broken and 4 in gs._graphs and 1 in gs._graphs

    m_e, eng_e, opt_e = _build(kind, 1)
    for _ in range(gs.warmup_steps):
        _eager(eng_e, opt_e, xs[:B], ts[:B])
    for i in range(S):
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    _assert_same(kind, m_g, opt_g, m_e, opt_e, gs.warmup_steps + S)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_load_state_dict_after_capture_keeps_the_graph_valid(kind):
    # load_state_dict writes into the flat buffers and the device counter
    # the captured step updates; fresh buffers would leave the graph
    # training on the old ones
    xs, ts = _shard(6, 47)
    m_g, eng_g, opt_g = _build(kind, 2)
    gs = GraphedAutogradStep(eng_g, ops.mse_loss, opt_g,
                             finalize=eng_g.finalize_backward)
    m_e, eng_e, opt_e = _build(kind, 2)
    for _ in range(gs.warmup_steps):
        _eager(eng_e, opt_e, xs[:B], ts[:B])
    for i in range(3):
        gs.step(xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    # hand the graphed optimizer the eager one's state, moved on one step
    _eager(eng_e, opt_e, xs[3 * B:4 * B], ts[3 * B:4 * B])
    torch.cuda.synchronize()
    opt_g.load_state_dict(copy.deepcopy(opt_e.state_dict()))
    with torch.no_grad():
        for a, b in zip(m_g.parameters(), m_e.parameters()):
            a.copy_(b)
    for i in (4, 5):
        gs.step(xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
        _eager(eng_e, opt_e, xs[i * B:(i + 1) * B], ts[i * B:(i + 1) * B])
    torch.cuda.synchronize()
    assert not gs._broken and 1 in gs._graphs
    _assert_same(kind, m_g, opt_g, m_e, opt_e, gs.warmup_steps + 6)
