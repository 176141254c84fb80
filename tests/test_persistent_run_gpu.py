"""GPU tests of PersistentToyStep over the one native run tracker: the mesh
path (world 2 as two processes on one device) now launches from it, and the
tensor-level run of step(x, t) lives in it. However a run is cut into
launches and however the two kinds of step interleave, the params carry the
same BITS as the same batches launched one at a time."""

import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

B, K, STEPS, LR = 32, 20, 12, 0.05


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _engine(comm, **kw):
    from mi355x_ddp.engine import PersistentToyStep
    from mi355x_ddp.models import toy_model
    torch.manual_seed(11)
    model = toy_model(K, 1).to("cuda")
    eng = PersistentToyStep(model, comm=comm, lr=LR, use_mse=True, **kw)
    if comm is not None:
        eng.reducer.broadcast_params(root=0)
    return eng


def _data(seed, steps=STEPS):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(steps * B, K, generator=g).to("cuda"),
            torch.rand(steps * B, 1, generator=g).to("cuda"))


def _words(eng, comm=None):
    torch.cuda.synchronize()
    if comm is not None:
        comm.check()
    return eng.flat_param.view(torch.int32).cpu().clone()


def _mesh_worker(rank, world, port, body, out_dir):
    from mi355x_ddp.parallel.comm import GlooComm, P2pMeshComm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    try:
        comm = P2pMeshComm(torch.device("cuda", 0), base=GlooComm())
        body(rank, comm)
        torch.save({"ok": True}, os.path.join(out_dir, f"ok{rank}.pt"))
        torch.distributed.barrier()
    finally:
        torch.distributed.destroy_process_group()


def _run_world2(body, tmp_path):
    mp.spawn(_mesh_worker, args=(2, _free_port(), body, str(tmp_path)),
             nprocs=2, join=True)
    for rank in range(2):  # every assertion of both ranks held
        assert torch.load(tmp_path / f"ok{rank}.pt", weights_only=True)["ok"]


def _split_body(rank, comm):
    from mi355x_ddp import ops
    X, T = _data(100 + rank)
    got = {}
    for max_defer in (5, 1024):
        eng = _engine(comm, max_defer=max_defer)
        assert eng.ramp_first == 0, "a mesh run takes no ramp"
        eng.bind_shard(X, T, B)
        for s in range(STEPS):
            eng.step_shard(s)
        eng.flush()
        got[max_defer] = (_words(eng, comm), eng.launch_count)
    assert (got[5][1], got[1024][1]) == (3, 1)  # 5 5 2 | 12
    assert torch.equal(got[5][0], got[1024][0]), \
        f"rank {rank}: {got[5][0].tolist()} vs {got[1024][0].tolist()}"
    assert not torch.equal(got[5][0], _words(_engine(comm)))  # it trained
    # an index outside the bound shard: refused before anything is launched
    for bad in (STEPS, -1):
        with pytest.raises(IndexError):
            eng.step_shard(bad)
        assert eng.launch_count == 1 and eng._run.pending == 0
    assert torch.equal(_words(eng, comm), got[1024][0])
    # with a mesh the tracker itself refuses a ramp
    with pytest.raises(RuntimeError, match="ramp"):
        ops.ext().ToyShardRun(eng.flat_param, eng.loss_out, True, eng.w_off,
                              eng.b_off, LR, 8, 2, 2.0, comm._mesh)


def test_mesh_launch_split_bitwise_and_index_bounds(tmp_path):
    _run_world2(_split_body, tmp_path)


def _ordering_body(rank, comm):
    X, T = _data(100 + rank, steps=8)
    P, PT = _data(300 + rank, steps=2)       # a second buffer
    Q = torch.rand(K, B, generator=torch.Generator().manual_seed(500 + rank))
    xq, tq = Q.to("cuda").t(), PT[:B] * 0.5  # [B, K], not contiguous
    assert not xq.is_contiguous()

    def tile(A, AT, i):
        return A[i * B:(i + 1) * B], AT[i * B:(i + 1) * B]

    seq = ([("s", i) for i in range(4)] + [("p", 0), ("p", 1), ("q", 0)]
           + [("s", 4), ("s", 5), ("s", 2)])

    def submit(eng, kind, i):
        if kind == "s":
            eng.step_shard(i)
        elif kind == "p":
            eng.step(*tile(P, PT, i))
        else:
            eng.step(xq, tq)

    eng = _engine(comm)
    eng.bind_shard(X, T, B)
    for kind, i in seq:
        submit(eng, kind, i)
    assert eng._run.pending == 1              # the restart at 2
    eng.flush()
    deferred = _words(eng, comm)
    # shard 0..3 | the two merged tensor steps | the eager one | 4..5 | 2
    assert eng.launch_count == 5

    one = _engine(comm)
    one.bind_shard(X, T, B)
    for kind, i in seq:
        submit(one, kind, i)
        one.flush()
    assert one.launch_count == len(seq)
    assert torch.equal(deferred, _words(one, comm)), f"rank {rank}"


def test_mesh_tensor_and_shard_steps_keep_submission_order(tmp_path):
    _run_world2(_ordering_body, tmp_path)


def test_world1_tensor_run_does_not_cross_storages():
    from mi355x_ddp.engine import ToyFusedStep
    from mi355x_ddp.models import toy_model
    # two storages of two tiles each; the batches are their first tiles, so
    # even a run wrongly merged across them would stay inside the first
    XA, TA = _data(1, steps=2)
    XB, TB = _data(2, steps=2)
    batches = [(XA[:B], TA[:B]), (XB[:B], TB[:B])]

    eng = _engine(None)
    before = eng.launch_count
    for x, t in batches:
        eng.step(x, t)
    assert eng._run.pending_tensors == 1      # the second started a new run
    eng.flush()
    assert eng.launch_count - before == 2

    torch.manual_seed(11)
    ref = ToyFusedStep(toy_model(K, 1).to("cuda"), comm=None, lr=LR,
                       use_mse=True)
    for x, t in batches:
        ref.step(x, t)
    assert torch.equal(_words(eng), _words(ref))
    # and the next tile of ONE storage does extend the run
    eng.step(XA[:B], TA[:B])
    eng.step(XA[B:], TA[B:])
    assert eng._run.pending_tensors == 2
    eng.flush()
    assert eng.launch_count - before == 3
