"""Fast train-step engines for the flagship (toy Linear DDP) workload.

The reference hot loop (single_gpu.py:21-26 / SURVEY §3.5) costs, per step:
zero_grad + fwd GEMM + loss fwd + loss bwd + two bwd GEMMs + bucket
all-reduce + SGD — with 84 B of gradients the whole thing is launch-latency
bound (SURVEY §7 hard-part 2). Three engines, in increasing aggression:

- `ToyFusedStep`: ONE kernel (fused fwd + loss grad + bwd [+ in-kernel SGD
  at world 1]); at world > 1, + one tiny all-reduce + one fused-SGD kernel.
- `GraphedToyStep`: the fused step captured in a hipGraph and replayed.
- `PersistentToyStep` (the bench default): DEFERRED runs of consecutive
  steps execute as one multi-step kernel with the weights LDS-resident;
  at world > 1 with a `P2pMeshComm` the kernel performs an in-kernel xGMI
  mesh all-reduce per step. The runs are tracked, ordered and launched by
  the extension's `ToyShardRun`; the class is a thin wrapper. See
  docs/KERNELS.md.

All engines train the SAME model parameters the generic autograd path
trains: the Reducer's flat bucket is shared state, so checkpoints and the
Trainer API are unaffected. Equivalence with the autograd path (and the
bitwise multi==single contract) is covered by tests/test_engine_gpu.py.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .models.toy import HipLinear
from .parallel.reducer import Reducer


def _ramp_defaults():
    """(ramp_first, growth) of the native stepper's launch ramp: the
    measured choice (profiles/README.md r08), or MI355X_RAMP=FIRST:GROWTH
    for A/B runs of bench.py (FIRST 0 = no ramp)."""
    import os
    env = os.environ.get("MI355X_RAMP")
    if not env:
        return 64, 1.5
    first, growth = env.split(":")
    return int(first), float(growth)


RAMP_FIRST, RAMP_GROWTH = _ramp_defaults()


# Process-wide capture poison: after ONE invalidated capture, any further
# capture_begin in this process is lethal on this torch/ROCm build —
# capture_begin raises "Cannot register the state during capturing stage"
# mid-registration and the partially-registered CUDAGraph's DESTRUCTOR
# then throws inside ~CUDAGraph ("The graph should be registered to the
# state") which calls std::terminate (measured: tools/recapture_probe.py,
# every cleanup variant dumps core). So: first failure -> never capture
# again in this process; all graphed engines run eager.
_CAPTURE_POISONED = False
# Graphs whose capture failed are LEAKED on purpose: destroying them can
# terminate the process (above). A handful of small host objects.
_DEAD_GRAPHS = []
# Capture streams of failed captures. The stream stays in the invalidated
# capture state: every later operation on it fails with
# hipErrorStreamCaptureInvalidated ("operation failed due to a previous
# error during capture"). torch hands its 32 pool streams out round-robin,
# so the dead one comes round again to whoever asks for a stream next.
_DEAD_STREAMS = []


def side_stream(device=None) -> "torch.cuda.Stream":
    """torch.cuda.Stream(device), skipping the capture stream of a failed
    capture (see _DEAD_STREAMS)."""
    for _ in range(64):  # the pool holds 32 streams
        s = torch.cuda.Stream(device=device)
        if not any(s == d for d in _DEAD_STREAMS):
            return s
    raise RuntimeError("every pool stream belongs to a failed capture")


def _poison_captures(graph):
    global _CAPTURE_POISONED
    _CAPTURE_POISONED = True
    _DEAD_GRAPHS.append(graph)


def _recover_failed_capture(ctx):
    """Best-effort cleanup after an INVALIDATED stream capture (e.g. a
    library allocating outside torch's allocator mid-capture — observed
    with MIOpen NHWC workspace allocs). torch.cuda.graph.__exit__ raises
    from capture_end BEFORE exiting its stream context or ending the
    allocator's route-to-pool state, leaving the thread on the capture
    stream, allocations routed to the dead graph pool, and
    hipErrorStreamCaptureInvalidated latched in HIP's thread state.
    Undo all three so the eager fallback can proceed."""
    _DEAD_STREAMS.append(ctx.capture_stream)
    try:
        ctx.stream_ctx.__exit__(None, None, None)
    except Exception:
        pass
    try:
        dev = torch.cuda.current_device()
        torch._C._cuda_endAllocateToPool(dev, ctx.pool[0])
        torch._C._cuda_releasePool(dev, ctx.pool[0])
    except Exception:
        pass
    try:
        # capture_begin registers the default CUDA generator and flips its
        # state to capture mode (capture_prologue); only a SUCCESSFUL
        # capture_end flips it back. Nothing on the failure path clears
        # it, so the next RNG op in the process would raise "Offset
        # increment outside graph capture". Swap in a fresh state object
        # carrying the same seed/offset (graphsafe_set_state shares the
        # new state, whose capture flag starts clear).
        dev = torch.cuda.current_device()
        dg = torch.cuda.default_generators[dev]
        fresh = torch.Generator(device=f"cuda:{dev}")
        fresh.set_state(dg.get_state())
        dg.graphsafe_set_state(fresh)
    except Exception:
        pass
    if ops.has_ext():
        ops.ext().clear_hip_errors()  # pop the latched HIP error
    torch.cuda.synchronize()


def _capture_graph(body, on_failure: str):
    """body() captured in a new hipGraph. None when an earlier capture in
    this process failed (capturing again is lethal, see _CAPTURE_POISONED)
    or when this one does: it then warns with on_failure (formatted with
    the exception as `e`), poisons further captures and cleans up. The
    caller runs eager from there on."""
    if _CAPTURE_POISONED:
        return None
    g = torch.cuda.CUDAGraph()
    ctx = torch.cuda.graph(g)
    try:
        with ctx:
            body()
        return g
    except Exception as e:
        import warnings
        warnings.warn(on_failure.format(e=e), RuntimeWarning, stacklevel=3)
        _poison_captures(g)
        _recover_failed_capture(ctx)
        return None


class ToyFusedStep:
    """One-kernel fwd+bwd for HipLinear(K,1) + MSE/CE, bucket all-reduce,
    fused SGD. Works for any world size (comm=None -> single process)."""

    def __init__(self, model: HipLinear, comm=None, lr: float = 1e-3,
                 use_mse: bool = True, reducer: Optional[Reducer] = None,
                 track_loss: bool = False):
        assert (isinstance(model, HipLinear) and model.out_features == 1
                and model.bias is not None), \
            "toy engines need HipLinear(K, 1) with a bias"
        self.model = model
        self.comm = comm
        self.lr = lr
        self.use_mse = use_mse
        self.reducer = reducer or Reducer(list(model.parameters()), comm=comm)
        assert len(self.reducer.buckets) == 1, "toy model is one bucket"
        b = self.reducer.buckets[0]
        self.flat_param = b.flat_param
        self.flat_grad = b.flat_grad
        _, widx = self.reducer._param_index[model.weight]
        _, bidx = self.reducer._param_index[model.bias]
        self.w_off = b.offsets[widx]
        self.b_off = b.offsets[bidx]
        self.loss_out = (torch.zeros((), device=self.flat_param.device)
                         if track_loss else torch.Tensor())

    def step(self, x: torch.Tensor, t: torch.Tensor) -> None:
        if self.comm is None:
            # single-process: one launch = one full training step
            # (fwd + loss grad + bwd + SGD fused; no collective to wait for)
            ops.ext().toy_fused_fwd_bwd(x, t, self.flat_param, self.flat_grad,
                                        self.loss_out, self.use_mse,
                                        self.w_off, self.b_off, self.lr)
            return
        ops.ext().toy_fused_fwd_bwd(x, t, self.flat_param, self.flat_grad,
                                    self.loss_out, self.use_mse,
                                    self.w_off, self.b_off, 0.0)
        self.comm.all_reduce_avg_inline(self.flat_grad)
        ops.ext().sgd_flat(self.flat_param, self.flat_grad, self.lr, True)


class PersistentToyStep(ToyFusedStep):
    """Deferred-launch engine: runs of consecutive steps execute as ONE
    multi-step kernel launch, weights resident in LDS across steps. Works
    at world 1 (no communicator) and, with a `P2pMeshComm`, at any world
    size: the kernel then performs one in-kernel xGMI mesh all-reduce per
    step.

    A thin wrapper over the extension's `ToyShardRun`, which tracks both
    kinds of deferred run, keeps them in submission order and launches from
    raw pointers (docs/KERNELS.md, "The shard-bound stepper"):

    - `step(x, t)` defers when the batch is the next contiguous [B, K] slice
      of the same device buffer as the pending run; any other batch launches
      what is pending and starts a new run. A batch that is not contiguous
      on the device runs eagerly, after what was submitted before it.
    - `bind_shard` / `step_shard(i)` step through a bound epoch shard by
      batch index (the path bench.py drives); `step_shard` is a C function.
      An index outside the bound shard raises IndexError before anything is
      launched for it.
    - `flush()` launches what is pending. Callers must flush before
      synchronizing the stream for timing or reading params: bench.py does
      before every barrier.

    Per-step arithmetic is bitwise-identical to the single-step fused
    kernel, so deferral changes WHEN work is launched, never what is
    computed. A run is launched when it reaches `max_defer` steps. At world
    1 the index run's first launches after a `flush()` (the caller is about
    to synchronize, so the GPU will be idle) are short and grow: `ramp_first`
    steps, then times `ramp_growth` per launch up to `max_defer`. With a
    mesh there is no ramp: every rank must issue the same launches in the
    same order, so the schedule depends on the submitted steps alone.

    With track_loss=True, loss_out holds the LAST executed step's loss.
    """

    def __init__(self, *args, max_defer: int = 1024,
                 ramp_first: int = RAMP_FIRST,
                 ramp_growth: float = RAMP_GROWTH, **kwargs):
        super().__init__(*args, **kwargs)
        # world-1 (no comm), or a mesh-capable comm: the in-kernel xGMI
        # mesh exchange keeps SGD in-kernel at any world size
        self._mesh = getattr(self.comm, "_mesh", None)
        assert self.comm is None or self._mesh is not None, \
            "PersistentToyStep needs world 1 or a P2pMeshComm"
        self.max_defer = max_defer
        self.ramp_first = ramp_first if self._mesh is None else 0
        self.ramp_growth = ramp_growth
        self._run = run = ops.ext().ToyShardRun(
            self.flat_param, self.loss_out, self.use_mse, self.w_off,
            self.b_off, self.lr, max_defer, self.ramp_first, ramp_growth,
            self._mesh)
        self.bind_shard = run.bind_shard
        self.step_shard = run.step_shard  # the C function itself
        self.flush = run.flush

    @property
    def launch_count(self) -> int:
        """Kernel launches issued by the run tracker (bench transparency)."""
        return self._run.launch_count

    def step(self, x: torch.Tensor, t: torch.Tensor) -> None:
        run = self._run
        if x.is_cuda and x.is_contiguous() and t.is_contiguous():
            run.step_tensors(x, t)
            return
        run.launch_pending()  # submitted earlier: runs earlier (no arming)
        if self._mesh is None:
            super().step(x, t)
        else:
            # a single step through the same mesh kernel (S = 1): keeps the
            # per-step collective order identical on all ranks
            run.step_tensors(x.contiguous(), t.contiguous())
            run.launch_pending()


class GraphedAutogradStep:
    """The GENERIC training step — forward, loss, autograd backward with
    the reducer hooks, bucket all-reduce, fused SGD — captured in ONE
    hipGraph and replayed (torch "whole-network capture").

    This is what makes the arbitrary-model path fast on MI355X: eager, the
    step pays ~10 kernel launches plus autograd-engine and Python dispatch
    overhead (~100 us for the toy model, profiles/README.md r02); replayed,
    it pays two tiny input copies plus the graph-replay floor (~10-16 us,
    MI355X_MICROARCH price list). The step is capture-safe BY CONSTRUCTION
    here: gradients are views into the reducer's static flat buckets,
    FusedSGD updates the static flat pairs, and the reducer's bucket
    collectives are launched with stream-event edges capture records.
    The wrapped model's reducer must use PYTHON hooks
    (DDP(..., cpp_hooks=False)): a C++ node post-hook — even a no-op one —
    segfaults hipStreamEndCapture on this torch/ROCm build (bisected on
    hardware, tools/capture_bisect2.py). Hooks never execute during
    replay, so the captured path loses nothing vs the C++ core.

    Deferred multi-step replay: besides the single-step `step(x, t)` API,
    the engine speaks the shard-bound protocol (`bind_shard`/`step_shard`/
    `flush`, same contract as PersistentToyStep): runs of consecutive
    batch indices execute as replays of MULTI-STEP graphs — a G-step graph
    amortizes the replay floor and the input copies over G steps, leaving
    the in-graph kernel-boundary cost (~1.2-1.5 us per dependent kernel)
    as the bound. Runs decompose greedily over `chunk_sizes` graphs, each
    captured once on first use; warmup covers the steady-state sizes so
    captures stay out of timed regions.

    Requirements: static shapes (same batch size every step) and a model
    without data-dependent control flow — the reference workloads (toy
    Linear, ResNet-50) qualify. Autocast regions inside the step must use
    cache_enabled=False (torch's AMP+graphs rule — the cast cache frees
    tensors between iterations and invalidates the capture). Capture
    failure falls back to eager with a warning; results are unchanged
    either way.
    """

    def __init__(self, model, loss_fn, optimizer, finalize=None,
                 warmup_steps: int = 3, zero_grad: bool = False,
                 chunk_sizes=(64, 8, 1)):
        self.model = model            # DDP-wrapped or bare
        self.loss_fn = loss_fn
        self.optimizer = optimizer
        self._finalize = finalize or (lambda: None)
        self.warmup_steps = warmup_steps
        # zero_grad=True: the optimizer does not fold grad zeroing into its
        # step (i.e. it is not a bucket-attached FusedSGD) — zero INSIDE
        # the captured step, set_to_none=False so the grad buffers stay
        # static (a capture requirement, and it keeps the bucket views).
        self._zero = zero_grad
        self.chunk_sizes = tuple(sorted(set(chunk_sizes) | {1},
                                        reverse=True))
        self.max_defer = self.chunk_sizes[0]
        self._graphs = {}             # G -> (graph, xbuf, tbuf)
        self._broken = False          # capture failed: eager forever
        self._warmed = False
        self._bshape = None           # (x batch shape, t batch shape)
        self.loss = None              # last captured loss tensor
        # shard-bound state
        self._shard_x = self._shard_t = None
        self._sbatch = 0
        self._s_start = self._s_next = 0

    def _eager_step(self, x, t):
        if self._zero:
            self.optimizer.zero_grad(set_to_none=False)
        loss = self.loss_fn(self.model(x), t)
        loss.backward()
        self._finalize()
        self.optimizer.step()
        return loss

    def _warm(self, x, t):
        """torch's capture recipe: a few eager steps on a side stream
        before the first capture (allocator + autograd engine initialize
        lazily-created state off-capture). These steps train for real —
        on the first batch, like any warmup."""
        s = side_stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(self.warmup_steps):
                self._eager_step(x, t)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._warmed = True

    def _get_graph(self, G):
        """The G-step graph (captured on first use). Returns None when
        capture is broken; xbuf/tbuf hold G consecutive batches."""
        got = self._graphs.get(G)
        if got is not None or self._broken:
            return got
        if _CAPTURE_POISONED:
            self._broken = True  # an earlier capture in this process
            return None          # failed: capturing again is lethal
        B = self._bshape[0][0]
        xbuf = torch.empty((G * B,) + self._bshape[0][1:],
                           dtype=self._bdtype[0], device=self._bdev)
        tbuf = torch.empty((G * B,) + self._bshape[1][1:],
                           dtype=self._bdtype[1], device=self._bdev)

        def body():
            for i in range(G):
                self.loss = self._eager_step(xbuf[i * B:(i + 1) * B],
                                             tbuf[i * B:(i + 1) * B])

        g = _capture_graph(
            body, "[mi355x_ddp] whole-step hipGraph capture failed ({e!r}); "
            "GraphedAutogradStep running eager (correct, slower; no "
            "further captures will be attempted in this process)")
        if g is None:
            self._broken = True
            return None
        self._graphs[G] = (g, xbuf, tbuf)
        return self._graphs[G]

    def _note_shapes(self, x, t):
        if self._bshape is None:
            self._bshape = (x.shape, t.shape)
            self._bdtype = (x.dtype, t.dtype)
            self._bdev = x.device

    def step(self, x, t):
        """Single-step API (Trainer): one G=1 graph replay per call."""
        self.flush()
        self._note_shapes(x, t)
        if not self._broken and x.shape != self._bshape[0]:
            self._eager_step(x, t)  # ragged final batch: run it eager
            return
        if not self._warmed:
            self._warm(x, t)
        got = self._get_graph(1)
        if got is None:
            self._eager_step(x, t)
            return
        g, xbuf, tbuf = got
        xbuf.copy_(x.reshape(xbuf.shape), non_blocking=True)
        tbuf.copy_(t.reshape(tbuf.shape), non_blocking=True)
        g.replay()

    # -- shard-bound protocol (same contract as PersistentToyStep) -------
    def bind_shard(self, xs, ts, batch):
        self.flush()
        assert xs.is_cuda and xs.is_contiguous() and ts.is_contiguous()
        self._shard_x, self._shard_t, self._sbatch = xs, ts, batch
        self._s_start = self._s_next = 0
        if (self._bshape is not None
                and (xs[:batch].shape, ts[:batch].shape) != self._bshape):
            # batch shape changed across binds: the captured graphs read
            # fixed-shape static buffers — drop them and recapture lazily
            # at the new shape (correct, pays one recapture)
            torch.cuda.synchronize()
            self._graphs.clear()
            self._bshape = None
        self._note_shapes(xs[:batch], ts[:batch])

    def step_shard(self, i):
        if i == self._s_next:
            self._s_next += 1
            if self._s_next - self._s_start >= self.max_defer:
                self.flush()
            return
        self.flush()
        self._s_start, self._s_next = i, i + 1

    def chunks(self, n):
        """Greedy decomposition of an n-step run over chunk_sizes graphs
        (largest-first; chunk_sizes always contains 1, so any n is
        covered exactly). Pure logic — property-tested on CPU."""
        out = []
        while n:
            for G in self.chunk_sizes:
                if G <= n:
                    break
            out.append(G)
            n -= G
        return out

    def flush(self):
        if self._s_next <= self._s_start:
            return
        lo, n = self._s_start, self._s_next - self._s_start
        self._s_start = self._s_next
        B = self._sbatch
        if not self._warmed:
            self._warm(self._shard_x[lo * B:(lo + 1) * B],
                       self._shard_t[lo * B:(lo + 1) * B])
        for G in self.chunks(n):
            s, e = lo * B, (lo + G) * B
            got = self._get_graph(G)
            if got is None:  # capture broken: eager the rest of the run
                for i in range(lo, lo + n):
                    self._eager_step(self._shard_x[i * B:(i + 1) * B],
                                     self._shard_t[i * B:(i + 1) * B])
                return
            g, xbuf, tbuf = got
            xbuf.copy_(self._shard_x[s:e], non_blocking=True)
            tbuf.copy_(self._shard_t[s:e], non_blocking=True)
            g.replay()
            lo += G
            n -= G


class GraphedToyStep(ToyFusedStep):
    """ToyFusedStep captured in a hipGraph.

    The input batch lives in static device buffers; `step` copies the batch
    view into them (D2D, tiny) and replays the graph. RCCL collectives are
    capturable on ROCm (stream capture follows the comm-stream event edges).
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._graph = None
        self._x_static = None
        self._t_static = None

    def _capture(self, x: torch.Tensor, t: torch.Tensor) -> None:
        self._x_static = torch.empty_like(x)
        self._t_static = torch.empty_like(t)
        self._x_static.copy_(x)
        self._t_static.copy_(t)
        # warm up collectives/kernels outside capture first
        super().step(self._x_static, self._t_static)
        torch.cuda.synchronize()
        g = _capture_graph(
            lambda: ToyFusedStep.step(self, self._x_static, self._t_static),
            "[mi355x_ddp] hipGraph capture failed ({e!r}); "
            "GraphedToyStep running eager (correct, slower)")
        self._graph = g if g is not None else False  # False: stay eager

    def step(self, x: torch.Tensor, t: torch.Tensor) -> None:
        if self._graph is None:
            self._capture(x, t)
            return
        if self._graph is False:
            super().step(x, t)
            return
        self._x_static.copy_(x, non_blocking=True)
        self._t_static.copy_(t, non_blocking=True)
        self._graph.replay()
