"""FlatBucketOptimizer: what every optimizer that steps over the reducer's
flat buckets shares (FusedSGD, FusedAdamW).

Attached to a Reducer, `step()` is one streaming kernel per bucket over
(flat_param, flat_grad) with the grad zeroing folded in, and the optimizer
state lives in fp32 flat buffers of the same layout, one per bucket;
`self.state[p]` holds per-parameter VIEWS of them. Un-attached (or for
parameters outside every bucket) the same formula runs per parameter.

Limits shared by the subclasses:
- attached, a single param_group: a bucket takes one set of hyper-parameters;
- `lr` is a host scalar: whole-step graph capture bakes it in, so a
  scheduler that changes it needs a recapture;
- bf16 parameters are updated in fp32 arithmetic with one rounding on the
  store; there are no fp32 master weights.
"""

from __future__ import annotations

import os
from typing import Dict, Iterable, List

import torch


class FlatBucketOptimizer(torch.optim.Optimizer):
    # names of the per-parameter state tensors kept in flat fp32 buffers,
    # under torch.optim's own state keys (state_dict interchange)
    _state_keys: tuple = ()

    def __init__(self, params: Iterable[torch.nn.Parameter], defaults: dict):
        super().__init__(params, defaults)
        self._flat_pairs = None  # bound by attach_reducer
        self._bucketed = set()
        self._reducer = None
        self._flat_state: Dict[str, List[torch.Tensor]] = {}

    # -- reducer binding ---------------------------------------------------
    def attach_reducer(self, reducer) -> None:
        """Bind the reducer's flat (param, grad) pairs; step() then runs one
        fused kernel per bucket instead of one update per parameter.
        Requires a single param_group: the flat-bucket step applies ONE set
        of hyper-parameters to each bucket, and the per-group loop in step()
        would otherwise re-apply every bucket once per group."""
        name = type(self).__name__
        if len(self.param_groups) != 1:
            raise ValueError(f"{name}.attach_reducer requires a single "
                             "param_group (flat buckets take one lr)")
        self._flat_pairs = reducer.flat_pairs()
        self._bucketed = {id(p) for b in reducer.buckets for p in b.params}
        self._reducer = reducer
        self._bind_flat_state()

    def _stateful(self) -> bool:
        """Whether the configured update keeps per-parameter state."""
        return bool(self._state_keys)

    def _bind_flat_state(self) -> None:
        """Allocate the flat fp32 state buffers (one per bucket and key)
        and point self.state[p] at views of them, carrying over whatever
        per-parameter state exists already (a load_state_dict or steps
        taken before the attach)."""
        if self._reducer is None or not self._stateful():
            self._flat_state = {}
            return
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        buckets = self._reducer.buckets
        for key in self._state_keys:
            have = self._flat_state.get(key)
            # buffers that already fit these buckets are KEPT and written
            # in place: a captured graph that updates them stays valid
            # across a load_state_dict or a repeated attach
            if have is not None and len(have) == len(buckets) and all(
                    f.numel() == b.numel
                    and f.device == b.flat_param.device
                    for f, b in zip(have, buckets)):
                continue
            self._flat_state[key] = [
                torch.zeros(b.numel, dtype=torch.float32,
                            device=b.flat_param.device) for b in buckets]
        for bi, b in enumerate(self._reducer.buckets):
            for i, p in enumerate(b.params):
                if id(p) not in mine:
                    continue
                off, st = b.offsets[i], self.state[p]
                for key in self._state_keys:
                    view = self._flat_state[key][bi][off:off + p.numel()] \
                        .view_as(p)
                    old = st.get(key)
                    if old is None:
                        view.zero_()
                    elif old.data_ptr() != view.data_ptr():
                        view.copy_(old)
                    st[key] = view
                self._init_param_state(p, st)

    def _init_param_state(self, p, st) -> None:
        """Fill in what self.state[p] holds besides the flat-state views."""

    def _param_state(self, p) -> dict:
        """State of a parameter stepped outside the buckets, created
        zero-filled on first use (fp32 whatever the parameter dtype)."""
        st = self.state[p]
        for key in self._state_keys:
            if key not in st:
                st[key] = torch.zeros_like(p, dtype=torch.float32,
                                           memory_format=torch.contiguous_format)
        self._init_param_state(p, st)
        return st

    # -- step-side helpers ---------------------------------------------------
    def _check_fenced(self) -> None:
        # Stream-race assertion (MI355X_DEBUG_SYNC=1): the
        # fused step reads flat_grad on the compute stream — if bucket
        # collectives were launched but finalize() never fenced them, that
        # read races the comm stream. Catch the protocol violation loudly
        # instead of training on half-reduced gradients.
        if (os.environ.get("MI355X_DEBUG_SYNC") == "1"
                and self._reducer is not None
                and self._reducer.unfenced):
            raise RuntimeError(
                f"{type(self).__name__}.step() called while bucket "
                "all-reduces are "
                "in flight and unfenced — call finalize_backward() (or "
                "Reducer.finalize()) between loss.backward() and "
                "optimizer.step()")

    def _loose_params(self, group):
        """The group's parameters that step() updates one by one: all of
        them un-attached, those outside every bucket otherwise."""
        for p in group["params"]:
            if p.grad is not None and id(p) not in self._bucketed:
                yield p

    def zero_grad(self, set_to_none: bool = True):
        if self._flat_pairs is not None:
            # bucketed grads are zeroed by the fused step; nothing to do
            # unless the user zeroes before the first step.
            for _, flat_grad in self._flat_pairs:
                flat_grad.zero_()
            return
        super().zero_grad(set_to_none=set_to_none)

    # -- state_dict interchange with torch.optim ---------------------------
    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """Accepts this class's own state_dict and the matching torch.optim
        one. The inherited loader deep-copies the state tensors and casts
        them to the parameter dtype; that would detach self.state[p] from
        the flat buffers and, for bf16 parameters, round the fp32 state to
        bf16. The state is therefore taken from the incoming dict at full
        precision and copied INTO the existing fp32 flat views, so the
        bucket kernels — and a graph captured over them — keep seeing it."""
        # the saved tensors, by parameter, BEFORE the inherited loader sees
        # them: it casts state to the parameter dtype, which for bf16
        # parameters would round the fp32 state to 8 bits of mantissa
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        saved = {}
        if len(ids) == len(params):  # else the inherited loader raises
            for i, p in zip(ids, params):
                st = state_dict["state"].get(i)
                if st is not None:
                    saved[p] = {k: st[k] for k in self._state_keys
                                if torch.is_tensor(st.get(k))}
        super().load_state_dict(state_dict)
        self._check_hyper()
        for p, tensors in saved.items():
            for key, t in tensors.items():
                self.state[p][key] = t.detach().to(
                    device=p.device, dtype=torch.float32).clone()
        self._adopt_loaded_state()
        self._bind_flat_state()

    def _check_hyper(self) -> None:
        """Reject hyper-parameters the kernels do not implement."""

    def _adopt_loaded_state(self) -> None:
        """Take over loaded state that is not a flat-buffer tensor."""
