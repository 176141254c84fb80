"""FlatBucketOptimizer: what every optimizer that steps over the reducer's
flat buckets shares (FusedSGD, FusedAdamW).

Attached to a Reducer, `step()` is one streaming kernel per bucket over
(flat_param, flat_grad) with the grad zeroing folded in, and the optimizer
state lives in fp32 flat buffers of the same layout, one per bucket;
`self.state[p]` holds per-parameter VIEWS of them. Un-attached (or for
parameters outside every bucket) the same formula runs per parameter.

`max_grad_norm` clips the gradient by its global L2 norm over all of the
optimizer's parameters, as torch.nn.utils.clip_grad_norm_ does between
backward() and step(), but inside the step: one read pass per bucket for
the norm (`ops.grad_sumsq_flat_`), one `ops.clip_coef_`, and the
coefficient folded into the update kernels, which read every gradient
anyway. Nothing is read back to the host, so an attached step still
captures into a hipGraph; every rank computes the same bits from the same
averaged buckets, so no collective is needed. `opt.grad_norm` /
`opt.clip_coef` are device views of the last step's pre-clip norm and
coefficient (reading them is the caller's sync). The total norm is fp32
whatever the gradient dtype (torch returns bf16 for bf16 gradients).
Non-finite gradients behave as torch's default error_if_nonfinite=False:
a NaN norm gives a NaN coefficient, an infinite one gives 0 (and inf * 0 =
NaN at the offending element).

Limits shared by the subclasses:
- attached, a single param_group: a bucket takes one set of hyper-parameters;
- `lr` is a host scalar: whole-step graph capture bakes it in, so a
  scheduler that changes it needs a recapture;
- bf16 parameters are updated in fp32 arithmetic with one rounding on the
  store; there are no fp32 master weights;
- clipping is by the global L2 norm only: no other norm type, no
  error_if_nonfinite, no per-group clipping. `max_grad_norm` is an
  attribute, not a param-group key, and not part of `state_dict()`.
"""

from __future__ import annotations

import math
import os
from typing import Dict, Iterable, List, Optional

import torch

from .. import ops


class FlatBucketOptimizer(torch.optim.Optimizer):
    # names of the per-parameter state tensors kept in flat fp32 buffers,
    # under torch.optim's own state keys (state_dict interchange)
    _state_keys: tuple = ()

    def __init__(self, params: Iterable[torch.nn.Parameter], defaults: dict,
                 max_grad_norm: Optional[float] = None):
        super().__init__(params, defaults)
        self._flat_pairs = None  # bound by attach_reducer
        self._bucketed = set()
        self._reducer = None
        self._flat_state: Dict[str, List[torch.Tensor]] = {}
        # clipping: float64 partial sums of squares, the buckets' segments
        # side by side plus one trailing slot for the loose parameters,
        # and float32 [total_norm, coef]; allocated on first need, reused
        self._clip_partials = None
        self._clip_segments = None  # per bucket (lo, hi); None = rebind
        self._loose_slot_used = False
        self._clip_state = None
        self._clipped = False  # a clipped step has run
        self.max_grad_norm = max_grad_norm

    # -- global grad-norm clipping -------------------------------------------
    @property
    def max_grad_norm(self) -> Optional[float]:
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value: Optional[float]) -> None:
        if value is not None:
            value = float(value)
            if not (math.isfinite(value) and value > 0):
                raise ValueError(f"invalid max_grad_norm {value}: a positive "
                                 "finite number, or None for no clipping")
        self._max_grad_norm = value

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """Pre-clip global L2 norm of the most recent clipped step: a 0-dim
        float32 view on the device; None before the first such step."""
        return self._clip_state[0] if self._clipped else None

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """The coefficient the most recent clipped step scaled its
        gradients by, min(1, max_grad_norm / (grad_norm + 1e-6))."""
        return self._clip_state[1] if self._clipped else None

    def _bind_clip_buffers(self, device) -> None:
        """(Re)allocate the clip buffers unless they already fit the bucket
        layout on `device` — kept across a repeated attach or a
        load_state_dict, like the flat state, so that a captured graph
        stays valid."""
        sizes = [] if self._flat_pairs is None else \
            [ops.sumsq_slots(fg.numel()) for _, fg in self._flat_pairs]
        total = sum(sizes) + 1
        have = self._clip_partials
        if have is None or have.numel() != total or have.device != device:
            self._clip_partials = torch.zeros(total, dtype=torch.float64,
                                              device=device)
            self._loose_slot_used = False
        if self._clip_state is None or self._clip_state.device != device:
            self._clip_state = torch.zeros(2, dtype=torch.float32,
                                           device=device)
            self._clipped = False
        self._clip_segments, lo = [], 0
        for n in sizes:
            self._clip_segments.append((lo, lo + n))
            lo += n

    def _clip(self) -> Optional[torch.Tensor]:
        """With max_grad_norm set: compute the global norm and the clip
        coefficient on the device, scale the loose gradients in place and
        return the 1-element grad_scale the bucket updates take. None when
        clipping is off."""
        if self._max_grad_norm is None:
            return None
        loose = [p for g in self.param_groups for p in self._loose_params(g)]
        if self._flat_pairs:
            device = self._flat_pairs[0][0].device
        else:
            device = self.param_groups[0]["params"][0].device
        if self._clip_segments is None \
                or self._clip_partials.device != device:
            self._bind_clip_buffers(device)
        partials = self._clip_partials
        if self._flat_pairs is not None:
            for (lo, hi), (_, flat_grad) in zip(self._clip_segments,
                                                self._flat_pairs):
                ops.grad_sumsq_flat_(flat_grad, partials[lo:hi])
        # the trailing slot: the loose parameters' sum of squares; zero
        # from the allocation on, so a fully bucketed model never writes it
        if loose:
            partials[-1:].copy_(torch.stack(
                [p.grad.double().square().sum().to(device)
                 for p in loose]).sum(0, keepdim=True))
            self._loose_slot_used = True
        elif self._loose_slot_used:
            partials[-1:].zero_()
            self._loose_slot_used = False
        ops.clip_coef_(partials, self._clip_state, self._max_grad_norm)
        self._clipped = True
        scale = self._clip_state[1:2]
        for p in loose:
            # the 1-ELEMENT view, not the 0-dim one: torch's type promotion
            # would cast a 0-dim coefficient to a bf16 gradient's dtype
            # before the multiply; this way it is the fp32 product rounded
            # once, as in the bucket kernels
            s = scale.to(p.grad.device)
            p.grad.mul_(s if p.grad.dim() else s[0])
        return scale

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
        if self._max_grad_norm is not None and self._flat_pairs:
            self._bind_clip_buffers(self._flat_pairs[0][0].device)
        else:
            self._clip_segments = None  # bound by the first clipped step

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
