"""FusedSGD: torch.optim.SGD's update (momentum, weight decay, nesterov; no
dampening) fused over the reducer's flat buckets when the model is
engine-wrapped. With the defaults it is the momentum-less SGD matching the
reference's torch.optim.SGD(lr=1e-3) (single_gpu.py:51).

- Bucketed params (marked by the Reducer): ONE hand-written HIP kernel per
  bucket does the update AND zeroes the flat grad (SURVEY §2.2 N8+N9 —
  optimizer.step + zero_grad in one launch). momentum == weight_decay == 0
  runs `k_sgd_flat` (p -= lr*g) and allocates no state; anything else
  runs `k_sgd_momentum_flat`, its momentum buffer a flat fp32 buffer per
  bucket. Both are in ops/csrc/optim_kernels.hip.
- Un-bucketed params: the same formula per parameter (CPU plumbing path
  and models trained without the DDP engine).

`state_dict()` interchanges with torch.optim.SGD over the same parameters
(`momentum_buffer`, here always fp32). `max_grad_norm` clips by the global
L2 norm inside the step (flat_optim.py): the clip coefficient is folded into
the same bucket kernels. Limits: see flat_optim.py — single param_group when
attached, host-scalar lr, no fp32 master weights for bf16; clipping by the
global L2 norm only (no other norm, no error_if_nonfinite), and
`max_grad_norm` is not part of `state_dict()`.
"""

from __future__ import annotations

from typing import Iterable, Optional

import torch

from .. import ops
from .flat_optim import FlatBucketOptimizer


class FusedSGD(FlatBucketOptimizer):
    _state_keys = ("momentum_buffer",)

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float,
                 momentum: float = 0, dampening: float = 0,
                 weight_decay: float = 0, nesterov: bool = False,
                 max_grad_norm: Optional[float] = None):
        if lr <= 0:
            raise ValueError(f"invalid lr {lr}")
        if momentum < 0:
            raise ValueError(f"invalid momentum {momentum}")
        if weight_decay < 0:
            raise ValueError(f"invalid weight_decay {weight_decay}")
        if dampening != 0:
            raise ValueError("FusedSGD does not support dampening "
                             f"(got {dampening}); use torch.optim.SGD")
        if nesterov and momentum <= 0:
            raise ValueError(
                "Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum,
                                      dampening=dampening,
                                      weight_decay=weight_decay,
                                      nesterov=nesterov),
                         max_grad_norm=max_grad_norm)

    def _stateful(self) -> bool:
        return any(g["momentum"] != 0 for g in self.param_groups)

    def _check_hyper(self) -> None:
        for g in self.param_groups:
            if g.get("dampening", 0) != 0:
                raise ValueError("FusedSGD does not support dampening")
            if g.get("maximize", False):
                raise ValueError("FusedSGD does not support maximize")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_fenced()
        scale = self._clip()  # loose grads are scaled in place there
        for group in self.param_groups:
            lr, mu = group["lr"], group["momentum"]
            wd, nesterov = group["weight_decay"], group["nesterov"]
            if mu == 0 and wd == 0:
                # the reference's plain SGD: one k_sgd_flat per bucket
                if self._flat_pairs is not None:
                    for flat_param, flat_grad in self._flat_pairs:
                        ops.sgd_flat_(flat_param, flat_grad, lr,
                                      zero_grad=True, grad_scale=scale)
                for p in self._loose_params(group):
                    p.add_(p.grad, alpha=-lr)
                continue
            if self._flat_pairs is not None:
                if mu != 0 and "momentum_buffer" not in self._flat_state:
                    # momentum switched on after the attach
                    self._bind_flat_state()
                bufs = self._flat_state.get("momentum_buffer")
                for bi, (flat_param, flat_grad) in enumerate(self._flat_pairs):
                    ops.sgd_momentum_flat_(
                        flat_param, flat_grad,
                        bufs[bi] if mu != 0 else None, lr, mu, wd, nesterov,
                        zero_grad=True, grad_scale=scale)
            for p in self._loose_params(group):
                buf = self._param_state(p)["momentum_buffer"] \
                    if mu != 0 else None
                ops.sgd_momentum_reference_(p, p.grad, buf, lr, mu, wd,
                                            nesterov)
        return loss
