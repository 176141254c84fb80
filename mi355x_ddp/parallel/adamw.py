"""FusedAdamW: torch.optim.AdamW's update (decoupled weight decay;
weight_decay=0 is plain Adam) fused over the reducer's flat buckets.

- Bucketed params: one `k_adamw_flat` launch per bucket updates p, exp_avg
  and exp_avg_sq and zeroes the flat grad, preceded by ONE one-thread
  `k_adamw_tick` per step. The step count lives on the device: the tick
  advances it and derives the bias corrections, the bucket kernels only
  read them — so a whole step, count included, captures into a hipGraph
  and replays correctly (torch's default AdamW keeps `step` on the host).
- exp_avg / exp_avg_sq are flat fp32 buffers, one per bucket, allocated by
  attach_reducer; `self.state[p]` holds per-parameter views of them plus
  `step`, a view of the device counter.
- `no_decay_params` (biases, norm weights) are exempt from weight decay
  through a one-byte-per-4-elements mask per bucket.
- Un-bucketed params: the same formula per parameter in plain torch ops.
  That path reads the count back to the host, so it is not capturable.

`state_dict()` interchanges with torch.optim.AdamW over the same
parameters, with two things to know. `no_decay_params` is NOT part of it
(it names parameters, which a state_dict cannot): a FusedAdamW that resumes
must be constructed with the same list, and a single-group torch.optim.AdamW
that loads the dict decays every parameter — give it two param groups to
keep the exemption. And a load writes into the existing flat buffers and the
existing device counter, so a step already captured in a graph keeps
working; a changed `lr` or other hyper-parameter still needs a recapture.
`eps` must be positive: with 0 the zero padding of the buckets would
compute 0/0. `max_grad_norm` clips by the global L2 norm inside the step
(flat_optim.py); within a step the order is clip launches, tick, bucket
kernels. Limits: see flat_optim.py — single param_group when attached,
host-scalar lr (a scheduler needs a recapture under graph capture), no
fp32 master weights for bf16; no amsgrad, no maximize; clipping by the
global L2 norm only (no other norm, no error_if_nonfinite), and
`max_grad_norm`, like `no_decay_params`, is not part of `state_dict()`.
"""

from __future__ import annotations

from typing import Iterable, Optional, Tuple

import torch

from .. import ops
from .flat_optim import FlatBucketOptimizer


class FusedAdamW(FlatBucketOptimizer):
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2,
                 no_decay_params: Optional[Iterable[torch.nn.Parameter]] = None,
                 max_grad_norm: Optional[float] = None):
        if lr <= 0:
            raise ValueError(f"invalid lr {lr}")
        if eps <= 0:
            # eps == 0 would make the buckets' zero padding 0/0 = NaN
            raise ValueError(f"invalid eps {eps}: FusedAdamW needs eps > 0")
        if not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"invalid betas {betas}")
        if weight_decay < 0:
            raise ValueError(f"invalid weight_decay {weight_decay}")
        # torch.optim.AdamW's own group keys, so that a state_dict loads
        # there with the same meaning (decoupled decay above all)
        super().__init__(params, dict(
            lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
            amsgrad=False, maximize=False, foreach=None, capturable=False,
            differentiable=False, fused=None, decoupled_weight_decay=True),
            max_grad_norm=max_grad_norm)
        self._no_decay = {id(p) for p in (no_decay_params or ())}
        self._step_state = None  # int32[4], see ops.adamw_tick_
        self._decay_masks = None

    def _check_hyper(self) -> None:
        for g in self.param_groups:
            if g["eps"] <= 0:
                raise ValueError("FusedAdamW needs eps > 0 (the buckets' "
                                 "zero padding would become 0/0)")
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdamW supports neither amsgrad nor "
                                 "maximize")
            if not g.get("decoupled_weight_decay", True) \
                    and g["weight_decay"] != 0:
                raise ValueError("FusedAdamW decays decoupled (AdamW); an "
                                 "Adam state_dict with L2 weight_decay "
                                 "does not mean the same here")
            g["betas"] = tuple(g["betas"])

    # -- the device-resident step count --------------------------------------
    def _steps(self, device) -> torch.Tensor:
        """The step-state buffer on `device` (parameters may have moved
        since construction: the count moves with them)."""
        ss = self._step_state
        if ss is None or ss.device != device:
            new = torch.zeros(4, dtype=torch.int32, device=device)
            if ss is not None:
                new[0] = int(ss[0])
            self._step_state = ss = new
            for st in self.state.values():
                if "step" in st:
                    st["step"] = ss[0]
        return ss

    def _set_step(self, t: int) -> None:
        dev = self.param_groups[0]["params"][0].device
        self._steps(dev)[0] = int(t)

    def _init_param_state(self, p, st) -> None:
        st["step"] = self._steps(p.device)[0]

    def attach_reducer(self, reducer) -> None:
        super().attach_reducer(reducer)
        self._decay_masks = None
        if not self._no_decay:
            return
        self._decay_masks = []
        for b in reducer.buckets:
            mask = torch.ones(b.numel // 4, dtype=torch.uint8)
            for i, p in enumerate(b.params):
                if id(p) in self._no_decay:
                    lo = b.offsets[i] // 4  # offsets are 4-aligned
                    mask[lo:lo + (p.numel() + 3) // 4] = 0
            self._decay_masks.append(mask.to(b.flat_param.device))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_fenced()
        scale = self._clip()  # loose grads are scaled in place there
        g0 = self.param_groups[0]
        ss = self._steps(g0["params"][0].device)
        # one tick per step, ahead of every bucket update
        ops.adamw_tick_(ss, g0["lr"], *g0["betas"])
        if self._flat_pairs is not None:
            (b1, b2), m, v = g0["betas"], self._flat_state["exp_avg"], \
                self._flat_state["exp_avg_sq"]
            step = ss if ss.is_cuda else int(ss[0])
            for bi, (flat_param, flat_grad) in enumerate(self._flat_pairs):
                ops.adamw_flat_(
                    flat_param, flat_grad, m[bi], v[bi], step, g0["lr"], b1,
                    b2, g0["eps"], g0["weight_decay"],
                    None if self._decay_masks is None
                    else self._decay_masks[bi], zero_grad=True,
                    grad_scale=scale)
        t = None
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in self._loose_params(group):
                if t is None:
                    t = int(ss[0])  # host read-back: this path syncs
                st = self._param_state(p)
                wd = 0.0 if id(p) in self._no_decay \
                    else group["weight_decay"]
                ops.adamw_reference_(p, p.grad, st["exp_avg"],
                                     st["exp_avg_sq"], t, group["lr"], b1,
                                     b2, group["eps"], wd)
        return loss

    # -- state_dict interchange with torch.optim.AdamW -----------------------
    def state_dict(self):
        """torch.optim.AdamW's layout: per parameter `step` (a float32
        scalar tensor on the host, as torch's default AdamW keeps it),
        `exp_avg`, `exp_avg_sq`."""
        sd = super().state_dict()
        if sd["state"]:
            t = torch.tensor(float(0 if self._step_state is None
                                   else int(self._step_state[0])),
                             dtype=torch.float32)
            sd["state"] = {k: {**st, "step": t.clone()}
                           for k, st in sd["state"].items()}
        return sd

    def _adopt_loaded_state(self) -> None:
        steps = [int(float(st["step"])) for st in self.state.values()
                 if "step" in st]
        if steps:
            self._set_step(max(steps))
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = self._steps(p.device)[0]
