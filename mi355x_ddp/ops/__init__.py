"""Python dispatch layer over the MI355X native kernel pack.

Every op has two paths:
- device tensors -> the hand-written CDNA4 HIP kernels in `mi355x_ddp._C`
  (MFMA-tiled linear, CE/MSE, fused SGD / momentum SGD / AdamW, global
  grad-norm clipping, bucket copies). If the extension
  is missing on a GPU host this layer raises — there is NO silent eager
  fallback on the GPU.
- CPU tensors -> plain PyTorch reference implementations, used by the
  CPU-only test tier (gloo, world_size>1) and the single_gpu CPU plumbing
  config (BASELINE.json config 1).

The CPU implementations double as the numerics references the GPU kernels
are tested against (tests/test_kernels_gpu.py).
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is None and _EXT_ERR is None:
        try:
            from mi355x_ddp import _C  # built in-tree by setup.py build_ext --inplace
            _EXT = _C
        except ImportError as e:  # pragma: no cover
            _EXT_ERR = str(e)
    return _EXT


def ext():
    """The native extension; raises loudly if unavailable."""
    m = _load_ext()
    if m is None:
        raise RuntimeError(
            "mi355x_ddp._C native extension is not built — run "
            "`python setup.py build_ext --inplace` (hipcc, gfx950). "
            f"Import error: {_EXT_ERR}")
    return m


def has_ext() -> bool:
    return _load_ext() is not None


# ---------------------------------------------------------------------------
# Linear (reference model: torch.nn.Linear(20,1), single_gpu.py:50)
# ---------------------------------------------------------------------------
def _library_gemm_shape(k: int, n: int) -> bool:
    """Plain library-GEMM territory (north star: hipBLASLt/rocBLAS only
    for plain library GEMMs): measured crossover on MI355X —
    32x2048@2048x1000 runs ~1.8x faster through rocBLAS, while our MFMA
    kernels win up to ~256x256 contractions (profiles/kernel_bench).
    The dispatch itself lives in C++ now (csrc/autograd_ops.hip
    library_gemm_shape — keep the two in sync); this mirror is the
    documented constant and is used by tests."""
    return k * n >= (1 << 20)


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None):
    """y = x @ w^T + b with hand-written MFMA kernels.
    Forward and dX route to rocBLAS for library-sized shapes; dW+db always
    use the fused hand kernel (measured ~3.8x faster than the two-op
    torch equivalent on the ResNet FC shape). The autograd Function lives
    in C++ (csrc/autograd_ops.hip) so the backward chain never re-enters
    Python — the dominant cost of the round-1 generic path."""
    if x.is_cuda:
        if torch.is_autocast_enabled("cuda"):
            # nn.Linear's autocast policy: run the matmul in the autocast
            # dtype (mixed-precision resnet/bf16 stage). Without this, a
            # bf16 activation meeting an fp32 weight is a dtype error.
            dt = torch.get_autocast_dtype("cuda")
            x, w = x.to(dt), w.to(dt)
            b = b.to(dt) if b is not None else None
        if x.dim() != 2:
            # nn.Linear semantics for arbitrary leading dims: flatten to
            # the kernels' 2-D contract, restore after (reshape is
            # autograd-transparent)
            lead = x.shape[:-1]
            y = ext().linear_autograd(x.reshape(-1, x.shape[-1]), w, b)
            return y.reshape(*lead, w.shape[0])
        return ext().linear_autograd(x, w, b)
    return F.linear(x, w, b)


# ---------------------------------------------------------------------------
# Losses (reference: CE at single_gpu.py:24, MSE at multinode_torchrun.py:46;
# both take float probability/value targets of the same shape as the output)
# ---------------------------------------------------------------------------
def cross_entropy(output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """torch.nn.CrossEntropyLoss()(output, target): probability targets
    (the reference's usage — float targets of the output's shape) AND the
    common class-INDEX form (integer targets of shape [B]), which torch
    dispatches on dtype; index targets run the same kernels through their
    exact one-hot probability equivalent.

    Note the reference's toy case is degenerate (C=1 -> loss == 0, grads
    == 0; SURVEY §2.1 'Degenerate loss') — both paths reproduce torch's
    exact semantics for it.
    """
    if output.is_cuda and torch.is_autocast_enabled("cuda") \
            and output.dtype != torch.float32:
        # torch's autocast policy runs losses in fp32; match it so the
        # mixed-precision (bf16-autocast) stage keeps fp32 loss numerics
        output = output.float()
    if not target.is_floating_point():
        if (target < 0).any():
            # torch maps negative indices to ignore_index semantics
            # (default -100: skip the sample, renormalize the mean). The
            # GPU kernels don't implement that, and letting the CPU
            # fallback silently honor it would make the two paths diverge
            # on identical inputs — reject on BOTH instead.
            raise ValueError(
                "mi355x_ddp.ops.cross_entropy: negative class indices "
                "(torch's ignore_index) are not supported; filter ignored "
                "samples out before the loss")
        if output.is_cuda:
            t = F.one_hot(target.long(), output.shape[-1]).to(output.dtype)
            return ext().ce_autograd(output, t)
        return F.cross_entropy(output, target)
    if output.is_cuda:
        return ext().ce_autograd(output, target.to(output.dtype))
    return F.cross_entropy(output, target.to(output.dtype))


def mse_loss(output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    if output.is_cuda:
        if torch.is_autocast_enabled("cuda") \
                and output.dtype != torch.float32:
            output = output.float()  # autocast loss policy: fp32
        return ext().mse_autograd(output, target.to(output.dtype))
    return F.mse_loss(output, target.to(output.dtype))


# ---------------------------------------------------------------------------
# Flat-bucket primitives used by the reducer / fused optimizer
# ---------------------------------------------------------------------------
_SUMSQ_THREADS, _SUMSQ_MAX_BLOCKS = 256, 2048  # optim_kernels.hip


def sumsq_slots(numel: int) -> int:
    """How many float64 partials `grad_sumsq_flat_` writes for a bucket of
    `numel` elements: one per block of k_sumsq_flat's grid."""
    if numel < 0 or numel % 4:
        raise ValueError("sumsq_slots: bucket length must be padded to a "
                         "multiple of 4")
    blocks = (numel // 4 + _SUMSQ_THREADS - 1) // _SUMSQ_THREADS
    return min(max(blocks, 1), _SUMSQ_MAX_BLOCKS)


def grad_sumsq_flat_(grad_flat: torch.Tensor, partials: torch.Tensor) -> None:
    """Sum of squares of one flat gradient bucket, as `sumsq_slots(numel)`
    float64 partial sums written into `partials` (usually a slice of the
    optimizer's buffer). Every slot is overwritten on every call; their sum
    is the bucket's contribution to the squared global L2 norm. fp32 or
    bf16 gradients; a lane squares and adds in fp32, the rest is float64.

    The CPU mirror puts the whole float64 sum into slot 0 and zeros into
    the rest."""
    if partials.dtype != torch.float64 \
            or partials.numel() != sumsq_slots(grad_flat.numel()):
        raise ValueError("grad_sumsq_flat_: partials must be float64 with "
                         "exactly sumsq_slots(numel) elements")
    if grad_flat.is_cuda:
        ext().grad_sumsq_flat(grad_flat, partials)
        return
    partials.zero_()
    partials[0] = grad_flat.double().square().sum()


def clip_coef_(partials: torch.Tensor, clip_state: torch.Tensor,
               max_norm: float) -> None:
    """From every bucket's partials (one float64 tensor, summed in a fixed
    order) to `clip_state`, float32[2]:

        clip_state[0] = total_norm = float32(sqrt(sum))
        clip_state[1] = coef = min(1, max_norm / (total_norm + 1e-6))

    the coefficient in torch.nn.utils.clip_grad_norm_'s own fp32 operation
    sequence (a reciprocal, a multiplication, clamp(max=1)), so a NaN norm
    gives a NaN coefficient and an infinite one gives 0. Called once per
    optimizer step after every `grad_sumsq_flat_`; `clip_state[1:2]` is the
    `grad_scale` of the update ops. The CPU mirror evaluates the same
    formula on fp32 tensors."""
    if partials.is_cuda:
        ext().clip_coef(partials, clip_state, max_norm)
        return
    norm = partials.sum().sqrt().to(torch.float32)
    clip_state[0] = norm
    clip_state[1] = torch.clamp((norm + 1e-6).reciprocal() * max_norm,
                                max=1.0)


def _scaled(g: torch.Tensor, grad_scale: torch.Tensor) -> torch.Tensor:
    """What grad.mul_(coef) would have stored, without storing it."""
    return (g.float() * grad_scale).to(g.dtype)


def sgd_flat_(param_flat: torch.Tensor, grad_flat: torch.Tensor, lr: float,
              zero_grad: bool = True,
              grad_scale: Optional[torch.Tensor] = None) -> None:
    """p -= lr*g over a flat bucket, grad zeroing folded in (SURVEY N8+N9).

    `grad_scale` (here and in the two stateful updates below): a float32
    tensor of 1 element on the bucket's device, the clip coefficient from
    `clip_coef_`. The update then uses g * grad_scale, one fp32 multiply
    (for bf16 rounded to bf16 and widened again: what `grad.mul_(coef)`
    would have stored). The scaled value is NOT written back: with
    zero_grad the gradient is zeroed, with zero_grad=False it is left
    UNSCALED."""
    if param_flat.is_cuda:
        ext().sgd_flat(param_flat, grad_flat, lr, zero_grad, grad_scale)
    else:
        g = grad_flat if grad_scale is None else _scaled(grad_flat, grad_scale)
        param_flat.add_(g, alpha=-lr)
        if zero_grad:
            grad_flat.zero_()


def _expand_mask(decay_mask: torch.Tensor, numel: int) -> torch.Tensor:
    """One byte per 4-element group -> one bool per element."""
    return decay_mask.to(torch.bool).repeat_interleave(4)[:numel]


def sgd_momentum_flat_(param_flat: torch.Tensor, grad_flat: torch.Tensor,
                       buf: Optional[torch.Tensor], lr: float,
                       momentum: float = 0.0, weight_decay: float = 0.0,
                       nesterov: bool = False,
                       zero_grad: bool = True,
                       grad_scale: Optional[torch.Tensor] = None) -> None:
    """torch.optim.SGD's update (no dampening) over a flat bucket, grad
    zeroing folded in:

        d = g + wd*p;  buf = mu*buf + d;  d = nesterov ? d + mu*buf : buf
        p -= lr*d;     g = 0 when zero_grad

    `buf` is fp32 whatever the parameter dtype and starts at zero, which
    reproduces torch's first-step `buf = d` with no step count. `buf=None`
    requires momentum 0 (weight decay only). bf16 parameters: arithmetic in
    fp32, ONE round-to-nearest on the parameter store; there are no fp32
    master weights (as with sgd_flat_). `grad_scale`: see sgd_flat_.

    The CPU path is the same operation sequence as torch's single-tensor
    SGD, in fp32; it is the numerics reference for the kernel."""
    if buf is None and (momentum != 0 or nesterov):
        raise ValueError("sgd_momentum_flat_: momentum needs a buffer")
    if param_flat.is_cuda:
        ext().sgd_momentum_flat(param_flat, grad_flat, buf, lr, momentum,
                                weight_decay, nesterov, zero_grad, grad_scale)
        return
    g = grad_flat if grad_scale is None else _scaled(grad_flat, grad_scale)
    sgd_momentum_reference_(param_flat, g, buf, lr, momentum,
                            weight_decay, nesterov)
    if zero_grad:
        grad_flat.zero_()


def sgd_momentum_reference_(p: torch.Tensor, g: torch.Tensor,
                            buf: Optional[torch.Tensor], lr: float,
                            momentum: float, weight_decay: float,
                            nesterov: bool) -> None:
    """The momentum-SGD update in plain torch ops, fp32 arithmetic, any
    shape and device: torch's single-tensor SGD operation for operation."""
    low = p.dtype != torch.float32
    pf = p.float() if low else p
    d = g.float() if low else g
    if weight_decay != 0:
        d = d.add(pf, alpha=weight_decay)
    if buf is not None:
        buf.mul_(momentum).add_(d)
        d = d.add(buf, alpha=momentum) if nesterov else buf
    pf.add_(d, alpha=-lr)
    if low:
        p.copy_(pf)


def adamw_tick_(step_state: torch.Tensor, lr: float, beta1: float,
                beta2: float) -> None:
    """Advance the optimizer's step count by one: `step_state` is int32[4],
    [0] the count t, [1]/[2] the fp32 bits of -(lr/(1-beta1^t)) and
    1/sqrt(1-beta2^t) that `adamw_flat_` reads on the device. Called ONCE per
    optimizer step, ahead of the per-bucket updates; on the GPU it is a
    one-thread kernel, so a captured graph advances the count on replay."""
    if step_state.is_cuda:
        ext().adamw_tick(step_state, lr, beta1, beta2)
    else:
        step_state[0] += 1


def adamw_flat_(param_flat: torch.Tensor, grad_flat: torch.Tensor,
                exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                step, lr: float, beta1: float, beta2: float, eps: float,
                weight_decay: float,
                decay_mask: Optional[torch.Tensor] = None,
                zero_grad: bool = True,
                grad_scale: Optional[torch.Tensor] = None) -> None:
    """torch.optim.AdamW's update over a flat bucket at step count t, grad
    zeroing folded in:

        p *= 1 - lr*wd                     (where decay_mask allows)
        m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
        p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)

    weight_decay=0 is plain Adam. `decay_mask` is uint8 with one byte per
    4-element group (the reducer aligns every parameter to 4 elements, so a
    group never straddles two); a zero byte exempts the group from decay.
    State is fp32 whatever the parameter dtype. bf16 parameters: arithmetic
    in fp32, ONE round-to-nearest on the parameter store; there are no fp32
    master weights. `grad_scale`: see sgd_flat_.

    `step`: on the GPU the int32 device tensor that `adamw_tick_` has
    ALREADY advanced for this step (the kernel never sees a host count, so
    the step is graph-capturable); on the CPU a Python int, the t of this
    step. The CPU path is the same operation sequence as torch's
    single-tensor AdamW on the CPU, in fp32; it is the numerics reference
    for the kernel, which follows torch's DEVICE kernels instead (three
    roundings placed differently: a few ulps)."""
    if param_flat.is_cuda:
        ext().adamw_flat(param_flat, grad_flat, exp_avg, exp_avg_sq, step,
                         lr, beta1, beta2, eps, weight_decay, decay_mask,
                         zero_grad, grad_scale)
        return
    g = grad_flat if grad_scale is None else _scaled(grad_flat, grad_scale)
    adamw_reference_(param_flat, g, exp_avg, exp_avg_sq, int(step),
                     lr, beta1, beta2, eps, weight_decay,
                     None if decay_mask is None
                     else _expand_mask(decay_mask, param_flat.numel()))
    if zero_grad:
        grad_flat.zero_()


def adamw_reference_(p: torch.Tensor, g: torch.Tensor, exp_avg: torch.Tensor,
                     exp_avg_sq: torch.Tensor, t: int, lr: float,
                     beta1: float, beta2: float, eps: float,
                     weight_decay: float,
                     decays: Optional[torch.Tensor] = None) -> None:
    """The AdamW update at step count t in plain torch ops, fp32
    arithmetic, any shape and device: torch's single-tensor AdamW operation
    for operation. `decays`: optional bool tensor of p's shape, False where
    the weight decay is skipped."""
    low = p.dtype != torch.float32
    pf = p.float() if low else p
    gf = g.float() if low else g
    if weight_decay != 0:
        if decays is None:
            pf.mul_(1 - lr * weight_decay)
        else:
            pf.copy_(torch.where(decays, pf * (1 - lr * weight_decay), pf))
    exp_avg.lerp_(gf, 1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    step_size = lr / (1 - beta1 ** t)
    denom = (exp_avg_sq.sqrt() / (1 - beta2 ** t) ** 0.5).add_(eps)
    pf.addcdiv_(exp_avg, denom, value=-step_size)
    if low:
        p.copy_(pf)


def perm_index(seed: int, p: int, n: int) -> int:
    """Python mirror of the kernel's seeded bijection on [0, n)
    (kernels.hip `mix_bijection`/`shard_consts`): source row for shard
    position p at epoch seed `seed`. Used by tests and the CPU data path."""
    M = 0xFFFFFFFF
    z = (seed * 0x9E3779B9 + 0x7F4A7C15) & M
    z ^= z >> 15
    z = (z * 0x2C1B3C6D) & M
    z ^= z >> 12
    c0, m0 = z, ((z >> 8) | 1) & M
    z = (z * 0x297A2D39 + 0x68E31DA4) & M
    z ^= z >> 16
    c1, m1 = z, ((z >> 7) | 1) & M
    k_mask = 1
    while k_mask + 1 < n:
        k_mask = (k_mask << 1) | 1
    x = p
    while True:
        x = (x + c0) & k_mask
        x = (x * m0) & k_mask
        x ^= x >> 3
        x = (x + c1) & k_mask
        x = (x * m1) & k_mask
        x ^= x >> 5
        if x < n:
            return x


def cpu_linear_bwd_weight(x, dy, dw, db, accumulate=False):
    """CPU reference for the bwd-weight kernel (used in numerics tests)."""
    w_new = dy.t() @ x
    b_new = dy.sum(dim=0)
    if accumulate:
        dw += w_new
        db += b_new
    else:
        dw.copy_(w_new)
        db.copy_(b_new)
