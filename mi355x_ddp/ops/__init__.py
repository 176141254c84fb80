"""Python dispatch layer over the MI355X native kernel pack.

Every op has two paths:
- device tensors -> the hand-written CDNA4 HIP kernels in `mi355x_ddp._C`
  (MFMA-tiled linear, the tiled-GEMM MLP, CE/MSE, the class-index
  cross-entropy with label smoothing and ignore_index, fused SGD / momentum
  SGD / AdamW, global grad-norm clipping, bucket copies). If the extension
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
# Linear -> GELU (-> Linear) on the tiled GEMMs (csrc/gemm_kernels.hip)
# ---------------------------------------------------------------------------
def _gemm_operands(x, *params):
    """x flattened to rows, everything contiguous (a no-op for parameters as
    nn.Linear holds them) and in the autocast dtype under autocast
    (nn.Linear's policy, as `linear` does)."""
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        x, params = x.to(dt), tuple(p.to(dt) for p in params)
    return (x.reshape(-1, x.shape[-1]).contiguous(),) \
        + tuple(p.contiguous() for p in params)


def mlp(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
        w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """linear(gelu(linear(x, w1, b1)), w2, b2) with exact (erf) GELU: the
    transformer MLP. On the GPU it is six launches of one LDS-tiled MFMA GEMM
    kernel, two forward and four backward; both bias adds, GELU, the
    multiplication by GELU' and both bias gradients ride in the GEMMs'
    epilogues, so no elementwise kernel runs. Every feature dimension must be
    a multiple of 16, the dtype fp32 or bf16 (other inputs raise); leading
    dimensions are flattened and restored. GELU is applied to the linear
    output as stored (rounded to bf16 under bf16), as torch does; weight and
    bias gradients are the same bits run to run. The CPU path is the formula
    in plain torch ops."""
    if x.is_cuda:
        lead = x.shape[:-1]
        y = ext().mlp_autograd(*_gemm_operands(x, w1, b1, w2, b2))
        return y.reshape(*lead, w2.shape[0])
    return F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)


def linear_gelu(x: torch.Tensor, w: torch.Tensor,
                b: torch.Tensor) -> torch.Tensor:
    """gelu(linear(x, w, b)), the first half of `mlp` on its own: the bias add
    and GELU in the forward GEMM's epilogue. Shapes and dtypes as `mlp`."""
    if x.is_cuda:
        lead = x.shape[:-1]
        y = ext().linear_gelu_autograd(*_gemm_operands(x, w, b))
        return y.reshape(*lead, w.shape[0])
    return F.gelu(F.linear(x, w, b))


# ---------------------------------------------------------------------------
# Fused self-attention (csrc/attention_kernels.hip)
# ---------------------------------------------------------------------------
def self_attention(qkv: torch.Tensor, heads: int,
                   matrix: str = "f32") -> torch.Tensor:
    """softmax(Q K^T / sqrt(D)) V per head, on the packed in-projection
    output: `qkv` is [B, N, 3*E] with columns [0,E) Q, [E,2E) K, [2E,3E) V
    and head h at columns h*D.. of each (E = heads*D); the result is
    [B, N, E], ready for the out-projection. No mask, no dropout.

    On the GPU, forward and backward, any N up to 4096 (D in 16/32/64, fp32
    or bf16 storage, fp32 arithmetic); other shapes raise. Up to 64 tokens
    one workgroup per (batch, head) runs the whole head out of LDS; above,
    the tiled kernels walk the keys in blocks of 64 with an online softmax
    and the backward additionally keeps the output. Under autocast the input
    is cast to the autocast dtype, as `linear` does.

    `matrix` names the matrix instruction of the five products. "f32" (the
    default) is the exact-fp32 path above, whatever the storage.
    "bf16" runs them on the wide bf16 MFMA for every N up to 4096 (D 32 or
    64): it needs bf16 `qkv` (after the autocast cast; anything else raises
    ValueError), keeps the softmax, the statistics and every accumulator in
    fp32 and rounds P and dS to bf16 once, on their way into the second
    product. The CPU path is the formula in plain torch ops, the kernels'
    mirror, for either value."""
    if matrix not in ("f32", "bf16"):
        raise ValueError(f"self_attention: matrix must be 'f32' or 'bf16', "
                         f"got {matrix!r}")
    if qkv.is_cuda:
        if torch.is_autocast_enabled("cuda"):
            qkv = qkv.to(torch.get_autocast_dtype("cuda"))
        if matrix == "bf16" and qkv.dtype != torch.bfloat16:
            raise ValueError(f"self_attention: matrix='bf16' needs bf16 qkv "
                             f"(or bf16 autocast), got {qkv.dtype}")
        return ext().attention_autograd(qkv, heads, matrix)
    B, N, E3 = qkv.shape
    if heads < 1 or E3 % (3 * heads):
        raise ValueError("self_attention: the last dimension must be "
                         "3 * heads * D")
    D = E3 // (3 * heads)
    q, k, v = qkv.view(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, N, heads * D)


# ---------------------------------------------------------------------------
# Fused LayerNorm, with or without the residual add (csrc/layernorm_kernels.hip)
# ---------------------------------------------------------------------------
def _ln_operands(*tensors):
    """Contiguous device operands; float32 under autocast (torch's own policy
    for layer_norm, as `cross_entropy` does for the losses)."""
    if torch.is_autocast_enabled("cuda"):
        tensors = tuple(t.float() for t in tensors)
    return (tensors[0].contiguous(),) + tuple(tensors[1:])


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    """F.layer_norm over the last dimension. On the GPU one wave normalises
    one row out of registers, forward and backward (last dimension a multiple
    of 4 up to 2048, fp32 or bf16 storage alike for all operands, fp32
    arithmetic; other shapes raise). The weight and bias gradients are summed
    in a fixed order without atomics: run to run the same bits."""
    if x.is_cuda:
        x, weight, bias = _ln_operands(x, weight, bias)
        return ext().layer_norm_autograd(x, weight, bias, eps)
    return F.layer_norm(x, x.shape[-1:], weight, bias, eps)


def add_layer_norm(x: torch.Tensor, residual: torch.Tensor,
                   weight: torch.Tensor, bias: torch.Tensor,
                   eps: float = 1e-5):
    """(s, y) with s = x + residual and y = layer_norm(s): the residual add
    folded into the LayerNorm that follows it, one pass over the rows forward
    and one backward. `s` is rounded to the storage dtype and `y` is computed
    from that rounded `s`. Shapes and dtypes as `layer_norm`."""
    if x.is_cuda:
        x, residual, weight, bias = _ln_operands(x, residual, weight, bias)
        s, y = ext().add_layer_norm_autograd(x, residual.contiguous(), weight,
                                             bias, eps)
        return s, y
    s = x + residual
    return s, F.layer_norm(s, s.shape[-1:], weight, bias, eps)


# ---------------------------------------------------------------------------
# Fused BatchNorm (+ residual add) (+ ReLU) (csrc/batchnorm_kernels.hip)
# ---------------------------------------------------------------------------
def batch_norm_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                   running_mean: torch.Tensor, running_var: torch.Tensor, *,
                   residual: Optional[torch.Tensor] = None, act: str = "relu",
                   training: bool = True, momentum: float = 0.1,
                   eps: float = 1e-5,
                   num_batches_tracked: Optional[torch.Tensor] = None):
    """z = act(batch_norm(x) + residual) over the channel dimension, `act`
    "relu" or "none", `residual` optional and only with "relu": BN, BN+ReLU
    and BN+add+ReLU, each three launches forward and three backward on the
    GPU, with the ReLU mask read back from the saved output.

    `x` is [R, C] (channels last) or [N, C, H, W]. A 4-D input is used in its
    channels-last form: a view when it already is channels-last, otherwise
    ONE `.contiguous(memory_format=torch.channels_last)` copy (and one of the
    residual); the 4-D result is channels-last. C must be a multiple of 4 up
    to 4096, the storage fp32 or bf16 (other inputs raise), the arithmetic is
    fp32. Under autocast `x` and `residual` keep their dtype (torch's policy
    for batch norm, unlike `layer_norm`); `weight`, `bias` and the running
    statistics go to the kernels as fp32.

    In training the batch statistics are used, `running_mean`/`running_var`
    are updated in place (unbiased variance, `(1-momentum)*old +
    momentum*new`) and `num_batches_tracked`, when given, is incremented on
    the device by the same launch, so a captured step needs none of its own.
    With `training=False` the running statistics are used in one launch;
    gradients are then not supported and asking for them raises. Statistics
    and the weight and bias gradients are summed in a fixed order without
    atomics: run to run the same bits. The CPU path is F.batch_norm, add,
    relu."""
    if act not in ("relu", "none"):
        raise ValueError(f"batch_norm_act: act must be 'relu' or 'none', "
                         f"got {act!r}")
    if residual is not None and act != "relu":
        raise ValueError("batch_norm_act: a residual needs act='relu'")
    if x.dim() not in (2, 4):
        raise ValueError(f"batch_norm_act: x must be [R, C] or [N, C, H, W], "
                         f"got {tuple(x.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"batch_norm_act: residual {tuple(residual.shape)} "
                         f"does not match x {tuple(x.shape)}")
    if not x.is_cuda:
        y = F.batch_norm(x, running_mean, running_var, weight, bias, training,
                         momentum, eps)
        if training and num_batches_tracked is not None:
            num_batches_tracked += 1
        if residual is not None:
            y = y + residual
        return F.relu(y) if act == "relu" else y

    def rows(t):
        if t.dim() == 2:
            return t.contiguous()
        t = t.contiguous(memory_format=torch.channels_last)
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()

    rm, rv = running_mean.float(), running_var.float()
    z = ext().batch_norm_act_autograd(
        rows(x), weight.float(), bias.float(), rm, rv,
        None if residual is None else rows(residual), act == "relu", training,
        momentum, eps, num_batches_tracked)
    if training and running_mean.dtype != torch.float32:  # rm, rv are copies
        running_mean.copy_(rm), running_var.copy_(rv)
    if x.dim() == 2:
        return z
    N, C, H, W = x.shape
    return z.view(N, H, W, C).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------
# Implicit-GEMM convolutions, 1x1 and 3x3 (csrc/conv_kernels.hip)
# ---------------------------------------------------------------------------
def conv_check_args(x: torch.Tensor, weight: torch.Tensor, stride: int,
                    padding: Optional[int]) -> None:
    """Every rule of `conv2d`, ahead of any launch; raises ValueError. The
    rules hold on either device, except that the CPU path also takes dtypes
    other than fp32 and bf16 (it serves the fp64 references) and has no
    alignment rule."""
    who = "conv2d"
    if x.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"{who}: x must be [N, Cin, H, W] and weight "
                         f"[Cout, Cin, k, k], got {tuple(x.shape)} and "
                         f"{tuple(weight.shape)}")
    cout, cin, k, k2 = weight.shape
    if k != k2 or k not in (1, 3):
        raise ValueError(f"{who}: kernel size must be 1x1 or 3x3, got "
                         f"{k}x{k2}")
    if padding is not None and padding != k // 2:
        raise ValueError(f"{who}: padding must be k//2 = {k // 2}, got "
                         f"{padding}")
    if stride not in (1, 2):
        raise ValueError(f"{who}: stride must be 1 or 2, got {stride}")
    if x.shape[1] != cin:
        raise ValueError(f"{who}: x has {x.shape[1]} channels, weight takes "
                         f"{cin} (groups are not supported)")
    if cin % 16 or cout % 16 or cin == 0 or cout == 0:
        raise ValueError(f"{who}: Cin and Cout must be multiples of 16, got "
                         f"{cin} and {cout}")
    dt = _conv_dtype(x)  # under autocast both operands are cast to it
    if (dt or x.dtype) != (dt or weight.dtype) or x.device != weight.device:
        raise ValueError(f"{who}: x is {x.dtype} on {x.device}, weight "
                         f"{weight.dtype} on {weight.device}")
    n, _, h, w = x.shape
    if h < 1 or w < 1 or n * h * w >= 2 ** 31:
        raise ValueError(f"{who}: H, W >= 1 and N*H*W < 2^31, got "
                         f"{tuple(x.shape)}")
    if x.is_cuda:
        if (dt or x.dtype) not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{who}: dtype must be float32 or bfloat16, got "
                             f"{dt or x.dtype}")
        # only storage the kernels read in place has to be aligned: a cast,
        # a layout change and the 3x3 packing each give a fresh allocation
        x_view = x.dtype == (dt or x.dtype) and \
            x.is_contiguous(memory_format=torch.channels_last)
        w_view = k == 1 and weight.dtype == (dt or x.dtype) and \
            weight.is_contiguous()
        if (x_view and x.data_ptr() % 16) or \
                (w_view and weight.data_ptr() % 16):
            raise ValueError(f"{who}: x and weight must be 16-byte aligned "
                             f"where they are read in place")


def conv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1,
           padding: Optional[int] = None) -> torch.Tensor:
    """F.conv2d(x, weight, None, stride, k//2) for the 1x1 and 3x3
    convolutions of a ResNet, forward and backward on implicit-GEMM MFMA
    kernels of our own.

    `x` is [N, Cin, H, W], `weight` [Cout, Cin, k, k] with k 1 or 3, `stride`
    1 or 2, `padding` k//2 (the default; anything else raises), no bias, no
    groups, no dilation. Cin and Cout must be multiples of 16, the dtype fp32
    or bf16 alike for both, N*H*W below 2^31; `conv_check_args` raises
    ValueError for everything else before anything is launched. Under
    autocast both operands are used in the autocast dtype (nn.Conv2d's
    policy, as `linear` does).

    On the GPU `x` is used in its channels-last form, as `batch_norm_act`
    does: a view when it already is channels-last, otherwise ONE
    `.contiguous(memory_format=torch.channels_last)` copy; the result is the
    channels-last [N, Cout, Ho, Wo] view of the kernels' [N*Ho*Wo, Cout]
    matrix, Ho = (H + 2*(k//2) - k)//stride + 1. The kernels read the weight
    packed as [Cout, k*k, Cin]: one small copy per call (a view for k = 1),
    folded into the autocast cast where there is one. The weight gradient is
    stored by the kernels in `weight`'s own layout and dtype and is the same
    bits run to run (no atomics). Nothing is read back to the host, so the
    call and its backward can be captured into a graph; as for any captured
    backward, `x` and `weight` must not carry an AccumulateGrad node made on
    another stream and still held by an earlier autograd graph (fresh leaves,
    or nothing retained from a run outside the capture: docs/KERNELS.md).
    The CPU path is F.conv2d."""
    conv_check_args(x, weight, stride, padding)
    k = weight.shape[-1]
    if not x.is_cuda:
        return F.conv2d(x, weight, None, stride, k // 2)
    dt = _conv_dtype(x) or x.dtype
    cout, cin = weight.shape[:2]
    n, _, h, w = x.shape
    # the packed copy takes no gradient: dW goes to `weight` from the kernels
    wp = weight.detach().permute(0, 2, 3, 1).reshape(cout, k * k, cin) \
        .to(dt).contiguous()
    xc = x.to(dt).contiguous(memory_format=torch.channels_last)
    rows = xc.permute(0, 2, 3, 1).reshape(-1, cin).contiguous()
    y = ext().conv2d_autograd(rows, weight.contiguous(), wp, n, h, w, stride)
    ho = (h + 2 * (k // 2) - k) // stride + 1
    wo = (w + 2 * (k // 2) - k) // stride + 1
    return y.view(n, ho, wo, cout).permute(0, 3, 1, 2)


def _conv_dtype(x):
    """The autocast dtype where the convolution is cast to one, else None."""
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return None


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


def cross_entropy_index(logits: torch.Tensor, labels: torch.Tensor,
                        label_smoothing: float = 0.0,
                        ignore_index: int = -100,
                        reduction: str = "mean") -> torch.Tensor:
    """F.cross_entropy(logits, labels, label_smoothing=..., ignore_index=...,
    reduction=...) for integer class labels without class weights, on kernels
    of its own (csrc/loss_kernels.hip).

    `logits` is [..., C], fp32 or bf16; `labels` is int64 or int32 with the
    leading shape; `reduction` is "mean", "sum" or "none". The result is fp32:
    a scalar, or the leading shape for "none". Rows whose label is
    `ignore_index` contribute nothing and "mean" divides by the number of the
    others, so with every row ignored it is NaN, as in torch. Other dtypes, a
    device or shape mismatch, `label_smoothing` outside [0, 1] and an unknown
    reduction raise ValueError on either device.

    On the GPU the forward reads the logits once and the backward reads them
    once and stores dlogits once; what is kept between them is two floats per
    row. Under autocast the logits are NOT cast: the kernels widen bf16 on
    load and compute in fp32, which gives the number a cast would give;
    dlogits is rounded once to the logits' dtype. The loss is summed in a
    fixed order without atomics: run to run the same bits. The logits must be
    contiguous after the flatten and their storage 16-byte aligned.

    Nothing is read back to the host, so the call can be captured into a
    graph. The price: a label that is neither `ignore_index` nor in [0, C)
    cannot raise. It is never used as an address; that row's loss and its row
    of dlogits are NaN, the row counts as non-ignored and the other rows'
    gradients are unaffected (torch asserts on the device instead).

    `cross_entropy` keeps its own routing: integer targets given to it still
    go through one-hot probabilities and negative ones still raise. Moving
    that branch here is a later decision. The CPU path is F.cross_entropy."""
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"cross_entropy_index: logits must be float32 or "
                         f"bfloat16, got {logits.dtype}")
    if labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"cross_entropy_index: labels must be int64 or "
                         f"int32, got {labels.dtype}")
    if labels.device != logits.device:
        raise ValueError(f"cross_entropy_index: logits on {logits.device}, "
                         f"labels on {labels.device}")
    if logits.dim() < 1 or logits.shape[-1] < 1 \
            or labels.shape != logits.shape[:-1]:
        raise ValueError(f"cross_entropy_index: labels {tuple(labels.shape)} "
                         f"do not match logits {tuple(logits.shape)}")
    if not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"cross_entropy_index: label_smoothing must be in "
                         f"[0, 1], got {label_smoothing}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"cross_entropy_index: reduction must be 'mean', "
                         f"'sum' or 'none', got {reduction!r}")
    if logits.is_cuda:
        return ext().cei_autograd(logits.contiguous(), labels.contiguous(),
                                  label_smoothing, ignore_index, reduction)
    C = logits.shape[-1]
    loss = F.cross_entropy(logits.reshape(-1, C).float(),
                           labels.reshape(-1).long(),
                           ignore_index=ignore_index, reduction=reduction,
                           label_smoothing=label_smoothing)
    return loss.reshape(labels.shape) if reduction == "none" else loss


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
