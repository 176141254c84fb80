"""Time the fused BatchNorm(+add)+ReLU kernels against the torch path at
ResNet-50's (R, C) shapes at batch 32, forward plus backward through autograd,
f32 and bf16, channels-last:

  bn           ops.batch_norm_act(act="none")  vs  F.batch_norm
  bn_relu      ops.batch_norm_act              vs  F.batch_norm, relu
  bn_add_relu  ops.batch_norm_act(residual=r)  vs  F.batch_norm, add, relu

Device events around `--iters` calls, every version warmed up first, the two
versions alternated inside one process and the pair repeated `--repeats`
times; prints and optionally writes one JSON with the median and the min..max
of the per-call microseconds, and the bytes a call has to move (each operand
and result once per pass that needs it) for rates from a kernel trace.

    python tools/bench_batch_norm.py [--json profiles/batch_norm.json]
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402

SHAPES = [(401408, 64), (100352, 64), (100352, 256), (25088, 128),
          (25088, 512), (6272, 256), (6272, 1024), (1568, 512), (1568, 2048)]
FORMS = {"bn": ("none", False), "bn_relu": ("relu", False),
         "bn_add_relu": ("relu", True)}
DEV = "cuda:0"


def timed(fn, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per call


def compare(pairs, iters, repeats):
    for fn in pairs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in pairs}
    for _ in range(repeats):
        for k, fn in pairs.items():
            samples[k].append(timed(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in samples.items()}


def passes(act, add):
    """Tensor passes of [R, C] a fused call needs: stats x; apply x (res) z;
    reduce dz x (z); bwd apply dz x (z) dx (dres)."""
    relu = act == "relu"
    return 1 + 2 + add + 2 + relu + 3 + relu + add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batch_norm needs a GPU"
    result = {"iters": args.iters, "repeats": args.repeats, "cases": []}
    for (R, C), (dtype, dname) in ((s, d) for s in SHAPES for d in (
            (torch.float32, "f32"), (torch.bfloat16, "bf16"))):
        torch.manual_seed(0)
        x, r = (torch.randn(R, C, device=DEV, dtype=dtype, requires_grad=True)
                for _ in range(2))
        dz = torch.randn(R, C, device=DEV, dtype=dtype)
        w, b = (torch.randn(C, device=DEV, requires_grad=True)
                for _ in range(2))
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        for form, (act, add) in FORMS.items():
            def hip():
                x.grad = r.grad = w.grad = b.grad = None
                ops.batch_norm_act(x, w, b, rm, rv, act=act,
                                   residual=r if add else None).backward(dz)

            def stock():
                x.grad = r.grad = w.grad = b.grad = None
                y = F.batch_norm(x, rm, rv, w, b, True)
                y = y + r if add else y
                (F.relu(y) if act == "relu" else y).backward(dz)

            case = {"R": R, "C": C, "dtype": dname, "form": form,
                    "bytes": passes(act, add) * R * C * x.element_size()}
            case.update(compare({"hip": hip, "torch": stock}, args.iters,
                                args.repeats))
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
