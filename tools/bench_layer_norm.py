"""Time the fused LayerNorm kernels against the torch path at the ViT-L/32
shape (R = 32 * 50 = 1600 rows, E = 1024), forward plus backward including
the weight and bias gradients, f32 and bf16:

  (a) ops.layer_norm      vs  F.layer_norm
  (b) ops.add_layer_norm  vs  x + r followed by F.layer_norm, with a gradient
      arriving at the sum as well as at the normalised output, as in a
      pre-norm block

Device events around `--iters` calls, every version warmed up first, the two
versions alternated inside one process and the pair repeated `--repeats`
times; prints and optionally writes one JSON with the median and the
min..max of the per-call microseconds.

    python tools/bench_layer_norm.py [--json profiles/layer_norm_r12a.json]
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402

B, N, E = 32, 50, 1024
EPS = 1e-6
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
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in pairs}
    for _ in range(repeats):
        for k, fn in pairs.items():
            samples[k].append(timed(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_layer_norm needs a GPU"
    result = {"shape": {"R": B * N, "E": E}, "iters": args.iters,
              "repeats": args.repeats}
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        torch.manual_seed(0)
        x, r = (torch.randn(B, N, E, device=DEV, dtype=dtype,
                            requires_grad=True) for _ in range(2))
        w = (1 + 0.5 * torch.randn(E, device=DEV)).to(dtype).requires_grad_()
        b = torch.randn(E, device=DEV, dtype=dtype, requires_grad=True)
        dy, ds = (torch.randn(B, N, E, device=DEV, dtype=dtype)
                  for _ in range(2))

        def torch_add_ln(x, r, w, b, eps):
            s = x + r
            return s, F.layer_norm(s, (E,), w, b, eps)

        def plain(f):
            def run():
                x.grad = w.grad = b.grad = None
                f(x, w, b, EPS).backward(dy)
            return run

        def fused(f):
            def run():
                x.grad = r.grad = w.grad = b.grad = None
                s, y = f(x, r, w, b, EPS)
                torch.autograd.backward((s, y), (ds, dy))
            return run

        def torch_ln(x, w, b, eps):
            return F.layer_norm(x, (E,), w, b, eps)

        # what is timed must agree before it is compared
        tol = 4e-2 if dtype == torch.bfloat16 else 1e-5
        for got, want in zip(
                (ops.layer_norm(x, w, b, EPS),
                 *ops.add_layer_norm(x, r, w, b, EPS)),
                (torch_ln(x, w, b, EPS), *torch_add_ln(x, r, w, b, EPS))):
            assert (got - want).abs().max() <= tol, (got - want).abs().max()

        result[name] = {
            "layer_norm": compare(
                {"hip": plain(ops.layer_norm), "torch": plain(torch_ln)},
                args.iters, args.repeats),
            "add_layer_norm": compare(
                {"hip": fused(ops.add_layer_norm),
                 "torch": fused(torch_add_ln)},
                args.iters, args.repeats)}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
