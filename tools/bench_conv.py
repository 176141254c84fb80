"""Time the implicit-GEMM convolution kernels against the library at
ResNet-50's batch-32 shapes, forward plus backward (dX and dW) through
autograd, f32 and bf16, channels-last:

  hip    ops.conv2d(x, w, stride)                  (csrc/conv_kernels.hip)
  torch  F.conv2d(x, w, None, stride, k // 2)      on channels-last tensors

Device events around `--iters` calls, every version warmed up first (the
library picks its algorithms there), the two versions alternated inside one
process and the pair repeated `--repeats` times; prints and optionally writes
one JSON with the median and the min..max of the per-call microseconds and the
floating-point operations of a call (2 per multiply-add, three products).

    python tools/bench_conv.py [--json profiles/conv.json]
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402

BATCH = 32
# (H = W of the input, Cin, Cout, k, stride)
SHAPES = [(56, 64, 64, 3, 1), (56, 128, 128, 3, 2), (28, 128, 128, 3, 1),
          (28, 256, 256, 3, 2), (14, 256, 256, 3, 1), (14, 512, 512, 3, 2),
          (7, 512, 512, 3, 1),
          (56, 64, 256, 1, 1), (56, 256, 64, 1, 1), (28, 512, 128, 1, 1),
          (14, 1024, 256, 1, 1), (7, 2048, 512, 1, 1), (56, 256, 512, 1, 2)]
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


def main():
    ap = argparse.ArgumentParser()
    # 400 calls of 90..900 us: a timed window of 40..400 ms
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv needs a GPU"
    result = {"iters": args.iters, "repeats": args.repeats, "batch": BATCH,
              "cases": []}
    for (hw, cin, cout, k, s), (dtype, dname) in ((sh, d) for sh in SHAPES
                                                  for d in (
            (torch.float32, "f32"), (torch.bfloat16, "bf16"))):
        torch.manual_seed(0)
        x = torch.randn(BATCH, cin, hw, hw, device=DEV, dtype=dtype) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(cout, cin, k, k, device=DEV, dtype=dtype)
             * (cin * k * k) ** -0.5).requires_grad_(True)
        wl = w.detach().contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)  # the layout the library prefers
        ho = (hw + 2 * (k // 2) - k) // s + 1
        dy = torch.randn(BATCH, cout, ho, ho, device=DEV, dtype=dtype) \
            .contiguous(memory_format=torch.channels_last)

        def hip():
            x.grad = w.grad = None
            ops.conv2d(x, w, s).backward(dy)

        def stock():
            x.grad = wl.grad = None
            F.conv2d(x, wl, None, s, k // 2).backward(dy)

        case = {"hw": hw, "cin": cin, "cout": cout, "k": k, "stride": s,
                "dtype": dname,
                "flop": 3 * 2 * BATCH * ho * ho * cout * cin * k * k}
        case.update(compare({"hip": hip, "torch": stock}, args.iters,
                            args.repeats))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
