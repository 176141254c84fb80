"""Time the tiled-GEMM MLP against the torch path at the ViT-L/32 shape
(R = 32 * 50 = 1600 rows, 1024 -> 4096 -> 1024), forward plus backward with
all gradients, f32 and bf16: ops.mlp vs nn.Sequential(Linear, GELU, Linear).

Device events around `--iters` calls, both versions warmed up first, the two
alternated inside one process and the pair repeated `--repeats` times; prints
and optionally writes one JSON with the median and the min..max of the
per-call microseconds. `--iters 5 --repeats 1` under a kernel tracer gives
the per-launch times of the six GEMMs beside the library's kernels.

    python tools/bench_mlp.py [--json profiles/mlp_r13a.json]
"""
import argparse
import json
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402

R, HIDDEN, MLP = 32 * 50, 1024, 4096
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlp needs a GPU"
    flops = 3 * 2 * 2 * R * HIDDEN * MLP  # fwd + dX + dW of both linears
    result = {"shape": {"R": R, "hidden": HIDDEN, "mlp": MLP},
              "iters": args.iters, "repeats": args.repeats, "flop": flops}
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        torch.manual_seed(0)
        seq = nn.Sequential(nn.Linear(HIDDEN, MLP), nn.GELU(),
                            nn.Linear(MLP, HIDDEN)).to(DEV, dtype)
        p = [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias]
        x = torch.randn(R, HIDDEN, device=DEV, dtype=dtype,
                        requires_grad=True)
        dy = torch.randn(R, HIDDEN, device=DEV, dtype=dtype)

        def run(f):
            def go():
                x.grad = None
                for t in p:
                    t.grad = None
                f().backward(dy)
            return go

        hip, ref = (lambda: ops.mlp(x, *p)), (lambda: seq(x))
        # what is timed must agree before it is compared
        tol = 8e-2 if dtype == torch.bfloat16 else 1e-3
        err = (hip() - ref()).abs().max()
        assert err <= tol, err
        r = compare({"hip": run(hip), "torch": run(ref)}, args.iters,
                    args.repeats)
        for v in r.values():
            v["tflops"] = round(flops / v["median_us"] / 1e6, 1)
        result[name] = r
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
