"""Time the class-index cross-entropy, forward plus backward, three versions
alternating in one call:

  "index"   ops.cross_entropy_index                  (csrc/loss_kernels.hip)
  "onehot"  ops.cross_entropy on the same labels     (one-hot + k_ce_*; it has
            no label smoothing, so it is left out of the smoothed rows)
  "torch"   F.cross_entropy

at (B, C) = (32, 1000), (256, 1000), (4096, 1000), (32, 21843), f32 and bf16,
label_smoothing 0 and 0.1. Device events around `--iters` calls, every version
warmed up first, the versions alternated and the round repeated `--repeats`
times; prints and optionally writes one JSON with the median and the min..max
of the per-call microseconds.

    python tools/bench_cross_entropy.py [--json profiles/cross_entropy.json]

`--shape B C`, `--dtype` and `--only` narrow the run, for a kernel trace of
one configuration.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402

SHAPES = [(32, 1000), (256, 1000), (4096, 1000), (32, 21843)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
DEV = "cuda:0"


def timed(fn, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per call


def compare(versions, iters, repeats):
    for fn in versions.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in versions}
    for _ in range(repeats):
        for k, fn in versions.items():
            samples[k].append(timed(fn, iters))
    return {k: {"median_us": round(statistics.median(v), 2),
                "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "C"))
    ap.add_argument("--dtype", choices=tuple(DTYPES))
    ap.add_argument("--only", choices=("index", "onehot", "torch"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cross_entropy needs a GPU"
    result = {"iters": args.iters, "repeats": args.repeats, "rows": []}
    for B, C in [tuple(args.shape)] if args.shape else SHAPES:
        for name in [args.dtype] if args.dtype else DTYPES:
            torch.manual_seed(0)
            x = (2 * torch.randn(B, C, device=DEV)).to(DTYPES[name])
            x.requires_grad_(True)
            labels = torch.randint(0, C, (B,), device=DEV)
            for smoothing in (0.0, 0.1):
                fns = {
                    "index": lambda: ops.cross_entropy_index(
                        x, labels, smoothing),
                    "onehot": lambda: ops.cross_entropy(x, labels),
                    "torch": lambda: F.cross_entropy(
                        x, labels, label_smoothing=smoothing)}
                if smoothing:
                    del fns["onehot"]
                if args.only:
                    fns = {k: f for k, f in fns.items() if k == args.only}

                def step(f):
                    def run():
                        x.grad = None
                        f().backward()
                    return run

                # what is timed must agree before it is compared
                tol = 2e-2 if name == "bf16" else 1e-5
                want = F.cross_entropy(x.float(), labels,
                                       label_smoothing=smoothing)
                for f in fns.values():
                    assert abs(float(f()) - float(want)) <= tol * float(want)
                result["rows"].append({
                    "B": B, "C": C, "dtype": name, "label_smoothing": smoothing,
                    **compare({k: step(f) for k, f in fns.items()},
                              args.iters, args.repeats)})
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
