"""Time the fused self-attention against the torch path at the ViT-L/32 shape
(B 32, H 16, N 50, D 64; `--shape B H N D` for another, such as ViT-B/16's
32 12 197 64), forward plus backward, f32 and bf16:

  (a) ops.self_attention on the packed qkv  vs  F.scaled_dot_product_attention
      WITH the reshapes and transposes nn.MultiheadAttention does around it
  (b) HipSelfAttention  vs  nn.MultiheadAttention

Device events around `--iters` calls, every version warmed up first, the two
versions alternated inside one process and the pair repeated `--repeats`
times; prints and optionally writes one JSON with the median and the
min..max of the per-call microseconds.

    python tools/bench_attention.py [--json profiles/attention_r10a.json]

`--matrix bf16` times bf16 storage only and adds the wide bf16 MFMA kernels
(`matrix="bf16"`, key "hip-bf16") as a third version, alternating with the
f32-MFMA path ("hip") and the library ("torch") in the same call.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops  # noqa: E402
from mi355x_ddp.models import HipSelfAttention  # noqa: E402

B, H, N, D = 32, 16, 50, 64
E = H * D
DEV = "cuda:0"


def torch_core(qkv):
    """nn.MultiheadAttention's own data movement around SDPA."""
    q, k, v = (t.reshape(B, N, H, D).transpose(1, 2)
               for t in qkv.chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(q, k, v)
    return o.transpose(1, 2).reshape(B, N, E)


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
    global B, H, N, D, E
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json")
    ap.add_argument("--shape", type=int, nargs=4, default=[B, H, N, D],
                    metavar=("B", "H", "N", "D"))
    ap.add_argument("--matrix", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()
    B, H, N, D = args.shape
    E = H * D
    wide = args.matrix == "bf16"
    assert torch.cuda.is_available(), "bench_attention needs a GPU"
    result = {"shape": {"B": B, "H": H, "N": N, "D": D},
              "iters": args.iters, "repeats": args.repeats,
              "matrix": args.matrix}
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        if wide and dtype != torch.bfloat16:
            continue
        torch.manual_seed(0)
        qkv = torch.randn(B, N, 3 * E, device=DEV, dtype=dtype,
                          requires_grad=True)
        dout = torch.randn(B, N, E, device=DEV, dtype=dtype)

        def core(f):
            def run():
                qkv.grad = None
                f(qkv).backward(dout)
            return run

        # what is timed must agree before it is compared
        a, b = ops.self_attention(qkv, H), torch_core(qkv)
        assert (a - b).abs().max() <= (2e-2 if dtype == torch.bfloat16
                                       else 1e-5), (a - b).abs().max()
        if wide:
            a = ops.self_attention(qkv, H, matrix="bf16")
            assert (a - b).abs().max() <= 2e-2, (a - b).abs().max()
        hip = HipSelfAttention(E, H).to(DEV, dtype)
        mha = nn.MultiheadAttention(E, H, batch_first=True).to(DEV, dtype)
        mha.load_state_dict(hip.state_dict())
        x = torch.randn(B, N, E, device=DEV, dtype=dtype, requires_grad=True)

        def module(f):
            def run():
                x.grad = None
                f(x).backward(dout)
            return run

        cores = {"hip": core(lambda t: ops.self_attention(t, H)),
                 "torch": core(torch_core)}
        modules = {"hip": module(hip),
                   "torch": module(
                       lambda t: mha(t, t, t, need_weights=False)[0])}
        if wide:
            hip_wide = HipSelfAttention(E, H, matrix="bf16").to(DEV, dtype)
            hip_wide.load_state_dict(hip.state_dict())
            cores = {"hip-bf16": core(
                lambda t: ops.self_attention(t, H, matrix="bf16")), **cores}
            modules = {"hip-bf16": module(hip_wide), **modules}
        result[name] = {
            "core": compare(cores, args.iters, args.repeats),
            "module": compare(modules, args.iters, args.repeats)}
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
