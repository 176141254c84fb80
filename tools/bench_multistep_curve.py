"""Per-step cost of the multi-step trainer vs steps-per-launch S:
quantifies how launch/dispatch overhead amortizes (docs/KERNELS.md).

Each launch reads a DIFFERENT window of a buffer far larger than L2
(`--pool-steps` tiles, default 32768 = 84 MB of X at batch 32), so the
large-S rows are not one re-read warm tile (profiles r01q caveat).
`--impl` switches the fp32 kernel (MFMA spec kernel vs the lane-parallel
fmaf-chain kernel) through the extension's process-wide selector;
`--impl both` alternates them per S and per repeat for same-box A/Bs.
`--depth` selects the chain kernel's prefetch ring depth (0 = default).
"""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mi355x_ddp import ops
from mi355x_ddp.models import toy_model
from mi355x_ddp.parallel.reducer import Reducer

ap = argparse.ArgumentParser()
ap.add_argument("--impl", default="both",
                help="mfma | chain | both (alternating)")
ap.add_argument("--depth", default="0",
                help="chain prefetch ring depth(s), comma-separated; 0 = default")
ap.add_argument("--sizes", default="1,2,4,8,16,32,64,256,1024")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--pool-steps", type=int, default=32768)
ap.add_argument("--bf16", action="store_true", help="also time the bf16 kernel")
args = ap.parse_args()

dev = "cuda:0"
ext = ops.ext()
B = args.batch
torch.manual_seed(0)
m = toy_model(20, 1).to(dev)
red = Reducer(list(m.parameters()), comm=None)
b = red.buckets[0]
w_off = b.offsets[red._param_index[m.weight][1]]
b_off = b.offsets[red._param_index[m.bias][1]]
P = args.pool_steps
X = torch.rand(P * B, 20, device=dev)
T = torch.rand(P * B, 1, device=dev)
dummy = torch.Tensor()
has_switch = hasattr(ext, "set_toy_multistep_impl")
impls = ["mfma", "chain"] if args.impl == "both" else [args.impl]
if not has_switch:
    impls = ["mfma"]
depths = [int(d) for d in args.depth.split(",")]
variants = []
for impl in impls:
    if impl == "chain":
        variants += [("chain", d) for d in depths]
    else:
        variants.append((impl, 0))


def select(impl, depth):
    if has_switch:
        ext.set_toy_multistep_impl(impl)
        ext.set_toy_multistep_chain_depth(depth)


def timed(x, t, p, S, reps):
    """ns/step over `reps` launches, each on its own window of the pool."""
    nwin = max(P // S, 1)

    def run(n, base):
        for i in range(n):
            lo = ((base + i) % nwin) * S * B
            ext.toy_multistep(x[lo:lo + S * B], t[lo:lo + S * B], p, dummy,
                              True, w_off, b_off, 1e-4, B)

    run(20, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(reps, 20)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps / S * 1e9


names = [i if i != "chain" or d == 0 else f"chain D={d}" for i, d in variants]
print(f"batch {B}, pool {P} tiles, {args.repeats} repeats per cell (ns/step)")
print("| S (steps/launch) | " + " | ".join(f"fp32 {n}" for n in names)
      + (" | bf16 |" if args.bf16 else " |"))
print("|---|" + "---|" * (len(names) + (1 if args.bf16 else 0)))
if args.bf16:
    Xb, Tb = X.bfloat16(), T.bfloat16()
for S in (int(s) for s in args.sizes.split(",")):
    reps = max(2000 // S, 100)
    cells = [[] for _ in variants]
    for _ in range(args.repeats):  # alternate implementations per repeat
        for j, (impl, d) in enumerate(variants):
            select(impl, d)
            p = b.flat_param.clone()
            cells[j].append(timed(X, T, p, S, reps))
    row = [" / ".join(f"{v:.0f}" for v in c) for c in cells]
    if args.bf16:
        pb = b.flat_param.bfloat16()
        row.append(f"{timed(Xb, Tb, pb, S, reps):.0f}")
    print(f"| {S} | " + " | ".join(row) + " |", flush=True)
