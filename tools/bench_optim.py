"""Per-step cost of the flat-bucket optimizers against torch.optim on the
same GPU, at the sizes a user runs: ResNet-50's real buckets and one 64 MiB
fp32 bucket.

Ours: FusedSGD(momentum=0.9, weight_decay=1e-4) and FusedAdamW attached to
a world-1 DDP reducer — one kernel per bucket (plus one tick for AdamW),
grad zeroing folded in. Baselines: torch.optim.SGD / AdamW with
foreach=True and with fused=True, each timed WITH the
zero_grad(set_to_none=False) it needs on the bucket-view gradients (the
Trainer issues exactly that for a non-flat optimizer).

Method: every configuration is warmed up, then timed ITERS steps between
two device events, REPEATS times, the configurations alternating inside
each repeat so that drift on a shared host hits all of them alike. Reported
per configuration: the median step time, the min-max spread of the repeats,
the device kernels and copies one step launches (counted by the profiler in a step of
its own, after the timing; named for our configurations), and the effective bandwidth — the bytes the update MUST move over
the median time, beside the measured float4-copy rate of the chip
(6.29 TB/s). fp32 momentum SGD reads p, g, buf and writes p, buf, g: 24 B
per element; fp32 AdamW reads p, g, m, v and writes p, m, v, g: 32 B.

The `+clip` configurations add clipping by the global L2 norm at 1.0:
ours with max_grad_norm=1.0 (one k_sumsq_flat per bucket, one k_clip_coef,
the coefficient folded into the update kernels), torch's as
clip_grad_norm_(params, 1.0, foreach=True) ahead of the fused=True step
and its zero_grad. Clipping MUST read g once more for the norm: 28 and
36 B per element.

Prints one JSON line (and writes it to --out when given). Needs a GPU.

Usage: python tools/bench_optim.py [--iters 200] [--repeats 7] [--out F]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mi355x_ddp.parallel import DDP, FusedAdamW, FusedSGD  # noqa: E402

DEV = "cuda:0"
COPY_RATE_TBS = 6.29  # measured float4 copy, MI355X_MICROARCH
BYTES_PER_ELEM = {"sgd": 24, "adamw": 32}
CLIP_EXTRA_BYTES = 4  # one more fp32 read of g, for the norm
MAX_GRAD_NORM = 1.0


class OneBucket(torch.nn.Module):
    def __init__(self, numel):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(numel))


def make_model(workload):
    torch.manual_seed(0)
    if workload == "resnet50":
        from mi355x_ddp.models import resnet50
        return resnet50().to(DEV)
    return OneBucket(64 * 1024 * 1024 // 4).to(DEV)


def fill_grads(params):
    gen = torch.Generator(device=DEV).manual_seed(1)
    for p in params:
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_(torch.randn(p.shape, device=DEV, generator=gen) * 1e-2)


def build(workload, name):
    """-> (step callable, numel stepped, bucket count or None, the objects
    the step needs kept alive)."""
    model = make_model(workload)
    params = [p for p in model.parameters() if p.requires_grad]
    numel = sum(p.numel() for p in params)
    kind, impl = name.split("/")
    clip = impl.endswith("+clip")
    impl = impl[:-len("+clip")] if clip else impl
    if impl == "flat":
        eng = DDP(model, comm=None, bucket_cap_mb=1024.0
                  if workload == "bucket64MiB" else None)
        kw = {"max_grad_norm": MAX_GRAD_NORM} if clip else {}
        opt = (FusedSGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-4,
                        **kw)
               if kind == "sgd" else FusedAdamW(params, **kw))
        opt.attach_reducer(eng.reducer)
        fill_grads(params)
        return opt.step, numel, len(eng.reducer.buckets), (model, eng, opt)
    kw = {"foreach": True} if impl == "foreach" else {"fused": True}
    opt = (torch.optim.SGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-4,
                           **kw)
           if kind == "sgd" else torch.optim.AdamW(params, **kw))
    fill_grads(params)

    def step():
        if clip:
            torch.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM,
                                           foreach=True)
        opt.step()
        opt.zero_grad(set_to_none=False)

    return step, numel, None, (model, opt)


def count_kernels(step):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) \
            as prof:
        step()
        torch.cuda.synchronize()
    # device-side events only: the host ops that launched them carry the
    # same device time a second time, and so does the Optimizer.step#...
    # range that torch mirrors onto the device timeline
    return {ev.key: ev.count for ev in prof.key_averages()
            if ev.device_type == torch.autograd.DeviceType.CUDA
            and not ev.key.startswith("Optimizer.step#")}


def time_once(step, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on a GPU; none found")

    names = ["sgd/flat", "sgd/foreach", "sgd/fused",
             "sgd/flat+clip", "sgd/fused+clip",
             "adamw/flat", "adamw/foreach", "adamw/fused",
             "adamw/flat+clip", "adamw/fused+clip"]
    result = {"tool": "bench_optim", "device": torch.cuda.get_device_name(0),
              "iters": args.iters, "repeats": args.repeats,
              "copy_rate_TBs": COPY_RATE_TBS, "workloads": {}}
    for workload in ("resnet50", "bucket64MiB"):
        cfgs = {n: build(workload, n) for n in names}
        for step, *_ in cfgs.values():
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        samples = {n: [] for n in names}
        for _ in range(args.repeats):
            for n in names:  # alternate: drift hits every config alike
                samples[n].append(time_once(cfgs[n][0], args.iters))
        out = {}
        events = {n: count_kernels(cfgs[n][0]) for n in names}
        for n in names:
            step, numel, buckets, _keep = cfgs[n]
            med = statistics.median(samples[n])
            need = numel * (BYTES_PER_ELEM[n.split("/")[0]]
                            + (CLIP_EXTRA_BYTES if n.endswith("+clip")
                               else 0))
            out[n] = {
                "step_us_median": round(med, 2),
                "step_us_min": round(min(samples[n]), 2),
                "step_us_max": round(max(samples[n]), 2),
                "spread_pct": round(
                    100 * (max(samples[n]) - min(samples[n])) / med, 2),
                "kernels_per_step": sum(events[n].values()),
                "effective_TBs": round(need / med / 1e6, 3),
                "share_of_copy_rate": round(
                    need / med / 1e6 / COPY_RATE_TBS, 3),
            }
            if buckets is not None:
                out[n]["buckets"] = buckets
                out[n]["device_events"] = events[n]  # what was counted
        for kind in ("sgd", "adamw"):
            ours, ref = out[f"{kind}/flat"], out[f"{kind}/fused"]
            out[f"{kind}/flat_vs_torch_fused"] = round(
                ref["step_us_median"] / ours["step_us_median"], 3)
            out[f"{kind}/flat_vs_torch_foreach"] = round(
                out[f"{kind}/foreach"]["step_us_median"]
                / ours["step_us_median"], 3)
            clipped = out[f"{kind}/flat+clip"]
            out[f"{kind}/flat+clip_vs_torch_fused+clip"] = round(
                out[f"{kind}/fused+clip"]["step_us_median"]
                / clipped["step_us_median"], 3)
            out[f"{kind}/flat+clip_vs_flat"] = round(
                clipped["step_us_median"] / ours["step_us_median"], 3)
        out["numel"] = cfgs[names[0]][1]
        result["workloads"][workload] = out
        del cfgs
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
