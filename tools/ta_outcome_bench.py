#!/usr/bin/env python3
"""What the 27-dof task's outcome counts cost (include/ppenv_ta_outcome.h; a TOOL, not the bench.py metric).

    python tools/ta_outcome_bench.py [--num-envs 4096] [--steps 2000] [--warmup 200] [--episode-length 160] [--outcomes]
        steps a TAEnv (the chain-wave kernel) on random actions and prints one JSON line: ms per step by the host clock around a
        synchronised window, and the windows the struct counted.  Every env starts at progress 0 and resets on the time-out alone, so
        control step k (1-based) is a window — the launch that sums and clears — iff k % (episode_length - 1) == 0.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ta_outcome_bench.py ... ; then, without a GPU:
    python tools/ta_outcome_bench.py --summarise-trace DIR/**/*_kernel_trace.csv --episode-length L --warmup W
        the launches of ta_chain_kernel in start order, split by that rule: count, mean, median, min, max in microseconds of the
        launches that clear and of those that do not (the first W are left out)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--num-envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--episode-length", type=int, default=160)
ap.add_argument("--outcomes", action="store_true")
ap.add_argument("--summarise-trace", metavar="CSV", default=None)
args = ap.parse_args()
period = args.episode_length - 1


def summary(us):
    return dict(count=len(us), mean_us=statistics.fmean(us), median_us=statistics.median(us), min_us=min(us), max_us=max(us)) if us else dict(count=0)


if args.summarise_trace:
    rows = [r for r in csv.DictReader(open(args.summarise_trace)) if "ta_chain_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    clears, plain = [], []
    for k, r in enumerate(rows, start=1):
        if k <= args.warmup:
            continue
        (clears if k % period == 0 else plain).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    print(json.dumps(dict(trace=args.summarise_trace, launches=len(rows), episode_length=args.episode_length, warmup=args.warmup,
                          kernel=sorted({r["Kernel_Name"] for r in rows}), launches_that_clear=summary(clears), other_launches=summary(plain))))
    sys.exit(0)

import torch  # noqa: E402

from isaacgym_amd.tensor_api import TAEnv  # noqa: E402

dev = torch.device("cuda", 0)
env = TAEnv(args.num_envs, device=dev, seed=0, env=dict(episodeLength=args.episode_length))
assert env.sim.kernel == "chain"
out = env.enable_outcomes() if args.outcomes else None
gen = torch.Generator(device=dev).manual_seed(0)
acts = torch.rand(64, args.num_envs, 27, device=dev, generator=gen) * 2 - 1
for k in range(args.warmup):
    env.step(acts[k % 64])
torch.cuda.synchronize()
t0 = time.perf_counter()
for k in range(args.steps):
    env.step(acts[k % 64])
torch.cuda.synchronize()
dt = time.perf_counter() - t0
total = args.warmup + args.steps
res = dict(what="TAEnv.step on random actions, host clock around a synchronised window (launch-bound: see the kernel trace for the kernel's own time)",
           kernel=env.sim.kernel_name, num_envs=args.num_envs, steps=args.steps, warmup=args.warmup, episode_length=args.episode_length,
           outcomes=bool(args.outcomes), ms_per_step=dt / args.steps * 1e3, expected_windows=total // period)
if out is not None:
    f = {k: int(v) for k, v in env.outcome_fields().items()}
    assert f["windows"] == total // period and f["envs"] == f["windows"] * args.num_envs, f
    res["struct"] = f
print(json.dumps(res))
