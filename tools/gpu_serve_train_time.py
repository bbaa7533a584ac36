#!/usr/bin/env python3
"""What training on a serve plan or a serve curriculum costs the rollout (PPOTrainer(serve_plan=, curriculum=); include/ppenv_serve.h,
include/ppenv_serve_curric.h): us per collected horizon of one task at --num-envs envs.

A horizon here is what train_epoch() runs before the learning: collect() (32 env steps + policy forwards + the per-step serve launch, the
bootstrap forward, GAE), the curriculum's fold and update, the score meter.  After three horizons of statistics and a warm-up horizon,
--horizons horizons are timed one by one (host clock around a synchronise) and the median is reported, every horizon kept.
--mode none | plan | curriculum (a 64-bin grid, 8 speeds x 8 tilts).  --root DIR imports the package from another checkout — the parent
commit's, labelled with --build, mode none only — so that a caller can alternate processes of the two builds.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--mode", choices=("none", "plan", "curriculum"), default="none")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=32768)
    ap.add_argument("--horizons", type=int, default=30)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--build", default="this build", help="the label of --root in the output")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    ta = "27DOF" in args.task
    speed = (4.0, 6.0) if ta else (6.0, 9.0)
    kw = {}
    if args.mode == "plan":
        kw = dict(serve_plan=[{"serve_speed": speed, "serve_tilt": (-5.0, 5.0)}])
    elif args.mode == "curriculum":
        from isaacgym_amd import curriculum
        kw = dict(curriculum=dict(bins=curriculum.grid({"serve_speed": speed + (8,), "serve_tilt": (-5.0, 5.0, 8)}), power=1, mix=0.25, alpha=0.3))
    task = isaacgym_amd.make(seed=0, task=args.task, num_envs=args.num_envs)
    tr = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, **kw)
    H = tr.cfg.horizon_length

    def horizon():
        tr.collect()
        if getattr(tr, "curriculum", None) is not None:
            tr.curriculum.epoch() if hasattr(tr.curriculum, "epoch") else tr._curriculum_epoch()      # (--root: a checkout from before HorizonStage.epoch)
        tr.meter.update(tr.col.rewards, tr.col.dones)
        tr.col.next_horizon()
    for _ in range(3):                      # a run that has been going for a while (tools/ppo_epoch_bench.py)
        horizon()
        for t in range(H):
            tr.learner.rms.update(tr.col.obs[t])
    horizon()
    us = []
    for _ in range(args.horizons):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        horizon()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    out = dict(task=args.task, build=args.build, mode=args.mode, num_envs=args.num_envs, horizon=H, horizons=args.horizons,
               us_per_horizon=round(statistics.median(us), 1), us_min=round(min(us), 1), us_max=round(max(us), 1), us_all=[round(t, 1) for t in us])
    if args.mode == "curriculum":
        out["games"] = int(tr.curriculum.games.sum())
    if args.mode == "plan":
        out["serves"] = int(tr.task._serve_plan.count.sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
