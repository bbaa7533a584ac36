#!/usr/bin/env python3
"""What privileged critic inputs cost (PPOTrainer(critic_inputs=); include/ppenv_critic_input.h): us per collected horizon and us per
minibatch step of one task at --num-envs envs, under ADR of the link masses and the friction and --action-delay 0:3.

A horizon is what tools/gpu_adr_train_time.py times: collect() (32 env steps + policy forwards + the per-step launches, the bootstrap
forward, GAE), ADR's fold and update, the score meter.  A minibatch step is PPOTrainer.minibatch_step on --minibatch rows of the prepared
horizon: forward (statistics update), loss gradient, backward, the two optimizer launches, the recast.  After three horizons of
statistics and a warm-up, --horizons horizons and --steps minibatch steps are timed one by one (host clock around a synchronise); the
medians are reported, every sample kept.  --critic-inputs NAMES (empty: none).  --root DIR imports the package from another checkout —
the parent commit's, labelled with --build, without --critic-inputs — so that a caller can alternate processes of the two builds.
One JSON line."""
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
    ap.add_argument("--critic-inputs", default="")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=8192)
    ap.add_argument("--horizons", type=int, default=30)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--build", default="this build", help="the label of --root in the output")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    task = isaacgym_amd.make(seed=0, task=args.task, num_envs=args.num_envs)
    kw = dict(adr=dict(dims={"link_mass_scale": dict(start=(0.8, 1.2), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(0.7, 1.3), limit=(0.4, 1.6), step=0.1)},
                       boundary_frac=0.25, min_games=256, t_low=-1e30, t_high=1e30), action_delay=(0, 3))
    if args.critic_inputs:
        kw["critic_inputs"] = args.critic_inputs
    tr = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, **kw)
    H = tr.cfg.horizon_length

    def horizon():
        tr.collect()
        tr.adr.epoch() if hasattr(tr.adr, "epoch") else tr._adr_epoch()          # (--root: a checkout from before HorizonStage.epoch)
        tr.meter.update(tr.col.rewards, tr.col.dones)
        tr.col.next_horizon()

    def timed(fn, n):
        us = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        return us
    for _ in range(3):                      # a run that has been going for a while (tools/ppo_epoch_bench.py)
        horizon()
        for t in range(H):
            tr.learner.rms.update(tr.col.obs[t])
    horizon()
    hz = timed(horizon, args.horizons)
    tr.collect()
    tr.prepare()
    step = lambda: tr.minibatch_step(0, tr.stats[0])
    step()
    mb = timed(step, args.steps)
    rec = tr.critic_inputs() if hasattr(tr, "critic_inputs") else None
    print(json.dumps(dict(task=args.task, build=args.build, critic_inputs=rec, num_envs=args.num_envs, horizon=H, minibatch=args.minibatch,
                          first_layer_k=int(tr.learner.net.w[0].shape[-1]), us_per_horizon=round(statistics.median(hz), 1), us_horizon_min=round(min(hz), 1),
                          us_per_minibatch_step=round(statistics.median(mb), 1), us_minibatch_min=round(min(mb), 1),
                          us_horizons=[round(t, 1) for t in hz], us_minibatch_steps=[round(t, 1) for t in mb])), flush=True)


if __name__ == "__main__":
    main()
