#!/usr/bin/env python3
"""What training under domain randomisation costs the rollout (PPOTrainer(randomization=, adr=); include/ppenv_dr.h,
include/ppenv_dr_adr.h): us per collected horizon of one task at --num-envs envs.

A horizon here is what train_epoch() runs before the learning: collect() (32 env steps + policy forwards + the per-step randomisation
launch, the bootstrap forward, GAE), ADR's fold and update, the score meter.  After three horizons of statistics and a warm-up horizon,
--horizons horizons are timed one by one (host clock around a synchronise) and the median is reported, every horizon kept.
--mode none | tables | randomization | adr.  `tables` hands the env tables of ones and launches nothing for them: the randomised step
kernels' own share, apart from the per-step launch the other two modes add.  `randomization` is a plan of uniform scalings
of the link masses and the friction; `adr` the same two tables as dims, a quarter of the envs on a boundary.  --root DIR imports the
package from another checkout — the parent commit's, labelled with --build, mode none only — so that a caller can alternate processes of
the two builds.  One JSON line."""
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
    ap.add_argument("--mode", choices=("none", "tables", "randomization", "adr"), default="none")
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
    task = isaacgym_amd.make(seed=0, task=args.task, num_envs=args.num_envs)
    mass_rows = task.env.DR_TABLE_ROWS["link_mass_scale"]
    kw = {}
    if args.mode == "randomization":
        uniform = lambda rows, lo, hi: dict(rows=rows, distribution="uniform", operation="scaling", range=(lo, hi), schedule=None, schedule_steps=0)
        kw = dict(randomization={"frequency": 1, "tables": {"link_mass_scale": uniform(mass_rows, 0.8, 1.2), "friction_scale": uniform(1, 0.7, 1.3)}})
    elif args.mode == "adr":
        kw = dict(adr=dict(dims={"link_mass_scale": dict(start=(0.8, 1.2), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(0.7, 1.3), limit=(0.4, 1.6), step=0.1)},
                           boundary_frac=0.25, min_games=256, t_low=-1e30, t_high=1e30))
    tr = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, **kw)
    if args.mode == "tables":
        n, dev = task.env.num_envs, task.env.device
        task.env.set_randomization(link_mass_scale=torch.ones((mass_rows, n), device=dev), friction_scale=torch.ones(n, device=dev))
    H = tr.cfg.horizon_length

    def horizon():
        tr.collect()
        if getattr(tr, "adr", None) is not None:
            tr.adr.epoch() if hasattr(tr.adr, "epoch") else tr._adr_epoch()      # (--root: a checkout from before HorizonStage.epoch)
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
    if args.mode == "adr":
        out["games"] = int(tr.adr.games.sum())
    if args.mode == "randomization":
        out["redraws"] = int(tr.env.reset_randomization.draws.sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
