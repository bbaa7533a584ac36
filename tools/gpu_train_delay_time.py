#!/usr/bin/env python3
"""What training under control latency costs (include/ppenv_train_delay.h; PPOTrainer(action_delay=, obs_delay=)), two measurements:

    push     train_delay_push_kernel (latency.DelayLine, delays drawn in 0..3) against play_delay_push_kernel (play.Delay, a table of the same
             range, depth 4) at the same shapes in ONE process, the two alternating: --rounds times --pushes pushes each after a warm-up, a
             done word on 3 % of the env-steps; us per push (host clock around a synchronise), every round kept.  Shapes: 4096 x 27 (the
             27-dof task's actions) and 4096 x 313 (its observations).
    epoch    one PPOTrainer epoch of the 27-dof task at --num-envs envs, tools/ppo_epoch_bench.py's way (three horizons of statistics, one
             warm-up epoch, then --epochs epochs timed: the rollout with the score meter, and the learning), with --action-delay / --obs-delay
             K | LO:HI.  --root DIR imports the package from another checkout — the parent commit's, labelled with --build, without the
             latency arguments — so that a caller can alternate processes of the two builds.

Each prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sync_timed(torch, fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def push_mode(args, torch):
    import numpy as np
    from isaacgym_amd.latency import DelayLine
    from isaacgym_amd.play import Delay
    dev, rows, out = "cuda:0", args.rows, []
    rng = np.random.default_rng(0)
    dones = [torch.from_numpy((rng.random(rows) < 0.03).astype(np.int64)).to(dev) for _ in range(16)]
    for width in (int(w) for w in args.widths.split(",")):
        x = torch.randn((rows, width), device=dev)
        play = Delay(rows, width, rng.integers(0, 4, rows).astype(np.int32), dev)
        train = DelayLine(rows, width, 0, 3, dev, seed=1)
        dst = torch.zeros((rows, width), device=dev)
        loops = {"play_delay_push": lambda i: play.push(x, dones[i % 16]), "train_delay_push": lambda i: train.push(x, dones[i % 16], dst)}
        for fn in loops.values():
            sync_timed(torch, fn, args.warmup)
        us = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k, fn in loops.items():
                us[k].append(sync_timed(torch, fn, args.pushes))
        row = dict(rows=rows, width=width, depth=4, pushes=args.pushes, rounds=args.rounds)
        for k, v in us.items():
            row[f"{k}_us"] = round(statistics.median(v), 3)
            row[f"{k}_us_all"] = [round(t, 3) for t in v]
        out.append(row)
    return dict(mode="push", shapes=out)


def epoch_mode(args, torch):
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    kw = {}
    if args.action_delay != "0" or args.obs_delay != "0":
        from isaacgym_amd.latency import delay_range
        kw = dict(action_delay=delay_range("--action-delay", args.action_delay), obs_delay=delay_range("--obs-delay", args.obs_delay))
    task = isaacgym_amd.make(seed=0, task="HumanoidPingpongTiltNESSparse27DOFG1", num_envs=args.num_envs)
    tr = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, **kw)
    H = tr.cfg.horizon_length
    for _ in range(3):                      # a run that has been training for a while (tools/ppo_epoch_bench.py)
        tr.col.collect().next_horizon()
        for t in range(H):
            tr.learner.rms.update(tr.col.obs[t])

    def rollout(_):
        tr.collect()
        tr.meter.update(tr.col.rewards, tr.col.dones)

    def learn(_):
        tr.prepare()
        tr.learn()
    rollout(0); learn(0); tr.col.next_horizon()
    roll, lrn = [], []
    for _ in range(args.epochs):
        roll.append(sync_timed(torch, rollout, 1) / 1e3)
        lrn.append(sync_timed(torch, learn, 1) / 1e3)
        tr.col.sigma.copy_(torch.exp(tr.logstd))
        tr.col.next_horizon()
    return dict(mode="epoch", build=args.build, num_envs=args.num_envs, horizon=H, minibatch=args.minibatch, epochs=args.epochs, action_delay=args.action_delay,
                obs_delay=args.obs_delay, ms_rollout=round(statistics.median(roll), 3), ms_learning=round(statistics.median(lrn), 3),
                ms_rollout_all=[round(t, 3) for t in roll], ms_learning_all=[round(t, 3) for t in lrn],
                finite=bool(all(torch.isfinite(p).all() for p in tr.learner.parameters())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("push", "epoch"))
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--widths", default="27,313", help="push: one width under `rocprofv3 --kernel-trace --stats` gives the two kernels' device time at that shape")
    ap.add_argument("--pushes", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=32768)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--action-delay", default="0")
    ap.add_argument("--obs-delay", default="0")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--build", default="this build", help="the label of --root in the output")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    print(json.dumps((push_mode if args.mode == "push" else epoch_mode)(args, torch)), flush=True)


if __name__ == "__main__":
    main()
