#!/usr/bin/env python3
"""What an observation and action history costs (PPOTrainer(history=); include/ppenv_history.h).  Two measurements, one JSON line each:

  kernel   pp_history_push at --rows rows for the 7-dof (80, 7) and the 27-dof (313, 27) widths with history (2, 2), between two rows of a
           horizon buffer as the collector lays them out, next to a torch copy_ of one wide row slab into the other: the same number of
           bytes written on the same tensors, the yardstick of a pure copy.  Each is launched --launches times back to back inside one
           timed window (device events), after a warm-up; --repeats windows, the median and the minimum reported.
  train    us per collected horizon and per minibatch step of one task at --num-envs envs with --history Ho,Ha and without (the trainer
           without the argument launches nothing for it: the parent's path), alternating the two trainers window by window; host clock
           around a synchronise, as tools/gpu_critic_input_time.py."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def kernel(args):
    import torch
    from isaacgym_amd import history
    dev = torch.device("cuda:0")
    for rows in args.rows:
        for n, a in ((80, 7), (313, 27)):
            stack = history.HistoryStack(rows, n, a, 2, 2, dev)
            W = stack.width
            wide = torch.randn((2, rows, W), device=dev)
            obs, act = torch.randn((rows, n), device=dev), torch.randn((rows, a), device=dev)
            done = (torch.rand(rows, device=dev) < 0.03).to(torch.int64)
            push = lambda: stack.push(obs, act, done, wide[0], wide[1])
            copy = lambda: wide[1].copy_(wide[0])

            def window(fn):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.launches):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e3 / args.launches
            for fn in (push, copy):
                window(fn)
            us = {"push": [], "copy": []}
            for _ in range(args.repeats):                  # alternating: both see the same neighbours on the machine
                us["push"].append(window(push))
                us["copy"].append(window(copy))
            moved = 4 * rows * (2 * W)                      # a row read and a row written, either way (a start reads less)
            out = dict(measure="kernel", rows=rows, num_obs=n, num_actions=a, history=[2, 2], width=W, bytes_moved=moved, launches_per_window=args.launches)
            for k, v in us.items():
                out[f"us_{k}"], out[f"us_{k}_min"] = round(statistics.median(v), 2), round(min(v), 2)
                out[f"gbps_{k}"] = round(moved / statistics.median(v) / 1e3, 1)
            print(json.dumps(out), flush=True)


def train(args):
    import torch
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    trainers = {}
    for label, hist in (("plain", None), ("history", args.history)):
        task = isaacgym_amd.make(seed=0, task=args.task, num_envs=args.num_envs)
        trainers[label] = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, action_delay=(0, 3), history=hist)

    def horizon(tr):
        tr.collect()
        tr.meter.update(tr.col.rewards, tr.col.dones)
        tr.col.next_horizon()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6
    for tr in trainers.values():                            # a run that has been going for a while, and every shape warmed
        for _ in range(3):
            horizon(tr)
            for t in range(tr.cfg.horizon_length):
                tr.learner.rms.update(tr.col.obs[t])
        horizon(tr)
    hz = {k: [] for k in trainers}
    for _ in range(args.horizons):
        for k, tr in trainers.items():
            hz[k].append(timed(lambda: horizon(tr)))
    mb = {k: [] for k in trainers}
    for tr in trainers.values():
        tr.collect()
        tr.prepare()
        tr.minibatch_step(0, tr.stats[0])
    for _ in range(args.steps):
        for k, tr in trainers.items():
            mb[k].append(timed(lambda: tr.minibatch_step(0, tr.stats[0])))
    for k, tr in trainers.items():
        H = tr.cfg.horizon_length
        print(json.dumps(dict(measure="train", run=k, task=args.task, history=tr.history(), num_envs=args.num_envs, horizon=H, minibatch=args.minibatch,
                              first_layer_k=int(tr.learner.net.w[0].shape[-1]), us_per_horizon=round(statistics.median(hz[k]), 1),
                              us_horizon_min=round(min(hz[k]), 1), us_per_rollout_step=round(statistics.median(hz[k]) / H, 1),
                              us_per_minibatch_step=round(statistics.median(mb[k]), 1), us_minibatch_min=round(min(mb[k]), 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "train"))
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--history", default="2,2")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=8192)
    ap.add_argument("--horizons", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    kernel(args) if args.what == "kernel" else train(args)


if __name__ == "__main__":
    main()
