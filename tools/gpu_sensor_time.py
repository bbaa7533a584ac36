#!/usr/bin/env python3
"""What a sensor line costs (sensor.SensorLine; include/ppenv_sensor.h).  Two measurements, one JSON line each:

  kernel   pp_sensor_push at the delay line's yardstick shapes (4096 x 313, 4096 x 27, 16 384 x 80), with every column noised and —
           at width 80 — with only the six ball columns noised and held, drop 0.1, next to the delay line's push (latency.DelayLine, delay
           0..3) on the same shape IN THE SAME PROCESS.  Each is launched --launches times back to back inside one timed window (device
           events), after a warm-up; --repeats windows alternating between the two, the median and the minimum reported.  The method of
           tools/gpu_history_time.py.
  train    us per collected horizon and per rollout step of one task at --num-envs envs with one sensing sensor line on the ball columns and
           without (the trainer without the arguments launches nothing for it: the parent's path), alternating the two trainers window by
           window; host clock around a synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = ((4096, 313), (4096, 27), (16384, 80))


def kernel(args):
    import numpy as np
    import torch
    from isaacgym_amd import latency, sensor
    dev = torch.device("cuda:0")
    for rows, W in SHAPES:
        cases = [("all", None, None)]
        if W == 80:
            ball = sensor.columns("TT", "ball_pos,ball_vel", W)
            cases.append(("ball", ball, ball))
        x, out = torch.randn((rows, W), device=dev), torch.empty((rows, W), device=dev)
        done = (torch.rand(rows, device=dev) < 0.03).to(torch.int64)
        delay = latency.DelayLine(rows, W, 0, 3, dev, seed=1)
        for label, scale, hold in cases:
            line = sensor.SensorLine(rows, W, dev, sigma=np.full(rows, 0.01, np.float32), drop=np.full(rows, 0.1, np.float32), columns=scale, hold_columns=hold, seed=1)
            fns = {"sensor": lambda: line.push(x, done, out), "delay": lambda: delay.push(x, done, out)}

            def window(fn):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.launches):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                return t0.elapsed_time(t1) * 1e3 / args.launches
            for fn in fns.values():
                window(fn)
            us = {k: [] for k in fns}
            for _ in range(args.repeats):                  # alternating: both see the same neighbours on the machine
                for k, fn in fns.items():
                    us[k].append(window(fn))
            held = W if hold is None else int(hold.sum())
            moved = dict(sensor=4 * rows * (2 * W + held), delay=4 * rows * 3 * W)      # in, out and the held columns; in, the ring slot written, the one read, out
            res = dict(measure="kernel", rows=rows, width=W, noised=label, noised_columns=W if scale is None else int((scale != 0).sum()), held_columns=held,
                       launches_per_window=args.launches)
            for k, v in us.items():
                res[f"us_{k}"], res[f"us_{k}_min"] = round(statistics.median(v), 2), round(min(v), 2)
                res[f"gbps_{k}"] = round(moved[k] / statistics.median(v) / 1e3, 1)
            print(json.dumps(res), flush=True)


def train(args):
    import torch
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    trainers = {}
    for label, kw in (("plain", {}), ("sensor", dict(obs_noise=(0.0, 0.02), obs_drop=0.1, sensor_columns=dict(obs_noise_columns="ball_pos,ball_vel",
                                                                                                           obs_drop_columns="ball_pos,ball_vel")))):
        task = isaacgym_amd.make(seed=0, task=args.task, num_envs=args.num_envs)
        trainers[label] = PPOTrainer(task, PPOConfig(minibatch_size=args.minibatch), seed=0, **kw)

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
    for tr in trainers.values():
        for _ in range(4):
            horizon(tr)
    hz = {k: [] for k in trainers}
    for _ in range(args.horizons):
        for k, tr in trainers.items():
            hz[k].append(timed(lambda: horizon(tr)))
    for k, tr in trainers.items():
        H = tr.cfg.horizon_length
        print(json.dumps(dict(measure="train", run=k, task=args.task, sensor=tr.sensor(), num_envs=args.num_envs, horizon=H,
                              us_per_horizon=round(statistics.median(hz[k]), 1), us_horizon_min=round(min(hz[k]), 1),
                              us_per_rollout_step=round(statistics.median(hz[k]) / H, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "train"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=8192)
    ap.add_argument("--horizons", type=int, default=20)
    args = ap.parse_args()
    kernel(args) if args.what == "kernel" else train(args)


if __name__ == "__main__":
    main()
