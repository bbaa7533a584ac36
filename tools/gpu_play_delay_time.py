#!/usr/bin/env python3
"""What control latency costs a played checkpoint (include/ppenv_play_delay.h; Player(action_delay=, obs_delay=)), three measurements:

    lines     the control step of a Player with both delay lines (action_delay 2, obs_delay 1) against the same Player without, in one
              process, the two alternating, --rounds times --steps steps each after a warm-up: us per control step, every round kept
    plain     one plain Player (no line is built): us per control step, every round kept.  --root DIR imports the package from another
              checkout — the parent commit's, labelled with --build — so that a caller can alternate processes of the two builds
    trace     a short played run with ONE line (--axis action_delay | obs_delay), meant to run under
              `rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/gpu_play_delay_time.py trace ...`:
              play_delay_push_kernel's row of NAME_kernel_stats.csv is the launch's device time at that width
    stats     reads such a NAME_kernel_stats.csv and prints play_delay_push_kernel's row as JSON with the bytes the rule moves

Each prints one JSON line.  The policy is a randomly initialised network of the trained shape (tools/play_bench.py's); games_num is 2^40,
so nothing freezes and every step pays the full accounting."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def player(args, **kw):
    import torch
    import isaacgym_amd
    from isaacgym_amd.play import Player
    from isaacgym_amd.policy import UNITS, RLGamesPolicy
    from test_policy_mlp import _rlgames_state_dict
    task = isaacgym_amd.make(seed=1, task=args.task, num_envs=args.num_envs)
    sd = _rlgames_state_dict(torch, task.num_obs, tuple(UNITS), task.num_actions, torch.Generator().manual_seed(0))
    pl = Player(task, RLGamesPolicy(sd, task.device), games_num=1 << 40, **kw)
    pl.start()
    return pl


def timed(torch, fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("lines", "plain", "trace", "stats"))
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--build", default="this build", help="the label of --root in the output")
    ap.add_argument("--axis", default="action_delay")
    ap.add_argument("--csv", default=None)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    args = ap.parse_args()
    if args.mode == "stats":
        with open(args.csv) as fh:
            row = [r for r in csv.DictReader(fh) if "play_delay_push_kernel" in r["Name"]][0]
        moved = 3 * args.rows * args.width * 4
        avg = float(row["AverageNs"])
        print(json.dumps(dict(kernel="play_delay_push_kernel", rows=args.rows, width=args.width, calls=int(row["Calls"]), average_ns=avg, min_ns=int(row["MinNs"]),
                              max_ns=int(row["MaxNs"]), bytes_moved=moved, ns_at_6_3_TB_per_s=round(moved / 6.3e3, 1), GB_per_s=round(moved / avg, 1))))
        return
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "tests"))
    import torch
    out = dict(mode=args.mode, task=args.task, num_envs=args.num_envs, steps=args.steps, rounds=args.rounds, build=args.build)
    if args.mode == "trace":
        pl = player(args, **{args.axis: 2})
        timed(torch, pl.step, args.steps)
        line = pl._act_line if args.axis == "action_delay" else pl._obs_line
        out.update(axis=args.axis, rows=line.rows, width=line.width, depth=line.depth)
    else:
        loops = {"plain": player(args)}
        if args.mode == "lines":
            loops["lines"] = player(args, action_delay=2, obs_delay=1)
        for pl in loops.values():
            timed(torch, pl.step, args.warmup)
        us = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k, pl in loops.items():
                us[k].append(timed(torch, pl.step, args.steps))
        for k, v in us.items():
            out[f"{k}_us"] = round(statistics.median(v), 2)
            out[f"{k}_us_all"] = [round(x, 2) for x in v]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
