"""Time per control step of the play loop (isaacgym_amd.play.Player: policy -> task.step -> accumulate) against the same loop without the
accounting (the eager, non-graph step of tools/rollout_bench.py through the VecTask surface) and with a host read of the totals every
--poll-every steps.  The three loops alternate, --repeats times each; the medians are printed as one JSON line.

    python tools/play_bench.py --task HumanoidPingpongTiltG1 --num-envs 4096
    rocprofv3 --kernel-trace --stats -d out -o play -- python tools/play_bench.py --num-envs 4096 --repeats 1      # the launches' own time
    python tools/play_bench.py --num-envs 4096 --sweep-groups 16      # the same loops under Player(sweep=): 16 groups, the grouped accounting
    python tools/play_bench.py --num-envs 4096 --serve-plan 16        # ... under a paired sweep of 16 equal cells: a serve plan, one more launch per task.step
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--poll-every", type=int, default=64)
    ap.add_argument("--sweep-groups", type=int, default=0, help="G > 0: play under a sweep of G cells (friction_scale 0.5 .. 1.5), G groups of num_envs / G envs")
    ap.add_argument("--serve-plan", type=int, default=0, help="G > 0: play under a paired sweep of G equal cells (Sweep([{}] * G, paired=True)): every task.step "
                    "of the three loops also launches the serve plan's apply")
    args = ap.parse_args()
    if args.serve_plan > 0 and args.sweep_groups > 0:
        ap.error("--serve-plan and --sweep-groups are two runs")
    import torch
    import isaacgym_amd
    from isaacgym_amd.play import Player
    from isaacgym_amd.policy import UNITS, RLGamesPolicy
    from test_policy_mlp import _rlgames_state_dict
    task = isaacgym_amd.make(seed=1, task=args.task, num_envs=args.num_envs)
    sd = _rlgames_state_dict(torch, task.num_obs, tuple(UNITS), task.num_actions, torch.Generator().manual_seed(0))
    policy = RLGamesPolicy(sd, task.device)
    sweep = {}
    if args.sweep_groups > 0:
        from isaacgym_amd.play import Sweep
        sweep["sweep"] = Sweep.parse([f"friction_scale=0.5:1.5:{args.sweep_groups}"])
    if args.serve_plan > 0:
        from isaacgym_amd.play import Sweep
        sweep["sweep"] = Sweep([{} for _ in range(args.serve_plan)], paired=True)
    groups = max(args.sweep_groups, args.serve_plan)
    pl = Player(task, policy, games_num=1 << 40, poll_every=args.poll_every, **sweep)       # never frozen: every step pays the full accounting
    pl.start()

    def bare():
        actions, _ = policy.act(pl._obs, deterministic=True)
        pl._obs = task.step(actions)[0]["obs"]

    def polled():
        pl.step()
        if pl.steps_played % args.poll_every == 0:
            pl.stats.read()

    loops = {"step": bare, "step_accumulate": pl.step, "step_accumulate_poll": polled}

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e6

    for fn in loops.values():
        timed(fn, args.warmup)
    us = {k: [] for k in loops}
    for _ in range(args.repeats):
        for k, fn in loops.items():
            us[k].append(timed(fn, args.steps))
    tot = pl.stats.read()
    if groups > 0:
        from isaacgym_amd.play import sum_totals
        tot = sum_totals(tot)
        tot["launches"] //= groups
    out = {"task": args.task, "num_envs": args.num_envs, "sweep_groups": args.sweep_groups, "serve_plan": args.serve_plan, "rows": pl.stats.rows, "steps": args.steps, "repeats": args.repeats,
           "poll_every": args.poll_every, "games": tot["games"], "launches": tot["launches"]}
    for k, v in us.items():
        out[f"{k}_us"] = round(statistics.median(v), 2)
        out[f"{k}_us_all"] = [round(x, 2) for x in v]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
