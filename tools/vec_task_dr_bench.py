#!/usr/bin/env python3
"""`VecTask.step` per call with domain randomisation off, in the per-step host mode and in the reset-time device mode:
tools/vec_task_bench.py's loop — eager launches from Python, what rl_games' env wrapper pays — on the reference yaml's
randomization_params block (frequency 600).  python tools/vec_task_dr_bench.py --mode off|step|reset [--root <another checkout>]
prints one JSON line per task; --root times another checkout's package (the parent commit's, for a same-call comparison)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["off", "step", "reset"], required=True)
ap.add_argument("--root", default=HERE)
ap.add_argument("--label", default="")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
import isaacgym_amd  # noqa: E402
from isaacgym_amd import scene  # noqa: E402

golden = json.load(open(os.path.join(HERE, "tests", "golden", "task_cfgs.json")))
for name, n in (("HumanoidPingpongTiltG1", 16384), ("HumanoidPingpongTiltNESSparse27DOFG1", 4096)):
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[name])
    if args.mode != "off":
        block = dict(golden[name]["task"]["task"]["randomization_params"])
        if args.mode == "reset":
            block["apply_at"] = "reset"
        cfg["task"] = dict(randomize=True, randomization_params=block)
    task = isaacgym_amd.make(seed=1, task=name, num_envs=n, sim_device="cuda:0", rl_device="cuda:0", cfg=cfg)
    acts = [(torch.rand(task.num_envs, task.num_actions, device="cuda:0") * 2 - 1) for _ in range(8)]
    task.reset()
    for s in range(700):                 # past the first redraw of every mode and one `frequency` period of the per-step mode
        task.step(acts[s & 7])
    torch.cuda.synchronize()
    us = []
    for w in range(args.windows):
        t0 = time.perf_counter()
        for s in range(args.steps):
            task.step(acts[s & 7])
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / args.steps * 1e6)
    print(json.dumps({"label": args.label, "mode": args.mode, "task": name, "num_envs": n, "us_per_step_median": round(statistics.median(us), 2),
                      "us_per_step_windows": [round(u, 2) for u in us], "steps_per_window": args.steps,
                      "module": os.path.dirname(isaacgym_amd.__file__)}), flush=True)
    del task
