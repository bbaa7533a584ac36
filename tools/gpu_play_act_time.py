#!/usr/bin/env python3
"""What the actuator usage accounting costs per control step (include/ppenv_play_act.h), next to the episode accounting and the env
step it follows: pp_play_act_accumulate, pp_play_group_accumulate and task.step, eager launches, at the 27-dof task's 4096 envs (AoS
inputs) and the 7-dof task's 16384 envs (SoA inputs).  Device events around 400 back-to-back calls after 64 warm-up calls, the three
alternating, five rounds, the median reported; the accumulates read the tensors the env left and rotate over eight done buffers in
which every env finishes with probability 1 / 64 (the folds run in nearly every workgroup), never frozen (games_num 2^40).
Run on the GPU box:  python tools/gpu_play_act_time.py [--out profiles/play_act_time.jsonl]
Each size runs in its own process under its own time limit; the first that fails ends the run."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (("HumanoidPingpongTiltNESSparse27DOFG1", 4096), ("HumanoidPingpongTiltG1", 16384))
LIMIT_S = 240


def child(name, n):
    import torch
    import isaacgym_amd
    from isaacgym_amd import play
    task = isaacgym_amd.make(seed=3, task=name, num_envs=n)
    env, dev = task.env, task.device
    limits, names = play.actuator_limits(task)
    D = len(names)
    thr = dict(play.ACT_THRESHOLDS, action_clip=float(task.clip_actions))
    act = play.ActuatorStats(n, 1, D, 1 << 40, limits, thr, dev)
    grp = play.GroupStats(n, 1, 1, 1 << 40, dev)
    inputs = (env.dof_states[..., 0], env.dof_states[..., 1], env.dof_force_tensor) if hasattr(env, "dof_states") else (env.dof_pos.T, env.dof_vel.T, env.dof_force.T)
    actions = [torch.rand(n, task.num_actions, device=dev) * 2 - 1 for _ in range(8)]
    task.reset()
    rews = []
    for t in range(48):                                           # past the first resets; the last eight steps' rewards are the accumulates' inputs
        _, rew, _, _ = task.step(actions[t % 8])
        if t >= 40:
            rews.append(rew.clone())
    gen = torch.Generator(device=dev).manual_seed(5)              # an env finishes every 64th call: nearly every chunk of 256 folds somebody
    dones = [(torch.rand(n, device=dev, generator=gen) < 1.0 / 64).to(torch.int64) for _ in range(8)]
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    calls = dict(env_step=lambda t: task.step(actions[t % 8]), play_group_accumulate=lambda t: grp.accumulate(rews[t % 8], dones[t % 8]),
                 play_act_accumulate=lambda t: act.accumulate(*inputs, actions[t % 8], dones[t % 8]),
                 play_act_accumulate_nobody_finishes=lambda t: act.accumulate(*inputs, actions[t % 8], zero))

    def timed(fn, reps=400):
        for t in range(64):
            fn(t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(reps):
            fn(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    rounds = {k: [] for k in calls}
    for _ in range(5):
        for k, fn in calls.items():
            rounds[k].append(timed(fn))
    tot = act.read()[0]
    print(json.dumps(dict(task=name, num_envs=n, num_dofs=D, layout="aos" if hasattr(env, "dof_states") else "soa", unit="us per call, eager, median of 5 x 400",
                          finishing_envs_per_call=sum(int((d != 0).sum()) for d in dones) / len(dones), act_games=tot["games"], act_samples=tot["samples"],
                          **{k: round(statistics.median(v), 3) for k, v in rounds.items()}, **{k + "_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in rounds.items()})),
          flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        lines = []
        for name, n in SIZES:
            res = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, str(n)], check=True,
                                 capture_output=True, text=True)
            line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            lines.append(line)
        if out:
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
