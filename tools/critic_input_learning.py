#!/usr/bin/env python3
"""One learning run under the README's ADR example, with or without privileged critic inputs (PPOTrainer(critic_inputs=); DESIGN §6
"Privileged critic inputs"): --epochs epochs of the 7-dof task at --num-envs envs under ADR of the link masses and the friction
(--adr-low / --adr-high: the README's thresholds), seed --seed.  Per epoch it keeps c_loss, the score and — from the collector's own
buffers — the explained variance of the returns by the values, 1 - Var(returns - values) / Var(returns), all on the device; one host
read at the end.  Reports the means over the last --window epochs and ADR's final ranges.  One JSON line."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--critic-inputs", default="")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--adr-low", type=float, default=-5660.0)
    ap.add_argument("--adr-high", type=float, default=-5550.0)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    import isaacgym_amd
    from isaacgym_amd.ppo import PPOConfig, PPOTrainer
    task = isaacgym_amd.make(seed=args.seed, task=args.task, num_envs=args.num_envs)
    adr = dict(dims={"link_mass_scale": dict(start=(1.0, 1.0), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(1.0, 1.0), limit=(0.4, 1.6), step=0.1)},
               boundary_frac=0.25, min_games=256, t_low=args.adr_low, t_high=args.adr_high)
    tr = PPOTrainer(task, PPOConfig(), seed=args.seed, adr=adr, critic_inputs=args.critic_inputs)
    H = tr.cfg.horizon_length
    rows = []
    for _ in range(args.epochs):
        out = tr.train_epoch()
        with torch.no_grad():
            ret, val = tr.col.returns, tr.col.values[:H]
            ev = 1.0 - (ret - val).var() / ret.var().clamp(min=1e-12)
        rows.append(torch.stack([out["c_loss"].double(), ev.double(), out["meter_return"].double(), out["meter_games"].double(), out["mean_return"].double()]))
    t = torch.stack(rows).cpu()
    w = t[-args.window:]
    table = tr.adr.table()
    print(json.dumps(dict(task=args.task, critic_inputs=tr.critic_inputs(), seed=args.seed, num_envs=args.num_envs, epochs=args.epochs, window=args.window,
                          c_loss=float(w[:, 0].mean()), explained_variance=float(w[:, 1].mean()), score=float(t[-1, 2]), score_games=int(t[-1, 3]),
                          mean_return=float(w[:, 4].mean()), c_loss_first=float(t[:args.window, 0].mean()), explained_variance_first=float(t[:args.window, 1].mean()),
                          adr_names=list(tr.adr.names), adr_lo=[round(float(x), 4) for x in table["lo"]], adr_hi=[round(float(x), 4) for x in table["hi"]])), flush=True)


if __name__ == "__main__":
    main()
