"""One rank of a data-parallel PPOTrainer(critic_inputs=...) run on the 7-dof task for tests/test_ppo_critic_input_gpu.py, started as a
fresh child process under torch.distributed.run (two gloo ranks sharing cuda:0).  Trains --epochs epochs under ADR and a random action
delay with the tables and the delays shown to the critic, and writes the parameters, Adam's moments, the loss scale, the actor's
privileged columns (master and fp16 image), the privileged statistics right after the start-up broadcast and this rank's privileged rows
to <out>/rank<r>.pt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import isaacgym_amd  # noqa: E402
from isaacgym_amd import ppo, scene  # noqa: E402

TASK = "HumanoidPingpongTiltG1"
DIMS = {"link_mass_scale": dict(start=(0.9, 1.1), limit=(0.6, 1.4), step=0.05), "friction_scale": dict(start=(1.0, 1.0), limit=(0.4, 1.6), step=0.1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=21)
    a = ap.parse_args()
    rank, dev = ppo.init_rank("gloo")
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[TASK])
    cfg["env"]["episodeLength"] = 5
    task = isaacgym_amd.make(seed=a.seed + rank, task=TASK, num_envs=a.num_envs, multi_gpu=True, device=dev, cfg=cfg)
    tr = ppo.PPOTrainer(task, ppo.PPOConfig(horizon_length=4, minibatch_size=64, mini_epochs=2, init_scale=512.0), seed=a.seed + rank, action_delay=(0, 2),
                        adr=dict(dims=DIMS, boundary_frac=0.5, min_games=1000, t_low=0.0, t_high=1e9), critic_inputs=("tables", "latency"))
    assert tr.multi and tr.rank == rank and tr.critic_inputs() == dict(names=["tables", "latency"], columns=[8, 1], P=9)
    lr, n = tr.learner, tr.num_obs
    cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
    start_stats = cpu([getattr(lr.priv_rms, k) for k in ("running_mean", "running_var", "count", "mean", "inv_std")])
    for _ in range(a.epochs):
        tr.train_epoch()
    torch.cuda.synchronize()
    os.makedirs(a.out, exist_ok=True)
    torch.save(dict(params=cpu(lr.parameters() + [tr.logstd]), exp_avg=cpu(tr.opt.exp_avg), exp_avg_sq=cpu(tr.opt.exp_avg_sq),
                    scaler=tr.opt.state[tr.opt.cur].cpu().clone(), actor_priv32=lr.w32[0][0][:, n:].cpu().clone(),
                    actor_priv16=lr.net.w[0][0][:, n:].cpu().clone(), critic_priv32=lr.w32[0][1][:, n:].cpu().clone(), start_stats=start_stats,
                    priv=tr.col.priv.cpu().clone(), world=tr.world), os.path.join(a.out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
