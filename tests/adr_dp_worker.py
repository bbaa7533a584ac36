"""One rank of a PPOTrainer(adr=...) run on the 7-dof task for tests/test_ppo_adr_gpu.py, started as a fresh child process under
torch.distributed.run (two gloo ranks sharing cuda:0).  Trains --epochs epochs and writes ADR's ranges and per-slot state, and the totals
this rank folded in every epoch before they were summed over the ranks, to <out>/rank<r>.pt."""
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
    ap.add_argument("--t-move", type=float, required=True)
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--episode-length", type=int, default=12)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=21)
    a = ap.parse_args()
    rank, dev = ppo.init_rank("gloo")
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[TASK])
    cfg["env"]["episodeLength"] = a.episode_length
    task = isaacgym_amd.make(seed=a.seed + rank, task=TASK, num_envs=a.num_envs, multi_gpu=True, device=dev, cfg=cfg)
    tr = ppo.PPOTrainer(task, ppo.PPOConfig(horizon_length=16, minibatch_size=256), seed=a.seed + rank,
                        adr=dict(dims=DIMS, boundary_frac=0.5, min_games=2, t_low=a.t_move, t_high=a.t_move))
    assert tr.multi and tr.rank == rank
    own, fold = [], tr.adr.fold

    def recording_fold():
        tot = fold()
        own.append(tot.cpu().clone())                      # this rank's totals, before the trainer sums them over the ranks in place
        return tot
    tr.adr.fold = recording_fold
    for _ in range(a.epochs):
        tr.train_epoch()
    torch.cuda.synchronize()
    os.makedirs(a.out, exist_ok=True)
    state = {k: getattr(tr.adr, k).cpu().clone() for k in ("range", "acc_n", "acc_q", "games", "dropped", "mean", "widened", "narrowed")}
    torch.save(dict(state=state, own=own, world=tr.world, offset=tr.adr.env_id_offset), os.path.join(a.out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
