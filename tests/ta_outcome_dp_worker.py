"""One rank of a PPOTrainer(outcomes=True) run on the 27-dof task for tests/test_ta_outcome_gpu.py, started as a fresh child process under
torch.distributed.run (two gloo ranks sharing cuda:0).  Trains --epochs epochs and writes every epoch's returned statistics to
<out>/rank<r>.pt."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import isaacgym_amd  # noqa: E402
from isaacgym_amd import ppo, scene  # noqa: E402

TASK = "HumanoidPingpongTiltNESSparse27DOFG1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--num-envs", type=int, default=128)
    ap.add_argument("--episode-length", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--minibatch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    rank, dev = ppo.init_rank("gloo")
    cfg = scene.default_task_cfg("TA")
    cfg["env"]["episodeLength"] = a.episode_length
    task = isaacgym_amd.make(seed=a.seed + rank, task=TASK, num_envs=a.num_envs, multi_gpu=True, device=dev, cfg=cfg)
    tr = ppo.PPOTrainer(task, ppo.PPOConfig(minibatch_size=a.minibatch), seed=a.seed + rank, outcomes=True)
    assert tr.multi and tr.rank == rank
    results = []
    for _ in range(a.epochs):
        results.append({k: v.detach().cpu().clone() for k, v in tr.train_epoch().items()})
    torch.cuda.synchronize()
    os.makedirs(a.out, exist_ok=True)
    torch.save(dict(results=results, own=tr.outcome.cpu().clone(), world=tr.world), os.path.join(a.out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
