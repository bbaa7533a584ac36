"""One rank of a data-parallel PPOTrainer run for tests/test_ppo_multi_gpu.py, started as a fresh child process (by
torch.distributed.run, or directly for a one-rank world).  Trains --epochs epochs and writes what the tests compare to
<out>/rank<r>.pt: parameters, log-std, Adam moments, scaler state, the returned statistics of every epoch, the input statistics,
and the state before the last epoch's learning.  --capture also records the last epoch's local gradients (before the all-reduce),
the tensors the all-reduce left, and the gradients the optimizer stepped on."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import isaacgym_amd  # noqa: E402
from isaacgym_amd import distributed as D  # noqa: E402
from isaacgym_amd import ppo  # noqa: E402


class _Capture:
    """Stands in for the trainer's GradientBuckets: copies every bucket before its collective, keeps the tensors for after it."""

    def __init__(self, buckets):
        self.buckets, self.local, self.tensors = buckets, [], []

    def __call__(self, name, tensors):
        self.local = [] if name == "heads" else self.local           # the heads' bucket opens every step: keep the last step's
        self.tensors = [] if name == "heads" else self.tensors
        self.local += [t.clone() for t in tensors]                   # enqueued before the collective reads the tensor
        self.tensors += list(tensors)
        self.buckets(name, tensors)

    def wait(self):
        self.buckets.wait()


def _snapshot(tr):
    cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
    return dict(params=cpu(tr.learner.parameters() + [tr.logstd]), exp_avg=cpu(tr.opt.exp_avg), exp_avg_sq=cpu(tr.opt.exp_avg_sq),
                scaler=tr.opt.state[tr.opt.cur].cpu().clone())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--task", default="HumanoidPingpongTiltG1")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--minibatch", type=int, default=8192)
    ap.add_argument("--mini-epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--backend", default="none", choices=["none", "gloo", "nccl"], help="none: one process, no group")
    ap.add_argument("--force", action="store_true", help="PPOTrainer(force=True): the collectives in a one-rank world")
    ap.add_argument("--same-shard", action="store_true", help="every rank: the same seed and env_id_offset 0")
    ap.add_argument("--inf-rank", type=int, default=-1, help="this rank puts an inf into its advantages in the last epoch")
    ap.add_argument("--capture", action="store_true")
    ap.add_argument("--sync-check", action="store_true", help="epochs after the first under torch.cuda.set_sync_debug_mode('error')")
    a = ap.parse_args()
    cfg = ppo.PPOConfig(minibatch_size=a.minibatch, mini_epochs=a.mini_epochs)
    if a.backend == "none":
        rank, seed = 0, a.seed
        tr = ppo.PPOTrainer(isaacgym_amd.make(seed=seed, task=a.task, num_envs=a.num_envs), cfg, seed=seed)
    else:
        rank, dev = ppo.init_rank(a.backend, force=a.force)
        assert rank == D.rank_info()[0]
        seed = a.seed if a.same_shard else a.seed + rank
        if a.same_shard:                                             # every rank the single process's envs: env_id_offset 0
            task = isaacgym_amd.make(seed=seed, task=a.task, num_envs=a.num_envs, sim_device=str(dev), rl_device=str(dev))
        else:
            task = isaacgym_amd.make(seed=seed, task=a.task, num_envs=a.num_envs, multi_gpu=True, device=dev)
        tr = ppo.PPOTrainer(task, cfg, seed=seed, force=a.force)
        assert tr.multi and tr.rank == rank
    results, pre, cap = [], None, None
    for e in range(a.epochs):
        if e == a.epochs - 1:
            pre = _snapshot(tr)                                      # one minibatch per epoch: the state before the last step
            if a.capture and tr.buckets is not None:
                cap = tr.buckets = _Capture(tr.buckets)
            if rank == a.inf_rank:
                prepare = tr.prepare

                def poisoned():
                    prepare()
                    tr.adv[0] = float("inf")
                tr.prepare = poisoned
        if a.sync_check and e > 0:
            torch.cuda.set_sync_debug_mode("error")                 # a host synchronisation inside the epoch raises
            try:
                res = tr.train_epoch()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            res = tr.train_epoch()
        results.append({k: v.detach().cpu().clone() for k, v in res.items()})
    torch.cuda.synchronize()
    out = dict(_snapshot(tr), results=results, pre=pre, frame=tr.frame, world=tr.world,
               collectives=tr.buckets.buckets.collectives if cap is not None else tr.buckets.collectives if tr.buckets is not None else 0,
               input_mean=tr.learner.rms.running_mean.cpu().clone(), input_var=tr.learner.rms.running_var.cpu().clone())
    if cap is not None:
        out.update(local=[t.cpu() for t in cap.local], reduced=[t.detach().cpu().clone() for t in cap.tensors],
                   sum_grads=[t.detach().cpu().clone() for t in tr.learner.gradients() + [tr.g_logstd]])
    os.makedirs(a.out, exist_ok=True)
    torch.save(out, os.path.join(a.out, f"rank{rank}.pt"))
    if a.backend != "none":
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
