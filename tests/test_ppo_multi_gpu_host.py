"""Data-parallel PPO without a GPU: the CLI refuses --multi-gpu in a one-rank world, the ctypes mirror of ppenv_ppo_adam matches the C
header, and GradientBuckets(mean=False) leaves the sums in place."""
import ctypes as C
import os
import socket
import subprocess
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cli_refuses_multi_gpu_in_a_one_rank_world():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, "-m", "isaacgym_amd.ppo", "--multi-gpu"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode != 0
    assert "--multi-gpu needs a world above 1" in r.stderr and "torch.distributed.run" in r.stderr, r.stderr
    r = subprocess.run([sys.executable, "-m", "isaacgym_amd.ppo", "--force-dist"], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode != 0 and "--force-dist belongs to --multi-gpu" in r.stderr, r.stderr


def test_adam_struct_mirror_matches_the_c_header(tmp_path):
    from isaacgym_amd import ppo
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ppenv_ppo.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ppenv_ppo_adam), offsetof(ppenv_ppo_adam, beta2), offsetof(ppenv_ppo_adam, eps),
               offsetof(ppenv_ppo_adam, max_norm), offsetof(ppenv_ppo_adam, truncate), offsetof(ppenv_ppo_adam, growth_factor),
               offsetof(ppenv_ppo_adam, backoff_factor), offsetof(ppenv_ppo_adam, growth_interval), offsetof(ppenv_ppo_adam, world));
        return 0;
    }'''
    exe = str(tmp_path / "adam_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    A = ppo.PPOAdam
    names = [f[0] for f in A._fields_]
    assert names == ["beta1", "beta2", "eps", "max_norm", "truncate", "growth_factor", "backoff_factor", "growth_interval", "world"]
    assert got == [C.sizeof(A)] + [getattr(A, n).offset for n in names[1:]]
    assert A.world.offset == 40 and C.sizeof(A) == 48


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _buckets_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from isaacgym_amd import distributed as D
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    flat = torch.arange(8.0) * (rank + 1)                # two adjacent views of one buffer: one collective; a separate tensor: its own
    views, other = [flat[:6].view(2, 3), flat[6:]], torch.full((3,), float(rank))
    b = D.GradientBuckets(mean=False)
    b("layer", views + [other])
    assert b.collectives == 2 and b.bytes == 11 * 4 and b.names == ["layer"]
    b.wait()
    res["flat"], res["other"] = flat, other
    for mean in (True, False):
        b = D.GradientBuckets(mean=mean)
        t = [torch.full((5,), float(rank + 1)), torch.full((2, 3), 0.5 * (rank + 1))]
        b("layer", t)
        b.wait()
        res[mean] = t
    if rank == 0:
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_buckets_mean_false_keeps_the_sums(tmp_path):
    out = str(tmp_path / "buckets.pt")
    mp.spawn(_buckets_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = torch.load(out)
    assert torch.equal(res[True][0], torch.full((5,), 1.5)) and torch.equal(res[True][1], torch.full((2, 3), 0.75))     # default: the mean
    assert torch.equal(res[False][0], torch.full((5,), 3.0)) and torch.equal(res[False][1], torch.full((2, 3), 1.5))    # mean=False: the sum
    assert torch.equal(res["flat"], torch.arange(8.0) * 3) and torch.equal(res["other"], torch.ones(3))
