"""Data-parallel PPOTrainer (group=...) on the MI355X: ranks are fresh child processes (tests/ppo_dp_worker.py) under
torch.distributed.run, two gloo ranks sharing cuda:0; RCCL with one rank; the CLI on two devices when there are two.  Each child writes
its state to tmp_path and the test compares the files.  Plus DeviceAdam(world=...) on gradient sums in this process."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

UNITS = 6                                                           # hidden layers of the network (policy.UNITS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ppo_dp_worker.py")
SAME = ["--task", "HumanoidPingpongTiltG1", "--num-envs", "1024", "--minibatch", "8192", "--epochs", "3", "--seed", "7"]
ONE_STEP = ["--task", "HumanoidPingpongTiltG1", "--num-envs", "1024", "--minibatch", "32768", "--mini-epochs", "1", "--epochs", "2", "--seed", "7"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _check(r):
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"


def _ranks(out, args, nproc=2, timeout=900):
    """nproc ranks of the worker (at most 2 processes on the GPU beside this one); stops the test at the first failure."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", f"--nproc_per_node={nproc}", WORKER, "--out", str(out)] + args
    _check(subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT))


def _one(out, args, env=None, timeout=900):
    full = dict(os.environ, **(env or {}))
    _check(subprocess.run([sys.executable, WORKER, "--out", str(out)] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=full))


def _load(path):
    import torch
    return torch.load(path, weights_only=False)


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """The trainer without a group, the reference of the identical-shard and one-rank RCCL runs."""
    out = tmp_path_factory.mktemp("single")
    _one(out, SAME)
    return _load(out / "rank0.pt")


def _state_equal(a, b):
    import torch
    for key in ("params", "exp_avg", "exp_avg_sq"):
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.equal(x, y), f"{key} {i}"
    assert torch.equal(a["scaler"], b["scaler"]), (a["scaler"], b["scaler"])


def _results_equal(a, b, episodes=1):
    """The statistics train_epoch() returned, bitwise; the finished-episode count of `a` is `episodes` times b's (a sum over ranks)."""
    import torch
    assert len(a["results"]) == len(b["results"])
    for e, (x, y) in enumerate(zip(a["results"], b["results"])):
        assert x.keys() == y.keys()
        for k in x:
            want = y[k] * episodes if k == "episodes" else y[k]
            assert torch.equal(x[k], want), f"epoch {e}: {k} {x[k]} vs {want}"


def test_identical_shards_reproduce_one_rank_bitwise(single, tmp_path):
    """g + g and / 2 are exact: two gloo ranks on the same shard step exactly as one trainer (wiring, ordering, the folded mean)."""
    _ranks(tmp_path, SAME + ["--backend", "gloo", "--same-shard"])
    for r in range(2):
        got = _load(tmp_path / f"rank{r}.pt")
        assert got["world"] == 2 and got["frame"] == 3 * 32 * 1024 * 2
        assert got["collectives"] == UNITS + 1                 # per step: one per layer, the log-std inside the heads' one
        _state_equal(got, single)
        _results_equal(got, single, episodes=2)
        assert int(got["scaler"][2]) == 3 * 20                      # every step taken: 4 minibatches x 5 mini-epochs x 3 epochs


def test_real_shards_stay_in_lockstep_and_step_on_the_mean(tmp_path):
    import torch
    _ranks(tmp_path, ONE_STEP + ["--backend", "gloo", "--capture"])
    r0, r1 = _load(tmp_path / "rank0.pt"), _load(tmp_path / "rank1.pt")
    _state_equal(r0, r1)
    _results_equal(r0, r1)                                          # the statistics are global
    assert not torch.equal(r0["input_mean"], r1["input_mean"])      # the normalisers are per rank
    # the all-reduce left fl(g0 + g1) in every bucket
    assert len(r0["local"]) == len(r0["reduced"]) > 2
    for i, (a, b, s0, s1) in enumerate(zip(r0["local"], r1["local"], r0["reduced"], r1["reduced"])):
        assert not torch.equal(a, b), f"bucket tensor {i}: the shards gave identical gradients"
        assert torch.equal(s0, a + b) and torch.equal(s1, a + b), f"bucket tensor {i}"
    # the step: clip_grad_norm_ + torch.optim.Adam on the mean (fp64, as test_ppo_gpu.test_clip_adam_matches_torch)
    pre = r0["pre"]
    scale, step = float(pre["scaler"][0:1].view(torch.float32)), int(pre["scaler"][2])
    assert int(r0["scaler"][2]) == step + 1 and int(r0["scaler"][3]) == int(pre["scaler"][3])
    tp = [torch.nn.Parameter(p.double().clone()) for p in pre["params"]]
    topt = torch.optim.Adam(tp, lr=2e-5, eps=1e-8, foreach=False)
    for p, g, m, v in zip(tp, r0["sum_grads"], pre["exp_avg"], pre["exp_avg_sq"]):
        p.grad = (g / 2).double() / scale                           # fl(g_sum / world), then the unscale
        topt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    torch.nn.utils.clip_grad_norm_(tp, 10.0)
    topt.step()
    for i, (p, q) in enumerate(zip(r0["params"], tp)):
        q = q.detach()
        torch.testing.assert_close(p.double(), q, rtol=1e-6, atol=1e-7 * float(q.abs().max()), msg=f"parameter {i}")
        st = topt.state[tp[i]]
        for mine, theirs, what in ((r0["exp_avg"][i], st["exp_avg"], "exp_avg"), (r0["exp_avg_sq"][i], st["exp_avg_sq"], "exp_avg_sq")):
            torch.testing.assert_close(mine.double(), theirs, rtol=1e-6, atol=1e-6 * float(theirs.abs().max()), msg=f"{what} {i}")


def test_nonfinite_on_one_rank_skips_the_step_on_every_rank(tmp_path):
    import torch
    _ranks(tmp_path, ONE_STEP + ["--backend", "gloo", "--inf-rank", "1"])
    for r in range(2):
        got = _load(tmp_path / f"rank{r}.pt")
        pre, res = got["pre"], got["results"][-1]
        assert int(res["skipped"]) == 1, r
        scale0 = float(pre["scaler"][0:1].view(torch.float32))
        assert float(res["scale"]) == scale0 * 0.5, r
        assert int(got["scaler"][2]) == int(pre["scaler"][2]), r         # no Adam step counted
        for key in ("params", "exp_avg", "exp_avg_sq"):
            for i, (x, y) in enumerate(zip(pre[key], got[key])):
                assert torch.equal(x, y), f"rank {r}: {key} {i}"


@pytest.mark.parametrize("world", [2, 3])
def test_device_adam_steps_on_the_mean_of_sums(world):
    """DeviceAdam(world=w) on gradient sums against clip_grad_norm_ + torch.optim.Adam on fl(sum / w), in fp64; and world=1 / 0 are the
    default, bit for bit."""
    import torch
    from isaacgym_amd import ppo
    gen = torch.Generator(device="cuda").manual_seed(world)
    shapes = [(512, 320), (512, 512), (64, 48), (27,), (1,)]
    params = [torch.randn(s, device="cuda", generator=gen) * 0.1 for s in shapes]
    grads = [torch.zeros(s, device="cuda") for s in shapes]
    scale, lrate = 1024.0, 1e-3
    opt = ppo.DeviceAdam(params, grads, lrate, max_norm=10.0, init_scale=scale, world=world)
    tp = [torch.nn.Parameter(p.double().clone()) for p in params]
    topt = torch.optim.Adam(tp, lr=lrate, eps=1e-8, foreach=False)
    for step, std in enumerate([1e-1, 1e-1, 1e-3, 1e-1]):             # clip active, then not, then active again
        for g in grads:
            g.copy_(sum(torch.randn(g.shape, device="cuda", generator=gen) * std * scale for _ in range(world)))
        for p, g in zip(tp, grads):
            p.grad = (g / world).double() / scale
        norm = torch.nn.utils.clip_grad_norm_(tp, 10.0)
        topt.step()
        opt.step()
        torch.testing.assert_close(opt.fields()["grad_norm"].double().cpu(), norm.cpu(), rtol=1e-6, atol=0)
        for i, (p, q) in enumerate(zip(params, tp)):
            q = q.detach()
            torch.testing.assert_close(p.double(), q, rtol=1e-6, atol=1e-7 * float(q.abs().max()), msg=f"step {step}: parameter {i}")
            st = topt.state[tp[i]]
            for mine, theirs in ((opt.exp_avg[i], st["exp_avg"]), (opt.exp_avg_sq[i], st["exp_avg_sq"])):
                torch.testing.assert_close(mine.double(), theirs, rtol=1e-6, atol=1e-6 * float(theirs.abs().max()), msg=f"step {step}: moment {i}")
    assert int(opt.fields()["step"]) == 4 and int(opt.fields()["skipped"]) == 0
    # one rank: world 1 and 0 are today's kernel
    base = [p.clone() for p in params]
    runs = []
    for w in (None, 1, 0):
        ps = [p.clone() for p in base]
        o = ppo.DeviceAdam(ps, grads, lrate, init_scale=scale) if w is None else ppo.DeviceAdam(ps, grads, lrate, init_scale=scale, world=w)
        for _ in range(3):
            o.step()
        runs.append(ps + o.exp_avg + o.exp_avg_sq + [o.state[o.cur]])
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x, y)


def test_device_adam_divides_by_world_with_correct_rounding():
    """One step from zero moments at world 3, scale 1, no clip: exp_avg = fl(fl(0.1) x fl(g_sum / 3)), bitwise.  A multiply by the rounded
    reciprocal differs on part of these values, so this pins the IEEE division rl_games' all_grads / world_size performs."""
    import torch
    from isaacgym_amd import ppo
    g_sum = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 1e-3
    want = torch.tensor(0.1, dtype=torch.float32) * (g_sum / 3)
    assert not torch.equal(want, torch.tensor(0.1, dtype=torch.float32) * (g_sum * torch.tensor(1.0 / 3.0, dtype=torch.float32)))
    p, g = torch.zeros(4096, device="cuda"), g_sum.cuda()
    opt = ppo.DeviceAdam([p], [g], 1e-3, truncate=False, init_scale=1.0, dynamic=False, world=3)
    opt.step()
    assert torch.equal(opt.exp_avg[0].cpu(), want)


def test_rccl_one_rank_equals_the_trainer_without_a_group(single, tmp_path):
    """The collectives on RCCL with one rank (force=True): bitwise the trainer without a group, layers + 1 collectives per step, and no
    synchronisation in an epoch that torch.cuda's sync debug mode detects."""
    env = dict(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    _one(tmp_path, SAME + ["--backend", "nccl", "--force", "--sync-check"], env=env)
    got = _load(tmp_path / "rank0.pt")
    assert got["world"] == 1 and got["collectives"] == UNITS + 1
    _state_equal(got, single)
    _results_equal(got, single)


def test_two_devices_nccl(tmp_path):
    """The worker and the CLI under torch.distributed.run on two GPUs over RCCL: the ranks stay identical, rank 0 alone writes the checkpoint,
    and RLGamesPolicy serves it."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _ranks(tmp_path / "ranks", ["--task", "HumanoidPingpongTiltG1", "--num-envs", "1024", "--minibatch", "8192", "--epochs", "2", "--backend", "nccl"])
    r0, r1 = _load(tmp_path / "ranks" / "rank0.pt"), _load(tmp_path / "ranks" / "rank1.pt")
    _state_equal(r0, r1)
    _results_equal(r0, r1)
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc_per_node=2", "-m", "isaacgym_amd.ppo", "--multi-gpu",
           "--dist-backend", "nccl", "--task", "HumanoidPingpongTiltG1", "--num-envs", "1024", "--max-epochs", "2", "--minibatch-size", "8192",
           "--print-every", "1", "--out", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    _check(r)
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and f"frames {2 * 32 * 1024 * 2} " in lines[-1], r.stdout      # rank 0 prints, global frames
    files = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs]
    assert files == [str(out / "nn" / "HumanoidPingpongTiltG1.pth")], files
    from isaacgym_amd.policy import RLGamesPolicy
    pol = RLGamesPolicy.load(files[0], "cuda:0")
    obs = torch.randn(64, pol.net.num_obs, device="cuda:0")
    act, _ = pol.act(obs, deterministic=True)
    assert act.shape == (64, pol.net.num_actions) and bool(torch.isfinite(act).all())
