"""The trainer's score meter and run loop on the MI355X (isaacgym_amd.ppo.GameMeter / fit, include/ppenv_ppo_meter.h): the two kernels
against their host build byte for byte, against the trainer's existing episode bookkeeping, inside PPOTrainer.train_epoch, and `fit`
with its best checkpoint, its stop on score_to_win and its resume.  Bounds: tests/test_ppo_meter_host.py's (the kernels and the host
build add the same terms in the same order: every byte equal), and tests/ppo_reference.py's episodes_loop bound for the cross-check.
The tasks run with env.episodeLength 12, so games finish within every horizon.  Need a real MI355X.

Graph replay: nothing captures the trainer's epoch today.  The meter's launches read no host-side counter (their arguments are sizes,
strides and device pointers that do not change from call to call), so a captured update replays like an eager one: tested below."""
import os

import numpy as np
import pytest

import play_shim_binding as ps
import ppo_meter_shim_binding as ms
from test_play_gpu import DEV, T4, TT, make_plain
from test_ppo_meter_host import ENVS, HORIZONS, WINDOWS, WORDS

pytestmark = pytest.mark.gpu

START = 8                                                              # the scripted burst (steps 10 .. 13) falls into every horizon length


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def scripted(num_envs, num_agents, h, integer=False):
    """Three consecutive horizons of h steps: [3, h, rows] rewards and done words."""
    rows, steps = num_envs * num_agents, START + 3 * h
    rews = ps.rewards(steps, rows, seed=6 + num_envs, integer=integer)[START:]
    dones = ps.scripted_dones(steps, num_envs, num_agents, words=WORDS)[START:]
    return rews.reshape(3, h, rows), dones.reshape(3, h, rows)


def on_device(torch, rews, dones, strided):
    """[3, h, rows] on the device: contiguous horizons as RolloutCollector holds them, or row-strided views of wider buffers one row down
    (every row then starts at an address that is no multiple of 16 bytes for an odd width)."""
    if not strided:
        return torch.from_numpy(rews).to(DEV), torch.from_numpy(dones).to(DEV)
    k, h, rows = rews.shape
    r = torch.full((k, h + 2, rows + 3), 1e9, dtype=torch.float32, device=DEV)
    d = torch.ones((k, h + 2, rows + 3), dtype=torch.int64, device=DEV)
    r[:, 1:-1, 1:rows + 1], d[:, 1:-1, 1:rows + 1] = torch.from_numpy(rews).to(DEV), torch.from_numpy(dones).to(DEV)
    return r[:, 1:-1, 1:rows + 1], d[:, 1:-1, 1:rows + 1]


@pytest.mark.parametrize("h", HORIZONS)
@pytest.mark.parametrize("num_agents", [1, 2])
@pytest.mark.parametrize("num_envs", ENVS + [1000, 4096])
def test_kernels_match_the_host_build_byte_for_byte(torch_cuda, num_envs, num_agents, h):
    torch = torch_cuda
    from isaacgym_amd.ppo import GameMeter
    for k, w in enumerate(WINDOWS):
        integer, strided = k == 1, k != 0
        rews, dones = scripted(num_envs, num_agents, h, integer)
        r, d = on_device(torch, rews, dones, strided)
        dev, again, host = (GameMeter(num_envs, num_agents, w, DEV), GameMeter(num_envs, num_agents, w, DEV), ms.HostMeter(num_envs, num_agents, w))
        for i in range(3):
            dev.update(r[i], d[i])
            host.update(rews[i], dones[i])
            got, want = dev.state_bytes(), host.state_bytes()
            what = f"W {w}, horizon {i}"
            assert got[0] == want[0], f"{what}: cur_reward"
            assert got[1] == want[1], f"{what}: cur_len"
            assert got[2] == want[2], f"{what}: meter {ms.meter_dict(got[2])} vs {ms.meter_dict(want[2])}"
        for i in range(3):
            again.update(r[i], d[i])
        assert again.state_bytes() == dev.state_bytes()                # bitwise equal run to run
        m = ms.meter_dict(dev.state_bytes()[2])
        f = dev.fields()                                               # the device views name the same words
        assert m["games_total"] > 0 and int(f["games_total"]) == m["games_total"] and int(f["current_size"]) == m["current_size"] <= w
        assert float(f["mean_reward"]) == m["mean_reward"] and float(f["mean_length"]) == m["mean_length"] and int(f["updates"]) == m["updates"]


def test_update_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.ppo import GameMeter
    gm = GameMeter(8, 2, 5, DEV)
    r, d = torch.zeros((4, 16), device=DEV), torch.zeros((4, 16), dtype=torch.int64, device=DEV)
    gm.update(r, d)
    for bad_r, bad_d in ((r[:, :8], d[:, :8]), (r, d.int()), (r.double(), d), (torch.zeros((4, 32), device=DEV)[:, ::2], d), (r.cpu(), d), (r[0], d[0]),
                         (r[:3], d)):
        with pytest.raises(ValueError, match="update"):
            gm.update(bad_r, bad_d)


def test_captured_update_replays_like_eager(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.ppo import GameMeter
    num_envs, num_agents, h, w = 513, 2, 32, 3
    rews, dones = scripted(num_envs, num_agents, h)
    r, d = on_device(torch, rews, dones, strided=False)
    eager, cap = GameMeter(num_envs, num_agents, w, DEV), GameMeter(num_envs, num_agents, w, DEV)
    for i in range(3):
        eager.update(r[i], d[i])
    r_in, d_in = r[0].clone(), d[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.update(r_in, d_in)                                         # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    cap.load_state_dict({"meter": torch.zeros_like(cap.snapshot())})   # ... and its effect undone: the empty meter, the envs at zero
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.update(r_in, d_in)
    assert cap.state_bytes()[2] == bytes(40)                           # capturing launched nothing
    for i in range(3):
        r_in.copy_(r[i])
        d_in.copy_(d[i])
        graph.replay()
    torch.cuda.synchronize()
    assert cap.state_bytes() == eager.state_bytes()


# ------------------------------------------------------------------------------------------------------- inside the trainer
def make_trainer(name=TT, num_envs=256, seed=3, **cfg):
    from isaacgym_amd import ppo
    task = make_plain(name, num_envs, seed)
    cfg.setdefault("minibatch_size", 8192)
    return ppo.PPOTrainer(task, ppo.PPOConfig(**cfg), seed=seed)


def params(tr):
    return [p.detach().clone() for p in tr.learner.parameters()] + [tr.logstd.clone()]


def test_meter_agrees_with_the_trainers_episode_bookkeeping(torch_cuda):
    torch = torch_cuda
    import ppo_reference as pr
    from isaacgym_amd.ppo import GameMeter
    tr = make_trainer()
    gm = GameMeter(256, 1, 1 << 20, DEV)                               # a window no run fills: mean x size is the sum of all returns
    tr.collect()
    rews, dones = tr.col.rewards.cpu().numpy(), tr.col.dones.cpu().numpy()
    ref = pr.episodes_loop(rews, dones, np.zeros(256), np.zeros(256))
    ep = tr._episodes().cpu().numpy()
    gm.update(tr.col.rewards, tr.col.dones)
    f = {k: v.item() for k, v in gm.fields().items()}
    assert ref["count"] >= 256                                         # episodeLength 12: every env finished at least twice
    assert f["games_total"] == f["current_size"] == ref["count"] == int(ep[2])
    got_sum, got_len = f["mean_reward"] * f["current_size"], f["mean_length"] * f["current_size"]
    print(f"meter sum of returns {got_sum!r}, fp64 loop {ref['sum_ret']!r}, _episodes {float(ep[0])!r}, bound {ref['bound']:.3g}")
    assert abs(got_sum - ref["sum_ret"]) <= ref["bound"]
    assert abs(got_len - ref["sum_len"]) <= 1e-9 * ref["sum_len"]      # integers through fp64 means


@pytest.mark.parametrize("name,rows", [(TT, 256), (T4, 512)])
def test_trainer_meter_changes_nothing_else_and_equals_a_host_replay(torch_cuda, name, rows):
    torch = torch_cuda
    a, b = make_trainer(name), make_trainer(name)
    assert a.rows == b.rows == rows and a.meter.num_agents == rows // 256 and a.meter.games_to_track == 100
    b.meter.update = lambda rewards, dones: None                       # the second trainer never runs its meter
    host = ms.HostMeter(256, rows // 256, 100)
    for e in range(2):
        if e > 0 and hasattr(torch.cuda, "set_sync_debug_mode"):
            torch.cuda.set_sync_debug_mode("error")                    # train_epoch still reads nothing on the host
            try:
                ra = a.train_epoch()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            ra = a.train_epoch()
        rb = b.train_epoch()
        assert set(ra) == set(rb) and {"meter_return", "meter_length", "meter_games"} <= set(ra)
        for k in ra:
            if not k.startswith("meter_"):
                assert torch.equal(ra[k], rb[k]), f"epoch {e + 1}: {k}"
        assert int(rb["meter_games"]) == 0
        host.update(a.col.rewards.cpu().numpy(), a.col.dones.cpu().numpy())
        want = host.read()
        assert want["current_size"] > 0
        assert (ra["meter_return"].item(), ra["meter_length"].item(), ra["meter_games"].item()) == \
            (want["mean_reward"], want["mean_length"], want["current_size"]), f"epoch {e + 1}"
        assert ra["meter_return"].dtype == torch.float64 and ra["meter_return"].dim() == 0
        assert a.meter.state_bytes() == host.state_bytes()
    for x, y in zip(params(a), params(b)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------- fit
def test_fit_writes_a_best_checkpoint_that_plays(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import ppo
    from isaacgym_amd.play import Player
    from isaacgym_amd.policy import RLGamesPolicy
    tr = make_trainer(save_best_after=1, games_to_track=10)
    res = ppo.fit(tr, str(tmp_path), "run", print_every=0, max_epochs=4)
    nn = tmp_path / "nn"
    assert (res["epochs"], res["epoch"], res["stopped"], res["reason"]) == (4, 4, False, "max_epochs")
    assert res["paths"]["latest"] == str(nn / "run.pth") and res["paths"]["best"] == str(nn / "run_best.pth") and res["paths"]["won"] is None
    assert sorted(os.listdir(nn)) == ["run.pth", "run_best.pth"]
    assert res["best_score"] == tr.last_mean_rewards > ppo.NO_SCORE
    ck = torch.load(nn / "run_best.pth", map_location="cpu", weights_only=True)
    assert ck["last_mean_rewards"] == res["best_score"] and ck["meter"]["meter"].numel() == 40
    assert ms.meter_dict(ck["meter"]["meter"].numpy().tobytes())["mean_reward"] == res["best_score"]      # saved in the epoch that set it
    policy = RLGamesPolicy.load(str(nn / "run_best.pth"), DEV)
    out = Player(make_plain(TT, 64, 21), policy, games_num=8, poll_every=16, max_steps=2000).run()
    assert out["games"] >= 8 and np.isfinite(out["av_reward"])


def test_fit_stops_on_score_to_win(torch_cuda, tmp_path):
    from isaacgym_amd import ppo
    tr = make_trainer(save_best_after=1, games_to_track=10, score_to_win=-1e9)
    res = ppo.fit(tr, str(tmp_path), "run", print_every=0, max_epochs=4)
    assert (res["epochs"], res["stopped"], res["reason"]) == (1, True, "score_to_win")          # episodeLength 12: games finish in the first horizon
    won = f"run_ep_1_rew_{res['best_score']}.pth"
    assert sorted(os.listdir(tmp_path / "nn")) == sorted(["run.pth", "run_best.pth", won]) and res["paths"]["won"] == str(tmp_path / "nn" / won)


def test_fit_resumes(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import ppo
    kw = dict(save_best_after=1, games_to_track=10)
    whole = make_trainer(**kw)
    ppo.fit(whole, str(tmp_path / "whole"), "run", print_every=0, max_epochs=4)
    a = make_trainer(**kw)
    first = ppo.fit(a, str(tmp_path / "split"), "run", print_every=0, max_epochs=2)
    latest, best = tmp_path / "split" / "nn" / "run.pth", tmp_path / "split" / "nn" / "run_best.pth"
    assert first["epoch"] == 2 and first["paths"]["best"] == str(best)
    # the same env state as the uninterrupted run (what test_ppo_gpu.test_checkpoint_serves_and_resumes promises equality for): a trainer
    # that played the same two epochs, everything load() restores spoiled, then load and two more
    b = make_trainer(**kw)
    for _ in range(2):
        b.train_epoch()
    with torch.no_grad():
        for p in b.learner.parameters():
            p.add_(0.5)
        b.opt.state.zero_()
        b.meter._meter.fill_(7)
    b.last_mean_rewards = 123.0
    b.load(str(latest))
    assert b.last_mean_rewards == a.last_mean_rewards == first["best_score"] and b.epoch == 2
    assert b.meter.state_bytes()[2] == a.meter.state_bytes()[2] and not b.meter.cur_len.any() and not b.meter.cur_reward.any()
    seen = []
    train_epoch = b.train_epoch
    b.train_epoch = lambda: (train_epoch(), seen.append(b.epoch))[0]
    second = ppo.fit(b, str(tmp_path / "split"), "run", print_every=0, max_epochs=4)
    assert seen == [3, 4] and (second["epochs"], second["epoch"]) == (2, 4)                      # max_epochs is the total
    for x, y in zip(params(whole), params(b)):
        assert torch.equal(x, y)
    # a fresh process's resume: a new trainer, load, continue.  The best score travels: with one no run reaches, _best.pth stays as it is
    a.last_mean_rewards = 1e9
    a.save(str(latest))
    before = best.read_bytes()
    c = make_trainer(**kw)
    c.load(str(latest))
    assert (c.epoch, c.frame, c.last_mean_rewards) == (2, 2 * 32 * 256, 1e9)
    third = ppo.fit(c, str(tmp_path / "split"), "run", print_every=0, max_epochs=4)
    assert (third["epochs"], third["epoch"], third["paths"]["best"], third["best_score"]) == (2, 4, None, 1e9)
    assert best.read_bytes() == before
    # a checkpoint from before the meter: load() accepts it
    ck = torch.load(latest, map_location="cpu", weights_only=True)
    del ck["meter"], ck["last_mean_rewards"]
    torch.save(ck, tmp_path / "old.pth")
    c.load(str(tmp_path / "old.pth"))
    assert c.last_mean_rewards == ppo.NO_SCORE


def test_cli_trains_resumes_and_plays(torch_cuda, tmp_path, capsys):
    from isaacgym_amd import play, ppo
    common = ["--task", TT, "--num-envs", "256", "--minibatch-size", "8192", "--save-best-after", "1", "--games-to-track", "20", "--print-every", "1",
              "--out", str(tmp_path)]
    res = ppo.main(common + ["--max-epochs", "4"])
    nn = tmp_path / "nn"
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch ")]
    assert [l.split()[1] for l in lines] == ["1", "2", "3", "4"] and all(" score " in l and l.endswith(" games)") for l in lines)
    assert res["epoch"] == 4 and (nn / f"{TT}.pth").exists()
    assert res["paths"]["best"] == str(nn / f"{TT}_best.pth") and (nn / f"{TT}_best.pth").exists()      # games finish within 128 steps of the default task
    res = ppo.main(common + ["--max-epochs", "6", "--checkpoint", str(nn / f"{TT}.pth")])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("epoch ")]
    assert [l.split()[1] for l in lines] == ["5", "6"] and (res["epochs"], res["epoch"]) == (2, 6) and "resumed " in out
    got = play.main(["--task", TT, "--checkpoint", str(nn / f"{TT}_best.pth"), "--num-envs", "64", "--games", "8", "--poll-every", "16", "--max-steps", "3000"])
    assert got["steps_played"] > 0
