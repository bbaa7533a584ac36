"""Sensor noise and dropouts in the player on the MI355X (isaacgym_amd.play: Player(obs_noise=, obs_drop=, action_noise=, action_drop=,
*_columns=), the sweep axes of those names; include/ppenv_sensor.h): what zero levels promise, the noised observation against
isaacgym_amd.sensor.reference step by step across resets, held ball columns, paired replicas, repeated commands, and the result's
`sensor` with its JSON files.  64 envs, a freshly initialised policy, 12-step episodes.  Need a real MI355X."""
import json

import numpy as np
import pytest

import sensor_shim_binding as sb
from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)
from test_rng_streams_gpu import E_MEASURED

pytestmark = pytest.mark.gpu

TT, T4 = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1"
TASKS = pytest.mark.parametrize("name", [TT, T4], ids=["7dof", "4actor"])
DEV = "cuda:0"
N, GAMES, STEPS = 64, 3, 30                 # 30 control steps of 12-step episodes: every env restarts at least twice


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def player(name, checkpoint, **kw):
    from isaacgym_amd.play import Player
    return Player(make_plain(name, N, 21), load_policy(checkpoint(TT)), games_num=GAMES, poll_every=8, max_steps=2000, **kw)


def drive(torch, pl, steps=STEPS):
    """start() and `steps` steps -> per step (the env's clean observation, the done of the step before or None, policy_obs, actions,
    applied_actions), cloned."""
    out = []
    pl.start()
    for _ in range(steps):
        raw, done = pl._obs.clone(), None if pl._done_prev is None else pl._done_prev.clone()
        pl.step()
        out.append((raw, done, pl.policy_obs.clone(), pl.actions.clone(), pl.applied_actions.clone()))
    return out


@TASKS
def test_zero_cells_are_the_sweep_without_the_axes(torch_cuda, checkpoint, name):
    torch = torch_cuda
    from isaacgym_amd.play import Sweep
    zero = player(name, checkpoint, sweep=Sweep([{"obs_noise": 0.0, "obs_drop": 0.0, "action_noise": 0.0, "action_drop": 0.0}] * 2, paired=True))
    plain = player(name, checkpoint, sweep=Sweep([{}] * 2, paired=True))
    keyword = player(name, checkpoint, sweep=Sweep([{}] * 2, paired=True), obs_noise=0.0, action_drop=0.0, obs_noise_columns="ball_pos")
    for pl in (zero, plain, keyword):
        assert pl._obs_sensor is None and pl._act_sensor is None                            # not built: no allocation, no launch
    runs = [drive(torch, pl) for pl in (zero, plain, keyword)]
    for t in range(STEPS):
        for other in runs[1:]:
            assert all(same_bits(torch, a, b) for a, b in zip(runs[0][t][2:], other[t][2:])), t
    for g in range(2):
        assert zero.stats.group_state_bytes(g) == plain.stats.group_state_bytes(g) == keyword.stats.group_state_bytes(g)
    assert zero.applied_actions is zero.actions
    for pl in (zero, plain, keyword):
        pl.end_sweep()
    res, res0 = player(name, checkpoint, sweep=Sweep([{"obs_noise": 0.0}] * 2, paired=True)).run(), player(name, checkpoint, sweep=Sweep([{}] * 2, paired=True)).run()
    assert "sensor" not in res and "sensor" not in res0
    strip = lambda r: {k: v for k, v in r.items() if k not in ("seconds", "groups")}
    assert strip(res) == strip(res0)
    assert [{k: v for k, v in g.items() if k != "cell"} for g in res["groups"]] == [{k: v for k, v in g.items() if k != "cell"} for g in res0["groups"]]
    assert res["groups"][0]["cell"] == {"obs_noise": 0.0}


@TASKS
def test_ball_position_noise_follows_the_reference_across_resets(torch_cuda, checkpoint, name):
    torch = torch_cuda
    from isaacgym_amd import sensor
    pl = player(name, checkpoint, obs_noise=0.05, obs_noise_columns="ball_pos")
    A, rows = pl.num_agents, pl.num_agents * N
    assert pl._act_sensor is None and pl._obs_sensor.width == 80 and pl._obs_sensor.rows == rows
    ref = sensor.reference(rows, 80, A, sigma=np.full(rows, 0.05, np.float32), drop=np.zeros(rows, np.float32), columns=sensor.columns(pl.task, "ball_pos", 80),
                           seed=pl.sensor_seed, channel=sensor.SENSING)
    touched, restarts = np.zeros(80, bool), 0
    for t, (raw, done, seen, _, _) in enumerate(drive(torch, pl)):
        x, got = raw.cpu().numpy(), seen.cpu().numpy()
        ref.push(x, None if done is None else done.cpu().numpy())
        sb.compare(got.view(np.uint32), dict(out=ref.out.view(np.uint32), s=ref.s, mag=ref.mag), 4 * E_MEASURED, (name, t))
        touched |= (got.view(np.uint32) != x.view(np.uint32)).any(axis=0)
        assert (got[:, 74:77] != x[:, 74:77]).mean() > 0.99, t
        restarts += 0 if done is None else int((done.cpu().numpy().reshape(-1, A)[:, 0] != 0).sum())
    assert list(np.flatnonzero(touched)) == [74, 75, 76]                                     # non-zero exactly on the ball position
    assert restarts >= 2 * N and ref.episode.min() >= 3
    assert np.array_equal(pl._obs_sensor.episode.cpu().numpy(), ref.episode) and np.array_equal(pl._obs_sensor.age.cpu().numpy(), ref.age)
    assert same_bits(torch, pl.applied_actions, pl.actions)


@TASKS
def test_a_certain_dropout_holds_each_episodes_first_ball_observation(torch_cuda, checkpoint, name):
    torch = torch_cuda
    pl = player(name, checkpoint, obs_drop=1.0, obs_drop_columns="ball_pos,ball_vel")
    A = pl.num_agents
    first, changed, live = None, 0, False
    for t, (raw, done, seen, _, _) in enumerate(drive(torch, pl)):
        if done is None:
            first = raw[:, 74:80].clone()
        else:
            start = (done.view(N, A)[:, :1] != 0).expand(N, A).reshape(-1, 1)                 # agent 0's word, for every row of the env
            first = torch.where(start, raw[:, 74:80], first)
            changed += int(start.sum())
        assert same_bits(torch, seen[:, 74:80], first) and same_bits(torch, seen[:, :74], raw[:, :74]), (name, t)
        live |= not same_bits(torch, raw[:, 74:80], seen[:, 74:80])
    assert changed >= 2 * N * A and live                                                     # every env restarted twice, and the held ball is not the live one


def test_paired_cells_with_equal_values_are_bitwise_replicas(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Sweep
    cell = {"obs_noise": 0.02, "obs_drop": 0.2, "action_noise": 0.05, "action_drop": 0.3}
    pl = player(TT, checkpoint, sweep=Sweep([cell, dict(cell)], paired=True), obs_noise_columns="ball_pos=1,ball_vel=4")
    assert pl._obs_sensor.key_period == pl._act_sensor.key_period == N // 2
    differs = False
    for t, (_, _, seen, actions, applied) in enumerate(drive(torch, pl)):
        for x in (seen, actions, applied):
            assert same_bits(torch, x[:N // 2], x[N // 2:]), t
        differs |= not same_bits(torch, actions, applied)
    assert differs and pl.stats.group_state_bytes(0) == pl.stats.group_state_bytes(1)
    pl.end_sweep()


def test_action_dropouts_repeat_the_last_applied_command(torch_cuda, checkpoint):
    torch = torch_cuda
    pl = player(TT, checkpoint, action_drop=0.5)
    assert pl._obs_sensor is None and pl._act_sensor.width == pl.task.num_actions
    prev, fresh, repeated = None, 0, 0
    for t, (_, done, seen, actions, applied) in enumerate(drive(torch, pl)):
        new = (applied.view(torch.int32) == actions.view(torch.int32)).all(dim=1)
        if prev is None:
            assert new.all()
        else:
            old = (applied.view(torch.int32) == prev.view(torch.int32)).all(dim=1)
            assert (new | old).all(), t
            assert new[done != 0].all(), t                                                   # an episode's first command is never dropped
            repeated += int((old & ~new).sum())
        fresh += int(new.sum())
        prev = applied
    assert repeated > STEPS * N // 4 and fresh > STEPS * N // 4


def test_the_result_and_the_json_files_carry_the_axes(torch_cuda, checkpoint, capsys, tmp_path):
    from isaacgym_amd import play
    cells_file, diff_file = tmp_path / "cells.json", tmp_path / "diff.json"
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "64", "--games", "6", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--sweep", "obs_noise=0,0.01", "--paired", "--paired-diff", "--obs-drop", "0.1", "--obs-noise-columns", "ball_pos=1,ball_vel=4",
                     "--obs-drop-columns", "ball_pos,ball_vel", "--sweep-out", str(cells_file), "--paired-out", str(diff_file)])
    want = dict(obs_noise=[0.0, 0.01], obs_drop=[0.1, 0.1], action_noise=[0.0, 0.0], action_drop=[0.0, 0.0],
                columns=dict(obs_noise_columns="ball_pos=1,ball_vel=4", obs_drop_columns="ball_pos,ball_vel", action_noise_columns=None, action_drop_columns=None))
    assert res["sensor"] == want
    lines = capsys.readouterr().out.splitlines()
    assert [l for l in lines if l.startswith("sensor: ")] == ["sensor: obs_noise 0,0.01; obs_drop 0.1,0.1; action_noise 0,0; action_drop 0,0; "
                                                              "obs_noise_columns ball_pos=1,ball_vel=4; obs_drop_columns ball_pos,ball_vel"]
    assert [c.split(":")[0] for c in lines if c.startswith("cell obs_noise=")] == ["cell obs_noise=0", "cell obs_noise=0.01"]
    assert [w["cell"] for w in json.loads(cells_file.read_text())] == [{"obs_noise": 0.0}, {"obs_noise": 0.01}]
    written = json.loads(diff_file.read_text())
    assert written["sensor"] == want and written["cells"][0]["diff"] == 0.0 and "latency" not in written
    plain = play.Player(make_plain(TT, 64, 21), load_policy(checkpoint(TT)), games_num=GAMES, action_noise=0.1)
    assert plain.run()["sensor"] == dict(obs_noise=[0.0], obs_drop=[0.0], action_noise=[0.1], action_drop=[0.0], columns=dict.fromkeys(want["columns"]))
    for kw, text in ((dict(obs_noise=-1.0), "'obs_noise': a noise amplitude"), (dict(action_drop=1.5), "'action_drop': a dropout probability"),
                     (dict(obs_noise_columns="ball"), "obs_noise_columns: 'ball': unknown column group"), (dict(action_drop_columns="0:9"), "action_drop_columns: '0:9': the range")):
        with pytest.raises(ValueError, match=text):
            play.Player(make_plain(TT, 64, 21), load_policy(checkpoint(TT)), **kw)
