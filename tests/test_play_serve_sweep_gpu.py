"""Serve sweeps and paired groups through the Player on the MI355X (isaacgym_amd.play: Sweep serve axes, paired=; VecTask.set_serve_plan).

The swept Player against the test's own loop on a second task of the same seed, which sets the sweep's tables (task.env.set_randomization)
and its serve plan (task.set_serve_plan) by hand and feeds one EpisodeStats per group the group's slices: byte-equal totals.  Then what
pairing promises (equal cells: equal groups), that the task is left as found, that nothing new is launched when no plan is asked for, and
the trainer's refusal.  The tasks run with env.episodeLength 12.  Need a real MI355X."""
import json

import numpy as np
import pytest

from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
N_ENVS = 128


def rows_of(task):
    return task.env.DR_TABLE_ROWS


def manual_loop(torch, task, policy, sweep, games_num, steps):
    """The swept run by hand -> the list of EpisodeStats, one per group."""
    from isaacgym_amd.play import EpisodeStats
    G, A = len(sweep), task.num_agents
    S = task.num_envs // G
    w = A * S
    tables = sweep.tables(rows_of(task), task.num_envs)
    if tables:
        task.env.set_randomization(**tables)
    task.set_serve_plan(sweep.serve_cells(task.env.serve_defaults()), paired=sweep.paired)
    task.reset_idx()
    policy._counter = 0
    obs = task.reset()["obs"]
    stats = [EpisodeStats(S, A, games_num, DEV) for _ in range(G)]
    for _ in range(steps):
        actions, _ = policy.act(obs, deterministic=True, seed=0)
        od, rew, done, _ = task.step(actions)
        for g, st in enumerate(stats):
            st.accumulate(rew[g * w:(g + 1) * w], done[g * w:(g + 1) * w])
        obs = od["obs"]
    torch.cuda.synchronize()
    return stats


def without_clock(res):
    return {k: v for k, v in res.items() if k not in ("seconds", "steps_played")}


def sweep_and_compare(torch, name, path, sweep, games_num, poll_every=16):
    from isaacgym_amd.play import Player, group_summary, sum_totals, summarize
    pl = Player(make_plain(name, N_ENVS, 21), load_policy(path), games_num=games_num, poll_every=poll_every, max_steps=2000, sweep=sweep)
    res = pl.run()
    G, A = len(sweep), pl.num_agents
    assert res["steps_played"] < 2000 and res["steps_played"] % poll_every == 0
    assert len(res["groups"]) == G and all(g["complete"] and g["games"] >= games_num and g["paired"] == sweep.paired for g in res["groups"])
    stats = manual_loop(torch, make_plain(name, N_ENVS, 21), load_policy(path), sweep, games_num, res["steps_played"])
    per = pl.stats.read()
    for g, st in enumerate(stats):
        want = st.read()
        assert pl.stats.group_state_bytes(g) == st.state_bytes(), (name, g)                   # cur_reward, cur_steps and the 72 bytes of totals
        assert per[g] == want, (name, g)
        assert res["groups"][g] == group_summary(sweep.cells[g], want, A, games_num, sweep.paired), (name, g)
    top = summarize(sum_totals([st.read() for st in stats]), A)
    assert without_clock(res) == dict(top, groups=res["groups"])
    assert pl.task._serve_plan is None and pl.task.env.serve_plan is None                     # cleared by run()
    return pl, res


# ------------------------------------------------------------------------------------------------------ 11. Player = the test's own loop
@pytest.mark.parametrize("name,table_axis", [(TT, "friction_scale"), (TA, "dof_stiffness_scale"), (T4, "restitution_scale")])
def test_player_serve_sweep_matches_manual_loop(torch_cuda, checkpoint, name, table_axis):
    from isaacgym_amd.play import Sweep
    path = checkpoint(TT if name == T4 else name)
    speeds = [4.0, 6.0] if name == TA else [6.5, 9.0]
    sweep = Sweep.grid({"serve_speed": speeds, table_axis: [0.8, 1.2]})
    pl, res = sweep_and_compare(torch_cuda, name, path, sweep, 24)
    assert [g["cell"] for g in res["groups"]] == [{"serve_speed": s, table_axis: f} for s in speeds for f in (0.8, 1.2)]
    assert len({g["av_reward"] for g in res["groups"]}) == 4
    pl, res = sweep_and_compare(torch_cuda, name, path, Sweep([{}, {}], paired=True), 24)    # paired alone: the configured ranges, no table
    assert [g["cell"] for g in res["groups"]] == [{}, {}]


def test_polling_does_not_change_the_serve_swept_result(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    sweep = Sweep.grid({"serve_speed": [6.5, 9.0], "friction_scale": [0.5, 1.0]}, paired=True)
    out = []
    for poll in (1, 64):
        pl = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=40, poll_every=poll, max_steps=2000, sweep=sweep)
        res = pl.run()
        out.append((without_clock(res), pl.stats.state_bytes(), res["steps_played"]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2] < out[1][2] == 64


# ------------------------------------------------------------------------------------------------------ 12. equal paired cells
@pytest.mark.parametrize("name", [TT, TA])
def test_equal_paired_cells_give_equal_groups(torch_cuda, checkpoint, name):
    from isaacgym_amd.play import Player, Sweep
    speed = 5.2 if name == TA else 8.3
    for cells in ([{}] * 4, [{"serve_speed": speed}] * 4):
        res = Player(make_plain(name, N_ENVS, 21), load_policy(checkpoint(name)), games_num=24, poll_every=16, max_steps=2000,
                     sweep=Sweep(cells, paired=True)).run()
        first = res["groups"][0]
        assert first["games"] >= 24 and first["paired"]
        for g in res["groups"][1:]:
            for k in ("av_reward", "av_steps", "games", "reward_min", "reward_max", "reward_std"):
                assert g[k] == first[k], (name, k)
    unpaired = Player(make_plain(name, N_ENVS, 21), load_policy(checkpoint(name)), games_num=24, poll_every=16, max_steps=2000, sweep=Sweep([{"serve_speed": (speed - 0.3, speed + 0.3)}] * 4)).run()
    assert len({g["av_reward"] for g in unpaired["groups"]}) == 4 and not unpaired["groups"][0]["paired"]


# ------------------------------------------------------------------------------------------------------ 13. restore
def zero_action_rows(torch, task, steps):
    actions = torch.zeros((task.num_envs * task.num_agents, task.num_actions), device=DEV)
    out = []
    for _ in range(steps):
        task.step(actions)
        out.append((task.obs_buf.clone(), task.rew_buf.clone(), task.reset_buf.clone()))
    torch.cuda.synchronize()
    return out


def test_task_is_left_as_found(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Player, Sweep
    task, fresh = make_plain(TT, N_ENVS, 21), make_plain(TT, N_ENVS, 21)
    Player(task, load_policy(checkpoint(TT)), games_num=24, poll_every=16, max_steps=2000, sweep=Sweep.grid({"serve_speed": [6.5, 9.0]}, paired=True)).run()
    assert task.env.step_kernel_name == fresh.env.step_kernel_name
    task.reset_idx()
    fresh.reset_idx()
    a, b = zero_action_rows(torch, task, 40), zero_action_rows(torch, fresh, 40)
    assert sum(int(r.sum()) for _, _, r in b) >= 2 * N_ENVS
    for t in range(40):
        assert np.array_equal(a[t][0].cpu().numpy().view(np.uint32), b[t][0].cpu().numpy().view(np.uint32)), t
        assert np.array_equal(a[t][1].cpu().numpy().view(np.uint32), b[t][1].cpu().numpy().view(np.uint32)), t
        assert torch.equal(a[t][2], b[t][2]), t


class Interrupted(Exception):
    pass


def test_plan_is_cleared_after_an_exception(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    pl = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=40, poll_every=4, max_steps=2000, sweep=Sweep([{}, {}], paired=True))

    def on_poll(tot):
        assert pl.task._serve_plan is not None and int(pl.task._serve_plan.count.min()) >= 1   # set while the run is under way
        raise Interrupted

    with pytest.raises(Interrupted):
        pl.run(on_poll=on_poll)
    assert pl.task._serve_plan is None and pl.task.env.serve_plan is None and pl.steps_played == 4


# ------------------------------------------------------------------------------------------------------ 14. nothing new when off
def test_no_apply_launch_without_a_plan(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    calls = []

    def counting(task):
        inner = task.env.apply_serve_plan

        def wrapped(*a, **kw):
            calls.append(a)
            return inner(*a, **kw)
        task.env.apply_serve_plan = wrapped
        return task
    path = checkpoint(TT)
    for sweep in (None, Sweep.grid({"friction_scale": [0.5, 1.0]})):
        res = Player(counting(make_plain(TT, N_ENVS, 21)), load_policy(path), games_num=16, poll_every=16, max_steps=2000, sweep=sweep).run()
        assert res["games"] >= 16 and calls == []
    res = Player(counting(make_plain(TT, N_ENVS, 21)), load_policy(path), games_num=16, poll_every=16, max_steps=2000,
                 sweep=Sweep.grid({"friction_scale": [0.5, 1.0]}, paired=True)).run()
    assert len(calls) == res["steps_played"] + 1 and len(calls[0]) == 1 and calls[1] == ()  # the id variant after the reset, then one per step


# ------------------------------------------------------------------------------------------------------ 15. refusals
def test_trainer_refuses_a_task_with_a_plan(torch_cuda):
    from isaacgym_amd import ppo
    task = make_plain(TT, 64, 3)
    task.set_serve_plan([{"serve_speed": 7.0}])
    with pytest.raises(ValueError, match="clear_serve_plan"):
        ppo.PPOTrainer(task, ppo.PPOConfig(minibatch_size=32 * 64), seed=1)
    task.clear_serve_plan()
    ppo.PPOTrainer(task, ppo.PPOConfig(minibatch_size=32 * 64), seed=1)


def test_player_refusals(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    with pytest.raises(ValueError, match="serve axes are serve_speed, serve_tilt, serve_tilt_z$"):
        Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), sweep=Sweep.grid({"ball_y": [-0.2, 0.0]}))
    ta = make_plain(TA, N_ENVS, 21)
    with pytest.raises(ValueError, match="outcomes=True with a sweep"):
        Player(ta, load_policy(checkpoint(TA)), sweep=Sweep([{}, {}], paired=True), outcomes=True)
    pl = Player(ta, load_policy(checkpoint(TA)), sweep=Sweep.grid({"ball_y": [-0.2, 0.0], "ball_z": [1.0]}), games_num=8, poll_every=16, max_steps=600)
    res = pl.run()
    assert [g["cell"] for g in res["groups"]] == [{"ball_y": -0.2, "ball_z": 1.0}, {"ball_y": 0.0, "ball_z": 1.0}]


def test_cli_serve_sweep(torch_cuda, checkpoint, capsys, tmp_path):
    from isaacgym_amd import play
    out_file = tmp_path / "cells.json"
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "128", "--games", "6", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--sweep", "serve_speed=7.5:9:4", "--sweep", "friction_scale=0.5,1.0", "--paired", "--sweep-out", str(out_file)])
    lines = capsys.readouterr().out.splitlines()
    cells = [l for l in lines if l.startswith("cell ")]
    assert len(cells) == 8 and cells[0].startswith("cell serve_speed=7.5 friction_scale=0.5: games ") and cells[7].startswith("cell serve_speed=9 friction_scale=1: games ")
    written = json.loads(out_file.read_text())
    assert len(written) == len(res["groups"]) == 8 and all(w["paired"] is True for w in written)
    assert [w["cell"] for w in written] == [{"serve_speed": s, "friction_scale": f} for s in (7.5, 8.0, 8.5, 9.0) for f in (0.5, 1.0)]
