"""Sweeping physical parameters across env groups on the MI355X (isaacgym_amd.play: GroupStats, Player(sweep=); include/ppenv_play_group.h).

The kernels: group g's totals, cur_reward and cur_steps must be BYTE FOR BYTE what the single accounting (EpisodeStats: the same kernels
with one group, pinned by tests/test_play_gpu.py against its host build, rl_games' loop and the recorded digests) leaves on the same
device when it is given the group's S envs and the group's slices of the recorded sequences — never frozen, and with a games_num the
groups reach at different steps: a check of the group indexing.  No tolerance anywhere: the sums have the same order.  The Player: the swept run against the test's own loop on a second
task of the same seed, which sets the same tables through task.env.set_randomization and feeds one EpisodeStats per group the slices.
The tasks run with env.episodeLength 12.  Need a real MI355X."""
import json

import numpy as np
import pytest

import play_shim_binding as ps
from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)
from test_play_host import NEVER, STEPS, check_against_loop, rlgames_loop, run_shim

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 63, 3), (1, 65, 2), (2, 129, 3), (1, 257, 2), (1, 300, 3), (2, 300, 2)]      # (num_agents, S, G)


# ------------------------------------------------------------------------------------------------------- the kernels
def sequences(num_agents, S, G, integer):
    N = S * G
    return ps.rewards(STEPS, N * num_agents, seed=6 + N, integer=integer), ps.scripted_dones(STEPS, N, num_agents, words=(1, 2, 1 << 32))


def device_sequence(torch, rews, dones):
    """The recorded [steps, rows] sequences inside larger device buffers, one row down: every step's slice — and every group's slice of it —
    starts at a non-zero offset."""
    r = torch.zeros((rews.shape[0] + 2, rews.shape[1]), dtype=torch.float32, device=DEV)
    d = torch.ones((dones.shape[0] + 2, dones.shape[1]), dtype=torch.int64, device=DEV)
    r[1:-1], d[1:-1] = torch.from_numpy(rews).to(DEV), torch.from_numpy(dones).to(DEV)
    return r[1:-1], d[1:-1]


_REFERENCE = {}


def reference(torch, num_agents, S, G, integer, games_num):
    """Per group, the state bytes of an EpisodeStats(S, num_agents, games_num) fed the group's slices for STEPS steps on this device.
    Computed once per case and shared."""
    key = (num_agents, S, G, integer, games_num)
    if key not in _REFERENCE:
        from isaacgym_amd.play import EpisodeStats
        r, d = device_sequence(torch, *sequences(num_agents, S, G, integer))
        w = num_agents * S
        out = []
        for g in range(G):
            st = EpisodeStats(S, num_agents, games_num, DEV)
            for t in range(STEPS):
                st.accumulate(r[t, g * w:(g + 1) * w], d[t, g * w:(g + 1) * w])
            out.append(st.state_bytes())
        _REFERENCE[key] = out
    return _REFERENCE[key]


def run_grouped(torch, stats, r, d, first=0, steps=STEPS):
    for t in range(first, first + steps):
        stats.accumulate(r[t % STEPS], d[t % STEPS])
    torch.cuda.synchronize()


def assert_groups_equal(stats, ref, what):
    for g, want in enumerate(ref):
        got = stats.group_state_bytes(g)
        for k, name in enumerate(("cur_reward", "cur_steps", "totals")):
            assert len(got[k]) == len(want[k]) and got[k] == want[k], f"{what}: group {g}: {name} differs from the single accounting's"


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("num_agents,S,G", SHAPES)
def test_every_group_is_bytewise_the_single_accounting(torch_cuda, num_agents, S, G, integer):
    torch = torch_cuda
    from isaacgym_amd.play import GroupStats
    rews, dones = sequences(num_agents, S, G, integer)
    r, d = device_sequence(torch, rews, dones)
    st = GroupStats(S, G, num_agents, NEVER, DEV)
    assert (st.num_envs, st.rows) == (S * G, S * G * num_agents)
    run_grouped(torch, st, r, d)
    first = st.state_bytes()
    assert len(first[2]) == 72 * G
    assert_groups_equal(st, reference(torch, num_agents, S, G, integer, NEVER), "never frozen")
    per = st.read()
    assert len(per) == G and all(t["launches"] == STEPS and t["games"] > 0 and len(t["reward"]) == num_agents for t in per)
    w = num_agents * S
    for g in (0, G - 1):                                                                     # ... and rl_games' loop on the group's slice
        ref = rlgames_loop(rews[:, g * w:(g + 1) * w], dones[:, g * w:(g + 1) * w], num_agents, NEVER)
        check_against_loop(per[g], st.group_state_bytes(g), ref, num_agents, exact=integer, what=f"group {g} vs loop")
    if integer and G == 1:                                                                   # the whole struct equals the host build's
        shim = run_shim(rews, dones, num_agents, NEVER)
        assert first == shim.state_bytes()
    st.reset()                                                                               # a second run from reset(): bitwise the first
    cleared = st.read()
    assert all((t["games"], t["steps"], t["launches"]) == (0, 0, 0) and t["reward_min"][0] == np.inf and t["reward_max"][0] == -np.inf for t in cleared)
    run_grouped(torch, st, r, d)
    assert st.state_bytes() == first


@pytest.mark.parametrize("num_agents,S,G", SHAPES)
def test_groups_freeze_on_their_own(torch_cuda, num_agents, S, G):
    torch = torch_cuda
    from isaacgym_amd.play import GroupStats
    rews, dones = sequences(num_agents, S, G, False)
    w = num_agents * S
    slices = [(rews[:, g * w:(g + 1) * w], dones[:, g * w:(g + 1) * w]) for g in range(G)]
    games_num = max(min(rlgames_loop(rw, dn, num_agents, NEVER)["games"] for rw, dn in slices) // 2, 1)      # half the smallest group's final count
    refs = [rlgames_loop(rw, dn, num_agents, games_num) for rw, dn in slices]
    crossings = [ref["broke_at"] for ref in refs]
    assert all(c is not None and c < STEPS - 10 for c in crossings) and (G == 1 or len(set(crossings)) > 1), crossings      # at different steps
    r, d = device_sequence(torch, rews, dones)
    st = GroupStats(S, G, num_agents, games_num, DEV)
    run_grouped(torch, st, r, d)
    assert_groups_equal(st, reference(torch, num_agents, S, G, False, games_num), f"games_num {games_num}")
    per = st.read()
    for g in range(G):
        check_against_loop(per[g], st.group_state_bytes(g), refs[g], num_agents, what=f"group {g} at its crossing")
        assert per[g]["launches"] == crossings[g] + 1 and games_num <= per[g]["games"] <= games_num + S - 1
    frozen = st.state_bytes()
    run_grouped(torch, st, r, d, first=STEPS, steps=40)                                      # every group is frozen: 40 further launches
    assert st.state_bytes() == frozen


def test_accumulate_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.play import GroupStats
    st = GroupStats(4, 2, 2, 5, DEV)
    r, d = torch.zeros(16, device=DEV), torch.zeros(16, dtype=torch.int64, device=DEV)
    st.accumulate(r, d)
    for bad_r, bad_d in ((r[:8], d), (r, d.int()), (r.double(), d), (torch.zeros(32, device=DEV)[::2], d), (r.cpu(), d)):
        with pytest.raises(ValueError, match="GroupStats.accumulate"):
            st.accumulate(bad_r, bad_d)


# ------------------------------------------------------------------------------------------------------- the Player
N_ENVS = 128


def rows_of(task):
    return task.env.DR_TABLE_ROWS


def randomization_of(task):
    return task.env.dr_tables


def manual_loop(torch, task, policy, sweep, games_num, steps):
    """The swept run by hand: the sweep's tables through task.env.set_randomization before the reset, then `steps` control steps with one
    EpisodeStats per group fed the group's slices.  -> the list of EpisodeStats."""
    from isaacgym_amd.play import EpisodeStats
    G, A = len(sweep), task.num_agents
    S = task.num_envs // G
    w = A * S
    task.env.set_randomization(**sweep.tables(rows_of(task), task.num_envs))
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
    assert len(res["groups"]) == G and all(g["complete"] and g["games"] >= games_num for g in res["groups"])
    stats = manual_loop(torch, make_plain(name, N_ENVS, 21), load_policy(path), sweep, games_num, res["steps_played"])
    per = pl.stats.read()
    for g, st in enumerate(stats):
        want, got = st.read(), per[g]
        for k in ("games", "steps", "launches", "reward_min", "reward_max"):                  # integers and extrema
            assert got[k] == want[k], (name, g, k)
        assert pl.stats.group_state_bytes(g) == st.state_bytes(), (name, g)                   # cur_reward, cur_steps and the 72 bytes
        assert res["groups"][g] == group_summary(sweep.cells[g], want, A, games_num), (name, g)
        assert res["groups"][g]["cell"] == sweep.cells[g]
        assert res["groups"][g]["reward_stderr"] == res["groups"][g]["reward_std"] / np.sqrt(want["games"])
    top = summarize(sum_totals([st.read() for st in stats]), A)                               # the top level: the groups summed in group order
    assert without_clock(res) == dict(top, groups=res["groups"])
    assert res["games"] == sum(g["games"] for g in res["groups"])
    assert randomization_of(pl.task) is None                                                  # the handle has no randomisation set any more
    return pl, res


def test_player_sweep_matches_manual_loop(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Player, Sweep
    path = checkpoint(TT)
    sweep = Sweep.grid({"link_mass_scale": [0.7, 1.3], "friction_scale": [0.5, 1.0]})
    pl, res = sweep_and_compare(torch, TT, path, sweep, 40)
    assert [g["cell"] for g in res["groups"]] == [{"link_mass_scale": m, "friction_scale": f} for m in (0.7, 1.3) for f in (0.5, 1.0)]
    assert len({g["av_reward"] for g in res["groups"]}) == 4
    # a following un-swept run on that task is the one a fresh task of the same seed gives
    fresh_task = make_plain(TT, N_ENVS, 21)
    assert pl.task.env.step_kernel_name == fresh_task.env.step_kernel_name
    again = Player(pl.task, load_policy(path), games_num=100, poll_every=16, max_steps=2000)
    fresh = Player(fresh_task, load_policy(path), games_num=100, poll_every=16, max_steps=2000)
    res_again, res_fresh = again.run(), fresh.run()
    assert again.stats.state_bytes() == fresh.stats.state_bytes()
    assert {k: v for k, v in res_again.items() if k != "seconds"} == {k: v for k, v in res_fresh.items() if k != "seconds"}
    assert "groups" not in res_fresh


def test_player_sweep_27dof(torch_cuda, checkpoint):
    from isaacgym_amd.play import Sweep
    pl, res = sweep_and_compare(torch_cuda, TA, checkpoint(TA), Sweep.grid({"dof_stiffness_scale": [0.8, 1.2]}), 32)
    assert pl.task.num_obs == 313 and pl.stats.envs_per_group == 64


def test_player_sweep_4_actor(torch_cuda, checkpoint):
    from isaacgym_amd.play import Sweep
    pl, res = sweep_and_compare(torch_cuda, T4, checkpoint(TT), Sweep.grid({"restitution_scale": [0.8, 1.0]}), 32)
    assert pl.num_agents == 2 and pl.stats.rows == 2 * N_ENVS
    assert all(len(g["per_agent"]) == 2 for g in res["groups"]) and len(res["per_agent"]) == 2


def test_polling_does_not_change_the_swept_result(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    sweep = Sweep.grid({"link_mass_scale": [0.7, 1.3], "friction_scale": [0.5, 1.0]})
    out = []
    for poll in (1, 64):
        pl = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=40, poll_every=poll, max_steps=2000, sweep=sweep)
        res = pl.run()
        out.append((without_clock(res), pl.stats.state_bytes(), res["steps_played"]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2] < out[1][2] == 64                                                        # they stopped at different steps


class Interrupted(Exception):
    pass


def test_sweep_is_cleared_after_an_exception(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    pl = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=40, poll_every=4, max_steps=2000,
                sweep=Sweep.grid({"friction_scale": [0.5, 1.0]}))

    def on_poll(tot):
        assert randomization_of(pl.task) is not None                                          # set while the run is under way
        raise Interrupted

    with pytest.raises(Interrupted):
        pl.run(on_poll=on_poll)
    assert randomization_of(pl.task) is None and pl.steps_played == 4


def test_sweep_refusals(torch_cuda, checkpoint):
    from isaacgym_amd import scene
    from isaacgym_amd.play import Player, Sweep
    from isaacgym_amd.tasks import isaacgym_task_map
    sweep = Sweep.grid({"friction_scale": [0.5, 1.0]})
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[TT])
    cfg["env"]["numEnvs"], cfg["seed"] = N_ENVS, 21
    cfg["task"] = dict(cfg.get("task") or {}, randomize=True)
    randomized = isaacgym_task_map[TT](cfg, DEV, DEV, -1, True, False, False)
    assert randomized.randomize
    with pytest.raises(ValueError, match="randomize: True"):
        Player(randomized, load_policy(checkpoint(TT)), sweep=sweep)
    ta = make_plain(TA, N_ENVS, 21)
    with pytest.raises(ValueError, match="outcomes=True with a sweep"):
        Player(ta, load_policy(checkpoint(TA)), sweep=sweep, outcomes=True)
    assert ta.outcomes is None                                                                # refused before the counts were switched on
    with pytest.raises(ValueError, match="multiple of 3 envs, not 128.*126 and 129"):
        Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), sweep=Sweep.grid({"friction_scale": [0.5, 1.0, 1.5]}))


def test_cli_sweep(torch_cuda, checkpoint, capsys, tmp_path):
    from isaacgym_amd import play
    out_file = tmp_path / "cells.json"
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "126", "--games", "10", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--sweep", "friction_scale=0.5:1.5:3", "--sweep", "restitution_scale=0.8,1.0", "--sweep-out", str(out_file)])
    lines = capsys.readouterr().out.splitlines()
    assert any(l.startswith("av reward: ") and " av steps: " in l for l in lines), lines
    cells = [l for l in lines if l.startswith("cell ")]
    assert len(cells) == 6 and cells[0].startswith("cell friction_scale=0.5 restitution_scale=0.8: games ") and " +- " in cells[0] and " av steps " in cells[0]
    assert cells[5].startswith("cell friction_scale=1.5 restitution_scale=1: games ")
    assert lines.index(cells[0]) > next(i for i, l in enumerate(lines) if l.startswith("av reward: "))          # after the usual summary
    written = json.loads(out_file.read_text())
    assert len(written) == len(res["groups"]) == 6
    assert [w["cell"] for w in written] == [{"friction_scale": f, "restitution_scale": r} for f in (0.5, 1.0, 1.5) for r in (0.8, 1.0)]
    assert all(w["games"] == g["games"] and w["av_reward"] == g["av_reward"] and w["complete"] == g["complete"] for w, g in zip(written, res["groups"]))
