"""Paired differences and per-cell policies on the MI355X (isaacgym_amd.play: PairStats, Player(paired_diff=, baseline=), a sequence of
policies, --against; include/ppenv_play_pair.h).

The kernels against their host build (tests/csrc/play_pair_shim.cpp) on recorded sequences: the table, count, len and the `groups` sums
structs bit for bit.  Then the Player: paired_diff changes no word of the group accounting; its cells are those of the host build and,
within the host test's bound (tests/test_play_pair_host.py: n x 2^-52 x sum|term| per fp64 sum, the integers equal), of the numpy
restatement, both fed the rew / done of the test's own loop on a second task of the same seed; polling; equal cells; the 4-actor task;
one policy per cell; the CLI.  The tasks run with env.episodeLength 12.  Need a real MI355X."""
import ctypes as C
import json

import numpy as np
import pytest

import play_pair_shim_binding as pps
from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
N_ENVS = 4 * 65


def without(res, *keys):
    return {k: v for k, v in res.items() if k not in keys + ("seconds", "steps_played")}


# ------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("S,G,A,M,baseline", pps.SHAPES)
def test_kernels_match_shim(torch_cuda, S, G, A, M, baseline):
    torch = torch_cuda
    from isaacgym_amd.play import PairStats, PlayPairTotals
    rews, dones = pps.streams(S, G, A)
    shim = pps.HostPairs(S, G, A, M, baseline)
    r = torch.zeros((pps.STEPS + 2, rews.shape[1]), dtype=torch.float32, device=DEV)      # every step's slice at a non-zero offset
    d = torch.ones((pps.STEPS + 2, dones.shape[1]), dtype=torch.int64, device=DEV)
    r[1:-1], d[1:-1] = torch.from_numpy(rews).to(DEV), torch.from_numpy(dones).to(DEV)
    st = PairStats(S, G, A, M, baseline, DEV)
    for t in st.cur_reward, st.cur_steps, st.count, st.ret, st.len, st._out:              # garbage: reset() must clear it, reduce overwrite it
        t.fill_(7)
    st.reset()
    for t in range(pps.STEPS):
        st.record(r[1 + t], d[1 + t])
        shim.record(rews[t], dones[t])
    want = b"".join(bytes(s) for s in shim.reduce())
    assert st.state_bytes() == shim.state_bytes()                                           # cur_reward, cur_steps, count, ret, len
    assert st.reduce() == want and len(want) == G * C.sizeof(PlayPairTotals) == G * 80
    assert st.reduce() == want                                                              # overwritten, not accumulated
    got = st.read()
    assert [g["baseline"] for g in got] == list(shim.baseline) and sum(g["pairs"] for g in got) > 0
    with pytest.raises(ValueError, match="record"):
        st.record(r[1][:-1], d[1][:-1])


# ------------------------------------------------------------------------------------------------------- the Player
GRID = {"friction_scale": [0.5, 1.0], "serve_speed": [6.5, 9.0]}


def manual_streams(torch, task, policy, sweep, steps):
    """The swept run by hand, in the shape of test_play_serve_sweep_gpu.manual_loop -> the [steps, rows] rew and done it produced."""
    env = task.env
    tables = sweep.tables(env.DR_TABLE_ROWS, task.num_envs)
    if tables:
        task.env.set_randomization(**tables)
    task.set_serve_plan(sweep.serve_cells(task.env.serve_defaults()), paired=sweep.paired)
    task.reset_idx()
    policy._counter = 0
    obs = task.reset()["obs"]
    rews, dones = [], []
    for _ in range(steps):
        actions, _ = policy.act(obs, deterministic=True, seed=0)
        od, rew, done, _ = task.step(actions)
        rews.append(rew.clone())
        dones.append(done.clone())
        obs = od["obs"]
    torch.cuda.synchronize()
    return torch.stack(rews).cpu().numpy(), torch.stack(dones).cpu().numpy()


def test_paired_diff_leaves_the_groups_alone_and_matches_the_restatement(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep, pair_summary, pair_totals_dict
    sweep = Sweep.grid(GRID, paired=True)
    path = checkpoint(TT)
    plain = Player(make_plain(TT, N_ENVS, 21), load_policy(path), games_num=24, poll_every=16, max_steps=2000, sweep=sweep)
    res0 = plain.run()
    pl = Player(make_plain(TT, N_ENVS, 21), load_policy(path), games_num=24, poll_every=16, max_steps=2000, sweep=sweep, paired_diff=True, baseline=1)
    res = pl.run()
    assert "paired_diff" not in res0 and without(res, "paired_diff") == without(res0)
    assert pl.stats.state_bytes() == plain.stats.state_bytes()
    assert res["steps_played"] >= res0["steps_played"] and res["steps_played"] < 2000
    pd = res["paired_diff"]
    S, G, A, M = 65, 4, 1, 1
    assert pd["complete"] and pd["episodes"] == M == pl.pair_episodes and len(pd["cells"]) == G
    assert all(c["pairs"] == S * M and c["cell"] == g and c["baseline"] == 1 for g, c in enumerate(pd["cells"]))
    rews, dones = manual_streams(torch_cuda, make_plain(TT, N_ENVS, 21), load_policy(path), sweep, res["steps_played"])
    shim = pps.HostPairs(S, G, A, M, 1)
    for t in range(rews.shape[0]):
        shim.record(rews[t], dones[t])
    assert pl.pairs.state_bytes()[2:] == shim.state_bytes()[2:]                              # count, ret, len
    assert pd["cells"] == [pair_summary(g, 1, pair_totals_dict(t, A), A) for g, t in enumerate(shim.reduce())]
    want = pps.numpy_reduce(*pps.numpy_record(rews, dones, S, G, A, M), 1)
    for g, (got, w) in enumerate(zip(pl.pairs.read(), want)):
        pps.check_sums(got, w, A, what=g)
        n = w["pairs"]
        assert pd["cells"][g]["steps_diff"] == w["steps_diff"] / n
        for k, s in (("diff", "diff"), ("cell_mean", "cell"), ("base_mean", "base")):       # a mean is its sum / n: the sum's bound / n, and a rounding on either side
            assert abs(pd["cells"][g][k] - w[s][0] / n) <= 2.0 ** -52 * w["abs_" + s][0] + 2.0 ** -51 * abs(w[s][0] / n), (g, k)
    assert pd["cells"][1]["diff"] == 0.0 and pd["cells"][1]["diff_stderr"] == 0.0 and pd["cells"][1]["steps_diff"] == 0.0
    assert all(pd["cells"][g]["diff"] != 0.0 and pd["cells"][g]["diff_stderr"] > 0.0 for g in (0, 2))      # the cells of the other serve speed (the last axis runs fastest)


def test_polling_does_not_change_the_paired_diff(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    sweep = Sweep.grid(GRID, paired=True)
    out = []
    for poll in (1, 64):
        pl = Player(make_plain(TT, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=24, poll_every=poll, max_steps=2000, sweep=sweep, paired_diff=True,
                    baseline=[1, 0, 3, 2], pair_episodes=2)
        res = pl.run()
        out.append((without(res), pl.stats.state_bytes(), pl.pairs.state_bytes()[2:], res["steps_played"]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert out[0][3] < out[1][3] == 64
    pd = out[0][0]["paired_diff"]
    assert pd["complete"] and pd["episodes"] == 2 and [c["baseline"] for c in pd["cells"]] == [1, 0, 3, 2] and all(c["pairs"] == 130 for c in pd["cells"])
    assert pd["cells"][0]["diff"] == -pd["cells"][1]["diff"] != 0.0 and pd["cells"][0]["diff_stderr"] == pd["cells"][1]["diff_stderr"]      # serve speed 6.5 against 9


@pytest.mark.parametrize("name", [TT, TA])
def test_equal_cells_have_no_difference(torch_cuda, checkpoint, name):
    from isaacgym_amd.play import Player, Sweep
    res = Player(make_plain(name, N_ENVS, 21), load_policy(checkpoint(name)), games_num=24, poll_every=16, max_steps=2000, sweep=Sweep([{}] * 4, paired=True),
                 paired_diff=True, baseline=2).run()
    pd = res["paired_diff"]
    assert pd["complete"] and len(pd["cells"]) == 4
    for c in pd["cells"]:
        assert c["pairs"] == 65 and c["diff"] == 0.0 and c["diff_stderr"] == 0.0 and c["steps_diff"] == 0 and c["cell_mean"] == c["base_mean"], (name, c)


def test_four_actor_task_reports_both_agents(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    res = Player(make_plain(T4, N_ENVS, 21), load_policy(checkpoint(TT)), games_num=24, poll_every=16, max_steps=2000,
                 sweep=Sweep.grid({"serve_speed": [6.5, 9.0], "restitution_scale": [0.8, 1.2]}, paired=True), paired_diff=True).run()
    pd = res["paired_diff"]
    assert pd["complete"]
    for g, c in enumerate(pd["cells"]):
        assert c["pairs"] == 65 and len(c["per_agent"]) == 2
        assert c["per_agent"][0] == {k: c[k] for k in ("diff", "diff_stderr", "cell_mean", "base_mean")}
        assert (c["diff"] == 0.0 and c["per_agent"][1]["diff"] == 0.0) if g == 0 else (g == 1 or c["diff"] != 0.0)      # cells 2, 3: another serve speed


# ------------------------------------------------------------------------------------------------------- one policy per cell
def shifted_state_dict(torch, path, shift=0.3):
    """The checkpoint's file content with `shift` added to the actor's mu bias: another policy of the same shape."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    ck["model"] = dict(ck["model"])
    ck["model"]["a2c_network.mu.bias"] = ck["model"]["a2c_network.mu.bias"] + shift
    return ck


def test_policies_per_cell(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Player, Sweep
    from isaacgym_amd.policy import RLGamesPolicy
    path = checkpoint(TT)
    pA, pB = load_policy(path), RLGamesPolicy(shifted_state_dict(torch, path)["model"], DEV)
    two = Sweep([{}, {}], paired=True)

    def play(policies, sweep=two):
        pl = Player(make_plain(TT, 65 * len(sweep), 21), policies, games_num=24, poll_every=16, max_steps=2000, sweep=sweep, paired_diff=True)
        assert pl.policy is policies[0] and pl.policies == list(policies)
        return pl.run()
    ab, ba, aa = play([pA, pB]), play([pB, pA]), play([pA, pA])
    assert ab["groups"][0] == ba["groups"][1] and ab["groups"][1] == ba["groups"][0]
    assert aa["groups"][0] == aa["groups"][1]
    d_ab, d_ba = ab["paired_diff"]["cells"][1], ba["paired_diff"]["cells"][1]
    assert ab["paired_diff"]["complete"] and ba["paired_diff"]["complete"] and d_ab["pairs"] == d_ba["pairs"] == 65
    assert d_ab["diff"] == -d_ba["diff"] and d_ab["diff"] != 0.0 and d_ab["diff_stderr"] == d_ba["diff_stderr"] > 0.0
    assert d_ab["steps_diff"] == -d_ba["steps_diff"] and d_ab["cell_mean"] == d_ba["base_mean"] and d_ab["base_mean"] == d_ba["cell_mean"]
    for c in aa["paired_diff"]["cells"] + ab["paired_diff"]["cells"][:1]:
        assert c["diff"] == 0.0 and c["diff_stderr"] == 0.0 and c["steps_diff"] == 0
    four = play([pA] * 4, Sweep([{}] * 4, paired=True))                                      # one object, one act() over all rows
    assert all(g == four["groups"][0] for g in four["groups"]) and all(c["diff"] == 0.0 for c in four["paired_diff"]["cells"])
    mixed = play([pA, pB, pB, pA], Sweep([{}] * 4, paired=True))                             # pA serves two runs of cells: its buffer is copied out in between
    assert mixed["groups"][0] == mixed["groups"][3] == ab["groups"][0] and mixed["groups"][1] == mixed["groups"][2]
    diffs = [c["diff"] for c in mixed["paired_diff"]["cells"]]
    assert diffs[0] == diffs[3] == 0.0 and diffs[1] == diffs[2] != 0.0


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_against(torch_cuda, checkpoint, capsys, tmp_path):
    torch = torch_cuda
    from isaacgym_amd import play
    path, other = checkpoint(TT), str(tmp_path / "other.pth")
    torch.save(shifted_state_dict(torch, path), other)
    paired_file, cells_file = tmp_path / "diff.json", tmp_path / "cells.json"
    res = play.main(["--task", TT, "--checkpoint", path, "--num-envs", "128", "--games", "6", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--against", other, "--sweep", "friction_scale=0.5,1.0", "--paired-out", str(paired_file), "--sweep-out", str(cells_file)])
    lines = capsys.readouterr().out.splitlines()
    assert f"checkpoint 0: {path}" in lines and f"checkpoint 1: {other}" in lines
    written = json.loads(paired_file.read_text())
    assert written == res["paired_diff"] and written["complete"] and written["episodes"] == 1
    assert len(written["cells"]) == 4 and [c["baseline"] for c in written["cells"]] == [0, 1, 0, 1] and [c["cell"] for c in written["cells"]] == [0, 1, 2, 3]
    assert all(c["pairs"] == 32 for c in written["cells"])
    assert written["cells"][0]["diff"] == written["cells"][1]["diff"] == 0.0 and written["cells"][2]["diff"] != 0.0 and written["cells"][3]["diff"] != 0.0
    pair_lines = [l for l in lines if ": vs cell " in l]
    assert len(pair_lines) == 4 and pair_lines[2].startswith("cell 2 friction_scale=0.5: vs cell 0: pairs 32 diff ") and "(incomplete)" not in pair_lines[2]
    groups = json.loads(cells_file.read_text())                                              # --sweep-out as it always was: the result's `groups`
    assert groups == res["groups"] and [g["cell"] for g in groups] == [{"friction_scale": f} for f in (0.5, 1.0)] * 2 and all(g["paired"] is True for g in groups)
    assert len([l for l in lines if l.startswith("checkpoint 1 cell friction_scale=")]) == 2
