"""The control-latency delay line on the MI355X (include/ppenv_play_delay.h; isaacgym_amd.play: Delay, Player(action_delay=, obs_delay=), the
sweep axes action_delay / obs_delay).

The kernel against its host build (tests/csrc/play_delay_shim.cpp) bit for bit on the host tests' cases; a captured push replayed; Delay on
a strided view; then the Player under a paired latency sweep against the test's own host-synchronised loop, which keeps every observation
and every action it has seen and applies the header's rule with torch indexing: the applied actions and the observations handed to the
policy are bitwise equal at every step.  Then what zero delay and pairing promise, and that the lines compose with the other options.
The tasks run with env.episodeLength 12.  Need a real MI355X."""
import numpy as np
import pytest

import play_delay_shim_binding as pd
from test_play_gpu import checkpoint, load_policy, make_plain, torch_cuda        # noqa: F401  (two fixtures, two helpers)

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
GAMES = 3
STEPS = 30                                  # control steps of the hand-driven runs: every env (12-step episodes) restarts at least twice


def words(torch, x):
    """uint32 numpy [.., W] -> the float32 device tensor with those bits."""
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(DEV).view(torch.float32)


def same_bits(torch, a, b):
    """Two float32 tensors, compared as words (a NaN equals itself, 0.0 is not -0.0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------- the kernel against the shim
@pytest.mark.parametrize("shape", pd.SHAPES, ids=pd.shape_id)
def test_kernel_equals_the_shim_bit_for_bit(torch_cuda, shape):
    """Every host case; the row counts leave a partial last workgroup (pp::delay_rows_per_block rows each: 256, 146, 37, 12, 3)."""
    torch = torch_cuda
    from isaacgym_amd.play import Delay
    rows, A = shape
    for W, depth, pad in pd.subcases():
        d = pd.case_delays(rows, depth)
        xs, dones = pd.case_stream(rows, A, W, depth, pad)
        h = pd.HostDelay(rows, W, d, A)
        dl = Delay(rows, W, d, DEV, num_agents=A)
        dl.age.fill_(pd.GARBAGE)                                                            # reset() must clear it; the ring is never read unwritten
        dl.ring.view(torch.int32).fill_(pd.GARBAGE)
        dl.reset()
        x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
        keep = x_dev.clone()
        outs = [dl.push(x_dev[t][:, :W], done_dev[t]).clone() for t in range(len(xs))]       # pad: a view with a row stride of W + 3
        got = torch.stack(outs).view(torch.int32).cpu().numpy()
        for t in range(len(xs)):
            assert np.array_equal(got[t], h.push(xs[t], dones[t]).view(np.int32)), (rows, A, W, depth, pad, t)
        assert np.array_equal(dl.age.cpu().numpy(), h.age), (rows, A, W, depth, pad)
        assert torch.equal(x_dev.view(torch.int32), keep.view(torch.int32))                 # the input, its padding included, is not modified


def test_a_strided_output_keeps_its_padding(torch_cuda):
    """ld_out above the width through the plain C entry (Delay's own output is contiguous)."""
    torch = torch_cuda
    from isaacgym_amd import _lib
    L = _lib.lib()
    rows, A, W, depth = 130, 2, 27, 4
    d = pd.case_delays(rows, depth)
    xs, dones = pd.case_stream(rows, A, W, depth, 1)
    h = pd.HostDelay(rows, W, d, A, ld_out=W + 1)
    x_dev, done_dev, delay = words(torch, xs), torch.from_numpy(dones).to(DEV), torch.from_numpy(d).to(DEV)
    age = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ring = torch.zeros(L.pp_play_delay_ring_bytes(rows, W, depth) // 4, dtype=torch.float32, device=DEV)
    out = torch.full((rows, W + 1), pd.GARBAGE, dtype=torch.int32, device=DEV)
    _lib.check(L.pp_play_delay_reset(rows, age.data_ptr(), _lib.stream(age)), L)
    for t in range(len(xs)):
        _lib.check(L.pp_play_delay_push(x_dev[t].data_ptr(), W + 3, done_dev[t].data_ptr(), rows, A, W, depth, delay.data_ptr(), age.data_ptr(), ring.data_ptr(),
                                        out.data_ptr(), W + 1, _lib.stream(age)), L)
        h.push(xs[t], dones[t])
        assert np.array_equal(out.cpu().numpy(), h.out.view(np.int32)), t                     # the data and the untouched last column


def test_a_captured_push_replays_like_eager_pushes(torch_cuda):
    """No host-side counter: one captured push replayed 20 times (the input and done rewritten in place in between) equals 20 eager pushes."""
    torch = torch_cuda
    from isaacgym_amd.play import Delay
    rows, A, W, depth = 130, 2, 27, 4
    d = pd.case_delays(rows, depth)
    xs, dones = pd.case_stream(rows, A, W, 5, 0)                                             # 20 pushes
    assert len(xs) == 20
    x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
    eager, replayed = Delay(rows, W, d, DEV, num_agents=A), Delay(rows, W, d, DEV, num_agents=A)
    want = [eager.push(x_dev[t], done_dev[t]).clone() for t in range(20)]
    x, done = x_dev[0].clone(), done_dev[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        replayed.push(x, done)                                                              # warm-up outside the capture ...
        replayed.reset()                                                                    # ... undone
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.push(x, done)
    replayed.reset()                                                                        # the capture itself ran nothing
    for t in range(20):
        x.copy_(x_dev[t])
        done.copy_(done_dev[t])
        graph.replay()
        assert same_bits(torch, replayed.out, want[t]), t
    assert torch.equal(replayed.age, eager.age)


def test_delay_on_the_head_buffer_view(torch_cuda):
    """The network's head buffer is [rows, A + 1] (mu | value): its first A columns are a view with a row stride of A + 1."""
    torch = torch_cuda
    from isaacgym_amd.play import Delay
    rows, na, depth = 65, 7, 3
    d = pd.case_delays(rows, depth)
    xs, dones = pd.case_stream(rows, 1, na + 1, depth, 0)                                    # the value column rides along and is never moved
    x_dev, done_dev = words(torch, xs), torch.from_numpy(dones).to(DEV)
    dl, h = Delay(rows, na, d, DEV), pd.HostDelay(rows, na, d)
    for t in range(len(xs)):
        mu = x_dev[t][:, :na]
        assert mu.stride() == (na + 1, 1) and not mu.is_contiguous()
        out = dl.push(mu, None if t == 0 else done_dev[t])
        assert np.array_equal(out.view(torch.int32).cpu().numpy(), h.push(xs[t], None if t == 0 else dones[t]).view(np.int32)), t
    for bad in (torch.zeros((na, rows), device=DEV).t(), x_dev[0][:, :na].double(), x_dev[0][:-1, :na], x_dev[0][:, :na].cpu()):
        with pytest.raises(ValueError, match="Delay.push"):
            dl.push(bad)
    with pytest.raises(ValueError, match="Delay.push: done"):
        dl.push(x_dev[0][:, :na], done_dev[0].int())


# ------------------------------------------------------------------------------------------------------- the Player against a hand loop
def latency_sweep():
    from isaacgym_amd.play import Sweep
    return Sweep.grid({"action_delay": [0, 2], "obs_delay": [0, 1]}, paired=True)


def hand_loop(torch, task, policy, sweep, steps, games_num):
    """The latency sweep by hand, host-synchronised: the paired serve plan set as Player.start() sets it, then per control step the
    header's rule on Python lists of clone()d tensors — every observation and every action kept; per row the step its running episode
    began at; row r sees / is applied the entry of step start[r] + max(t - start[r] - d[r], 0) — and the accounting of rl_games' loop per
    cell, stopped per cell once games_num games are counted.  -> (observations handed to the policy, applied actions, raw actions: lists of
    [rows, .] tensors; per cell dict(games, steps, returns per agent); per env its number of resets)."""
    A, N, G = task.num_agents, task.num_envs, len(sweep)
    rows, w = A * N, A * N // G
    d = {k: torch.from_numpy(v).to(DEV).long() for k, v in sweep.delays(N, A).items()}
    task.set_serve_plan(sweep.serve_cells(task.env.serve_defaults()), paired=sweep.paired)
    task.reset_idx()
    policy._counter = 0
    obs = task.reset()["obs"]
    every = torch.arange(rows, device=DEV)
    start = torch.zeros(rows, dtype=torch.long, device=DEV)
    kept_obs, kept_act, seen, applied, raw = [], [], [], [], []
    cr = torch.zeros(rows, dtype=torch.float32, device=DEV)
    length = torch.zeros(rows, dtype=torch.int64, device=DEV)
    cells = [dict(games=0, steps=0, returns=[[] for _ in range(A)]) for _ in range(G)]
    resets = np.zeros(N, np.int64)
    done_prev = None
    for t in range(steps):
        if done_prev is not None:
            first = (done_prev.view(N, A)[:, :1] != 0).expand(N, A).reshape(rows)            # agent 0's word, for every row of the env
            start = torch.where(first, torch.full_like(start, t), start)
        kept_obs.append(obs.clone())
        src = start + torch.clamp(t - start - d["obs_delay"], min=0)
        obs_seen = torch.stack(kept_obs)[src, every].clone()
        a, _ = policy.act(obs_seen, deterministic=True, seed=0)
        kept_act.append(a.clone())
        src = start + torch.clamp(t - start - d["action_delay"], min=0)
        a_applied = torch.stack(kept_act)[src, every].clone()
        seen.append(obs_seen)
        raw.append(a.clone())
        applied.append(a_applied.clone())
        od, r, done, _ = task.step(a_applied)
        obs, done_prev = od["obs"], done.clone()
        cr += r
        length += 1
        fin = done.view(N, A)[:, 0].nonzero(as_tuple=False).flatten().cpu().numpy()         # the host read of every step
        resets[fin] += 1
        for g, cell in enumerate(cells):
            mine = fin[(fin >= g * N // G) & (fin < (g + 1) * N // G)]
            if cell["games"] >= games_num or len(mine) == 0:
                continue                                                                   # the freeze, or nothing finished
            cell["games"] += len(mine)
            cell["steps"] += int(length[torch.from_numpy(A * mine).to(DEV)].sum())
            for k in range(A):
                cell["returns"][k] += [float(x) for x in cr[torch.from_numpy(A * mine + k).to(DEV)].cpu().numpy()]
        all_done = done.nonzero(as_tuple=False).flatten()
        cr[all_done] = 0.0
        length[all_done] = 0
    task.clear_serve_plan()
    return seen, applied, raw, cells, resets


@pytest.mark.parametrize("name,n", [(TT, 64), (TA, 64), (T4, 32)], ids=["7dof", "27dof", "4actor"])
def test_player_under_a_latency_sweep_matches_the_hand_loop(torch_cuda, checkpoint, name, n):
    torch = torch_cuda
    from isaacgym_amd.play import Player, group_summary
    path = checkpoint(TT if name == T4 else name)
    sweep = latency_sweep()
    assert [(c["action_delay"], c["obs_delay"]) for c in sweep.cells] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    pl = Player(make_plain(name, n, 21), load_policy(path), games_num=GAMES, poll_every=8, max_steps=2000, sweep=sweep)
    assert pl._act_line.depth == 3 and pl._obs_line.depth == 2 and pl._act_line.width == pl.task.num_actions and pl._obs_line.width == pl.task.num_obs
    got_seen, got_applied, got_raw = [], [], []
    pl.start()
    for _ in range(STEPS):
        pl.step()
        got_seen.append(pl.policy_obs.clone())
        got_applied.append(pl.applied_actions.clone())
        got_raw.append(pl.actions.clone())
    per = pl.stats.read_groups()
    lat = pl.latency()
    pl.end_sweep()
    seen, applied, raw, cells, resets = hand_loop(torch, make_plain(name, n, 21), load_policy(path), sweep, STEPS, GAMES)
    assert resets.min() >= 2, resets
    A, w = pl.num_agents, pl.num_agents * n // 4
    for t in range(STEPS):
        for g in range(4):
            rows = slice(g * w, (g + 1) * w)
            assert same_bits(torch, got_seen[t][rows], seen[t][rows]), (name, "policy_obs", t, g)
            assert same_bits(torch, got_raw[t][rows], raw[t][rows]), (name, "actions", t, g)
            assert same_bits(torch, got_applied[t][rows], applied[t][rows]), (name, "applied_actions", t, g)
        assert same_bits(torch, got_applied[t][:2 * w], got_raw[t][:2 * w])                  # cells 0 and 1: no action delay
    assert any(not same_bits(torch, got_applied[t][2 * w:], got_raw[t][2 * w:]) for t in range(STEPS))       # cells 2 and 3: a delayed command
    assert any(not same_bits(torch, got_applied[t][:w], got_applied[t][2 * w:3 * w]) for t in range(STEPS))  # cells 0 and 2 differ
    for g, (cell, tot) in enumerate(zip(cells, per)):                                        # the cell summaries
        s = group_summary(sweep.cells[g], tot, A, GAMES, paired=True)
        assert s["cell"] == sweep.cells[g] and all(type(v) is int for v in s["cell"].values())
        assert s["games"] == cell["games"] >= GAMES and s["complete"] and s["av_steps"] == cell["steps"] / cell["games"], (name, g)
        for k in range(A):
            x = np.asarray(cell["returns"][k], np.float64)
            p = s["per_agent"][k]
            assert (p["reward_min"], p["reward_max"]) == (x.min(), x.max()), (name, g, k)
            assert abs(p["av_reward"] - x.mean()) <= 2.0 ** -50 * np.abs(x).sum() / len(x), (name, g, k)     # fp64 sums of the same fp32 returns, in two orders
            # E[x^2] - E[x]^2 in fp64 on both sides: each sum of n <= 32 terms is within n x 2^-53 of exact, the square doubles that
            assert abs(p["reward_std"] ** 2 - (np.mean(x * x) - x.mean() ** 2)) <= 2.0 ** -46 * np.mean(x * x), (name, g, k)
    assert lat == dict(control_dt=pl.task.env.control_dt, action_delay=[0, 0, 2, 2], obs_delay=[0, 1, 0, 1])


# ------------------------------------------------------------------------------------------------------- zero delay, replicas
def without_clock(res):
    return {k: v for k, v in res.items() if k != "seconds"}


def test_the_zero_delay_cell_is_the_sweep_without_the_axes(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    path = checkpoint(TT)
    kw = dict(games_num=GAMES, poll_every=8, max_steps=2000)
    pl = Player(make_plain(TT, 64, 21), load_policy(path), sweep=latency_sweep(), **kw)
    plain = Player(make_plain(TT, 64, 21), load_policy(path), sweep=Sweep([{}] * 4, paired=True), **kw)
    assert plain._act_line is None and plain._obs_line is None
    res, res0 = pl.run(), plain.run()
    assert "latency" not in res0 and res["latency"]["action_delay"] == [0, 0, 2, 2]
    assert pl.stats.group_state_bytes(0) == plain.stats.group_state_bytes(0)
    assert {k: v for k, v in res["groups"][0].items() if k != "cell"} == {k: v for k, v in res0["groups"][0].items() if k != "cell"}
    assert res["groups"][0]["cell"] == {"action_delay": 0, "obs_delay": 0} and res0["groups"][0]["cell"] == {}
    assert pl.stats.group_state_bytes(2) != plain.stats.group_state_bytes(2)


def test_zero_keywords_build_no_line_and_change_nothing(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player
    path = checkpoint(TT)
    kw = dict(games_num=40, poll_every=16, max_steps=2000)
    zero = Player(make_plain(TT, 64, 21), load_policy(path), action_delay=0, obs_delay=0, **kw)
    plain = Player(make_plain(TT, 64, 21), load_policy(path), **kw)
    assert zero._act_line is None and zero._obs_line is None
    a, b = zero.run(), plain.run()
    assert "latency" not in a and without_clock(a) == without_clock(b) and zero.stats.state_bytes() == plain.stats.state_bytes()
    assert zero.applied_actions is zero.actions


def test_equal_latency_cells_are_bitwise_replicas(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Player, Sweep
    pl = Player(make_plain(TT, 64, 21), load_policy(checkpoint(TT)), games_num=GAMES, sweep=Sweep([{"action_delay": 2}] * 2, paired=True))
    assert pl._obs_line is None and pl._act_line.depth == 3
    pl.start()
    for t in range(STEPS):
        pl.step()
        for x in (pl.applied_actions, pl.actions, pl.policy_obs):
            assert same_bits(torch, x[:32], x[32:]), t
    assert pl.stats.group_state_bytes(0) == pl.stats.group_state_bytes(1)
    pl.end_sweep()


def test_the_lines_compose_with_the_other_options(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    path = checkpoint(TT)
    sweep = Sweep([{"action_delay": 0}, {"action_delay": 2, "obs_delay": 1}], paired=True)
    pl = Player(make_plain(TT, 64, 21), [load_policy(path), load_policy(path)], games_num=GAMES, poll_every=8, max_steps=2000, sweep=sweep, paired_diff=True,
                actuators=True)
    res = pl.run()
    assert len(res["groups"]) == 2 and all(g["complete"] for g in res["groups"])
    assert res["paired_diff"]["complete"] and len(res["paired_diff"]["cells"]) == 2 and res["paired_diff"]["cells"][0]["diff"] == 0.0
    assert len(res["actuators"]["groups"]) == 2 and len(res["actuators"]["groups"][1]["per_joint"]) == 7
    assert res["latency"] == dict(control_dt=pl.task.env.control_dt, action_delay=[0, 2], obs_delay=[0, 1])
    assert tuple(pl.actions.shape) == tuple(pl.applied_actions.shape) == (64, 7) and tuple(pl.policy_obs.shape) == (64, pl.task.num_obs)


def test_the_keyword_without_a_sweep_is_the_one_cell_sweep(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player, Sweep
    path = checkpoint(TT)
    kw = dict(games_num=40, poll_every=16, max_steps=2000)
    a = Player(make_plain(TT, 64, 21), load_policy(path), action_delay=1, **kw)
    b = Player(make_plain(TT, 64, 21), load_policy(path), sweep=Sweep([{"action_delay": 1}]), **kw)
    plain = Player(make_plain(TT, 64, 21), load_policy(path), **kw)
    ra, rb, rp = a.run(), b.run(), plain.run()
    assert a._obs_line is None and a._act_line.depth == 2 and ra["latency"] == dict(control_dt=a.task.env.control_dt, action_delay=[1], obs_delay=[0])
    assert without_clock(ra) == {k: v for k, v in without_clock(rb).items() if k != "groups"}
    assert a.stats.state_bytes() == b.stats.state_bytes()
    assert {k: rb["groups"][0][k] for k in ("games", "av_reward", "av_steps")} == {k: ra[k] for k in ("games", "av_reward", "av_steps")}
    assert a.stats.state_bytes() != plain.stats.state_bytes()                                # one step of command latency is not nothing


def test_cli_latency_sweep(torch_cuda, checkpoint, capsys, tmp_path):
    import json
    from isaacgym_amd import play
    cells_file, diff_file = tmp_path / "cells.json", tmp_path / "diff.json"
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "128", "--games", "10", "--poll-every", "16", "--seed", "3", "--max-steps", "1500",
                     "--sweep", "action_delay=0,1,2,3", "--paired", "--paired-diff", "--baseline", "0", "--obs-delay", "1", "--sweep-out", str(cells_file),
                     "--paired-out", str(diff_file)])
    lines = capsys.readouterr().out.splitlines()
    ms = 1000.0 * res["latency"]["control_dt"]
    head = [l for l in lines if l.startswith("latency: ")]
    assert head == [f"latency: control dt {ms:.6g} ms; action_delay 0,1,2,3 steps = 0,{ms:.6g},{2 * ms:.6g},{3 * ms:.6g} ms; "
                    f"obs_delay 1,1,1,1 steps = {ms:.6g},{ms:.6g},{ms:.6g},{ms:.6g} ms"]
    cells = [l for l in lines if l.startswith("cell action_delay=")]
    assert [c.split(":")[0] for c in cells] == [f"cell action_delay={k}" for k in range(4)]
    diffs = [l for l in lines if l.startswith("cell ") and ": vs cell 0: pairs " in l]
    assert [d.split(":")[0] for d in diffs] == [f"cell {k} action_delay={k}" for k in range(4)] and " diff 0 +- 0 " in diffs[0]
    assert res["latency"] == dict(control_dt=res["latency"]["control_dt"], action_delay=[0, 1, 2, 3], obs_delay=[1] * 4)
    assert [w["cell"] for w in json.loads(cells_file.read_text())] == [{"action_delay": k} for k in range(4)]
    written = json.loads(diff_file.read_text())
    assert [c["cell"] for c in written["cells"]] == [0, 1, 2, 3] and written["cells"][0]["diff"] == 0.0 and written["latency"] == res["latency"]
