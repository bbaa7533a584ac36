"""Episode accounting for playing a checkpoint (include/ppenv_play.h) without a GPU: the kernels' per-env arithmetic
(isaacgym_amd/csrc/ppenv_play_device.h, compiled for the host by tests/play_shim_binding.py) against rl_games' player loop restated in
numpy below, and the host-side plumbing of isaacgym_amd.play (argument checks, the result arithmetic, the CLI's parser).

Bounds.  Integers, cur_reward (one fp32 addition per row and step) and the minima / maxima are compared for equality.  A fp64 sum of
`count` terms, in any order, is within count x 2^-53 x sum|x| of the exact sum (math.fsum here); with integer-valued rewards every
return, square and partial sum is an integer below 2^53 and the sums are compared for equality."""
import math
import types

import numpy as np
import pytest

import play_shim_binding as ps

STEPS = 60
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 257), (2, 1), (2, 33), (2, 129)]      # (num_agents, num_envs)
NEVER = 1 << 40                                                                         # a games_num no sequence reaches


def rlgames_loop(rews, dones, num_agents, n_games):
    """rl_games' BasePlayer.run on recorded [steps, rows] rewards and done words: float32 `cr += r`, `steps += 1`, `done.nonzero()` every
    step, `all_done_indices[::num_agents]`, the finished rows' values into the sums, their running values to zero, and a break after the
    step in which games_played >= n_games.  Two restatement choices: a done word counts when it is non-zero (rl_games' `done.float()`
    assumes 0 / 1), and the running values are zeroed by assignment (rl_games multiplies by 1 - done, which leaves -0 behind a negative
    return: the same value).  -> dict(games, steps, launches, returns [num_agents lists], cr, cur_steps, broke_at)."""
    rows = rews.shape[1]
    cr = np.zeros(rows, np.float32)
    steps = np.zeros(rows, np.int64)
    games = sum_steps = launches = 0
    returns = [[] for _ in range(num_agents)]
    broke_at = None
    for t in range(rews.shape[0]):
        cr = (cr + rews[t]).astype(np.float32)
        steps += 1
        launches += 1
        all_done = np.nonzero(dones[t])[0]
        done_idx = all_done[::num_agents]
        games += len(done_idx)
        if len(done_idx) > 0:
            sum_steps += int(steps[done_idx].sum())
            for a in range(num_agents):
                returns[a] += [float(x) for x in cr[done_idx + a]]
            cr[all_done] = 0.0
            steps[all_done] = 0
            if games >= n_games:
                broke_at = t
                break
    return dict(games=games, steps=sum_steps, launches=launches, returns=returns, cr=cr, cur_steps=steps[::num_agents].astype(np.int32),
                broke_at=broke_at)


def check_against_loop(got, state, ref, num_agents, exact=False, what=""):
    """got: a totals dict, state: (cur_reward bytes, cur_steps bytes, ...) — against rlgames_loop's result."""
    assert (got["games"], got["steps"], got["launches"]) == (ref["games"], ref["steps"], ref["launches"]), what
    assert state[0] == ref["cr"].tobytes(), f"{what}: cur_reward"
    assert state[1] == ref["cur_steps"].tobytes(), f"{what}: cur_steps"
    for a in range(num_agents):
        x = np.asarray(ref["returns"][a], np.float64)
        for key, terms in (("reward", x), ("reward_sq", x * x)):              # the square of a float is exact in fp64
            want = math.fsum(terms)
            bound = 0.0 if exact else len(terms) * 2.0 ** -53 * float(np.abs(terms).sum())
            assert abs(got[key][a] - want) <= bound, f"{what}: {key}[{a}] {got[key][a]!r} vs {want!r}, bound {bound:.3g}"
        assert got["reward_min"][a] == (x.min() if x.size else np.inf) and got["reward_max"][a] == (x.max() if x.size else -np.inf), what


def run_shim(rews, dones, num_agents, games_num):
    h = ps.HostStats(rews.shape[1] // num_agents, num_agents, games_num)
    for t in range(rews.shape[0]):
        h.accumulate(rews[t], dones[t])
    return h


PATTERNS = {"scripted": dict(p=0.08, seed=5), "dense": dict(p=0.5, seed=11), "sparse": dict(p=0.01, seed=12)}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("num_agents,num_envs", SHAPES)
def test_shim_matches_rlgames_loop(num_agents, num_envs, pattern):
    rows = num_agents * num_envs
    dones = ps.scripted_dones(STEPS, num_envs, num_agents, **PATTERNS[pattern])
    rews = ps.rewards(STEPS, rows, seed=6 + num_envs)
    h = ps.HostStats(num_envs, num_agents, NEVER)
    for t in range(STEPS):
        h.accumulate(rews[t], dones[t])
        if t in (0, 9, 13, STEPS - 1):                       # before, inside and after the burst
            ref = rlgames_loop(rews[:t + 1], dones[:t + 1], num_agents, NEVER)
            check_against_loop(h.read(), h.state_bytes(), ref, num_agents, what=f"step {t}")
    assert h.read()["games"] > 0


@pytest.mark.parametrize("num_agents,num_envs", SHAPES)
def test_integer_rewards_sum_exactly(num_agents, num_envs):
    rows = num_agents * num_envs
    dones = ps.scripted_dones(STEPS, num_envs, num_agents)
    rews = ps.rewards(STEPS, rows, integer=True)
    assert rews.min() >= -3000 and rews.max() <= 3000 and np.array_equal(rews, np.round(rews))
    h = run_shim(rews, dones, num_agents, NEVER)
    check_against_loop(h.read(), h.state_bytes(), rlgames_loop(rews, dones, num_agents, NEVER), num_agents, exact=True)


@pytest.mark.parametrize("num_agents,num_envs", [(1, 65), (2, 33)])
def test_every_nonzero_done_word_is_done(num_agents, num_envs):
    rows = num_agents * num_envs
    rews = ps.rewards(STEPS, rows)
    plain = ps.scripted_dones(STEPS, num_envs, num_agents, words=(1,))
    mixed = ps.scripted_dones(STEPS, num_envs, num_agents, words=(1, 2, 1 << 32))
    assert set(np.unique(mixed)) == {0, 1, 2, 1 << 32} and np.array_equal(mixed != 0, plain != 0)
    a, b = run_shim(rews, plain, num_agents, NEVER), run_shim(rews, mixed, num_agents, NEVER)
    assert a.state_bytes() == b.state_bytes()
    check_against_loop(b.read(), b.state_bytes(), rlgames_loop(rews, mixed, num_agents, NEVER), num_agents)


@pytest.mark.parametrize("num_agents,num_envs", [(1, 1), (1, 65), (1, 257), (2, 33)])
def test_freeze_counts_the_crossing_step_and_then_changes_nothing(num_agents, num_envs):
    rows = num_agents * num_envs
    dones = ps.scripted_dones(STEPS, num_envs, num_agents)
    rews = ps.rewards(STEPS, rows)
    available = rlgames_loop(rews, dones, num_agents, NEVER)["games"]
    games_num = max(available // 2, 1)
    ref = rlgames_loop(rews, dones, num_agents, games_num)
    t_cross = ref["broke_at"]
    assert t_cross is not None and t_cross < STEPS - 10, "the crossing must happen mid-sequence"
    if num_envs > 1:                                              # the crossing step finishes several envs: all of them are counted
        assert ref["games"] >= games_num and int((dones[t_cross, ::num_agents] != 0).sum()) >= 1
    h = ps.HostStats(num_envs, num_agents, games_num)
    frozen = None
    for t in range(STEPS):
        h.accumulate(rews[t], dones[t])
        if t == t_cross:
            frozen = h.state_bytes()
            check_against_loop(h.read(), frozen, ref, num_agents, what="at the crossing")
            assert games_num <= h.read()["games"] <= games_num + num_envs - 1
        elif t > t_cross:
            assert h.state_bytes() == frozen, f"call {t - t_cross} after the freeze changed the state"
    assert h.read()["launches"] == t_cross + 1


def test_freeze_edges_one_game_and_more_games_than_there_are():
    num_agents, num_envs = 1, 65
    dones = ps.scripted_dones(STEPS, num_envs, num_agents)
    rews = ps.rewards(STEPS, num_envs)
    ref1 = rlgames_loop(rews, dones, num_agents, 1)
    h = run_shim(rews, dones, num_agents, 1)
    check_against_loop(h.read(), h.state_bytes(), ref1, num_agents, what="games_num = 1")
    assert ref1["launches"] == ref1["broke_at"] + 1 < STEPS
    total = rlgames_loop(rews, dones, num_agents, NEVER)
    h = run_shim(rews, dones, num_agents, total["games"] + 1)     # one more than the sequence holds: never frozen
    got = h.read()
    assert got["launches"] == STEPS and got["games"] == total["games"]
    check_against_loop(got, h.state_bytes(), total, num_agents, what="games_num above the games available")


def test_reset_clears_the_state():
    h = ps.HostStats(65, 2, 5)
    got = h.read()
    assert (got["games"], got["steps"], got["launches"]) == (0, 0, 0) and got["reward"] == [0.0, 0.0] and got["reward_sq"] == [0.0, 0.0]
    assert got["reward_min"] == [np.inf, np.inf] and got["reward_max"] == [-np.inf, -np.inf]
    assert not h.cur_reward.any() and not h.cur_steps.any()


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _fake(rl="cuda:0", sim="cuda:0", pol="cuda:0", obs=80, act=7, pobs=80, pact=7):
    import torch
    task = types.SimpleNamespace(rl_device=torch.device(rl), device=torch.device(sim), num_obs=obs, num_actions=act, num_envs=4, num_agents=1)
    policy = types.SimpleNamespace(device=torch.device(pol), net=types.SimpleNamespace(num_obs=pobs, num_actions=pact))
    return task, policy


def test_player_argument_checks():
    from isaacgym_amd.play import EpisodeStats, Player
    for kw in (dict(games_num=0), dict(poll_every=0), dict(max_steps=0), dict(games_num=2.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            Player(*_fake(), **kw)
    with pytest.raises(ValueError, match=r"rl_device is cpu.*sim_device is cuda:0"):
        Player(*_fake(rl="cpu"))
    with pytest.raises(ValueError, match=r"rl_device is cpu.*sim_device is cpu"):
        Player(*_fake(rl="cpu", sim="cpu"))
    with pytest.raises(ValueError, match=r"rl_device is cuda:1.*sim_device is cuda:0"):
        Player(*_fake(rl="cuda:1"))
    with pytest.raises(ValueError, match="policy lives on"):
        Player(*_fake(pol="cuda:1"))
    with pytest.raises(ValueError, match="313 observations to 27 actions"):
        Player(*_fake(pobs=313, pact=27))
    for args in ((0, 1, 5), (4, 3, 5), (4, 1, 0)):
        with pytest.raises(ValueError, match="EpisodeStats"):
            EpisodeStats(*args, "cuda:0")


def test_result_arithmetic():
    from isaacgym_amd.play import summarize
    x0, x1 = np.array([3.0, -1.0, 10.0, 4.0]), np.array([1.0, 1.0, 1.0, 1.0])
    tot = dict(games=4, steps=50, launches=20, reward=[x0.sum(), x1.sum()], reward_sq=[(x0 * x0).sum(), (x1 * x1).sum()],
               reward_min=[-1.0, 1.0], reward_max=[10.0, 1.0])
    r = summarize(tot, 2)
    assert r["games"] == 4 and r["av_steps"] == 12.5 and r["av_reward"] == 4.0 and r["reward_min"] == -1.0 and r["reward_max"] == 10.0
    assert r["reward_std"] == pytest.approx(x0.std(), rel=1e-15)
    assert len(r["per_agent"]) == 2 and r["per_agent"][0]["av_reward"] == r["av_reward"]             # av_reward is agent 0's
    assert r["per_agent"][1] == dict(av_reward=1.0, reward_std=0.0, reward_min=1.0, reward_max=1.0)
    assert len(summarize(tot, 1)["per_agent"]) == 1
    # E[x^2] - E[x]^2 rounds below zero for equal returns: clamped at 0, not a nan
    v = 0.1
    neg = dict(tot, games=3, reward=[3 * v], reward_sq=[math.nextafter(3 * v * v, 0.0)], reward_min=[v], reward_max=[v])
    assert neg["reward_sq"][0] / 3 - (neg["reward"][0] / 3) ** 2 < 0
    assert summarize(neg, 1)["reward_std"] == 0.0
    empty = summarize(dict(games=0, steps=0, launches=9, reward=[0.0], reward_sq=[0.0], reward_min=[np.inf], reward_max=[-np.inf]), 1)
    assert empty["games"] == 0 and math.isnan(empty["av_reward"]) and math.isnan(empty["av_steps"])


def test_cli_parsing():
    from isaacgym_amd.play import parse_args
    a = parse_args(["--checkpoint", "x.pth"])
    assert (a.task, a.num_envs, a.games, a.stochastic, a.sigma, a.seed, a.cfg_dir, a.poll_every) == \
        ("HumanoidPingpongTiltNESSparse27DOFG1", 4096, 2000, False, None, 42, None, 64)
    a = parse_args(["--task", "HumanoidPingpongTiltG1", "--checkpoint", "runs/tt/nn/HumanoidPingpongTiltG1.pth", "--num-envs", "130", "--games", "200",
                    "--stochastic", "--sigma", "-6.0", "--seed", "3", "--cfg-dir", "cfg", "--poll-every", "7"])
    assert (a.task, a.checkpoint, a.num_envs, a.games, a.stochastic, a.sigma, a.seed, a.cfg_dir, a.poll_every) == \
        ("HumanoidPingpongTiltG1", "runs/tt/nn/HumanoidPingpongTiltG1.pth", 130, 200, True, -6.0, 3, "cfg", 7)
    with pytest.raises(SystemExit):
        parse_args(["--task", "HumanoidPingpongTiltG1"])                                             # no checkpoint


def test_totals_struct_layout():
    import ctypes as C
    from isaacgym_amd.play import PlayTotals
    assert C.sizeof(PlayTotals) == 72
    assert (PlayTotals.launches.offset, PlayTotals.reward.offset, PlayTotals.reward_sq.offset, PlayTotals.reward_min.offset,
            PlayTotals.reward_max.offset) == (16, 24, 40, 56, 64)
    ps.lib()                                                                                         # asserts the compiled sizes
