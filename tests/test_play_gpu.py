"""Playing a checkpoint on the MI355X (isaacgym_amd.play, include/ppenv_play.h): the accounting kernels against their host build and
rl_games' loop on recorded sequences, the freeze, and the Player against the test's own host-synchronised rl_games-style loop (`.nonzero()`
every step) on a second task built with the same seed — plain, under reset-time randomisation, on the 27-dof and the 4-actor task,
with different polling intervals, stochastic, and through the CLI.  Bounds: tests/test_play_host.py's (integers, cur_reward and the
extrema equal; a fp64 sum of `count` games within count x 2^-53 x sum|x| of the exact sum; integer rewards: equal); on float rewards the
sum order itself is held by the recorded digests of tests/golden/play_state_digests.json.  The tasks run with env.episodeLength 12, so
games finish within tens of steps.  Need a real MI355X."""
import importlib.util
import json
import os

import numpy as np
import pytest

import play_shim_binding as ps
from test_play_host import NEVER, SHAPES, STEPS, check_against_loop, rlgames_loop, run_shim

pytestmark = pytest.mark.gpu

TT, TA, T4 = "HumanoidPingpongTiltG1", "HumanoidPingpongTiltNESSparse27DOFG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ------------------------------------------------------------------------------------------------------- the kernels
def device_sequence(torch, rews, dones):
    """The recorded [steps, rows] sequences inside larger device buffers, one row down: every step's slice starts at a non-zero offset
    (and, for an odd row count, at an address that is no multiple of 8 / 16 bytes)."""
    r = torch.zeros((rews.shape[0] + 2, rews.shape[1]), dtype=torch.float32, device=DEV)
    d = torch.ones((dones.shape[0] + 2, dones.shape[1]), dtype=torch.int64, device=DEV)
    r[1:-1], d[1:-1] = torch.from_numpy(rews).to(DEV), torch.from_numpy(dones).to(DEV)
    return r[1:-1], d[1:-1]


def run_device(torch, stats, r, d, steps=None):
    for t in range(r.shape[0] if steps is None else steps):
        stats.accumulate(r[t % r.shape[0]], d[t % r.shape[0]])
    torch.cuda.synchronize()


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("num_agents,num_envs", SHAPES + [(1, 1000), (2, 1000)])
def test_kernel_matches_shim_and_loop(torch_cuda, num_agents, num_envs, integer):
    torch = torch_cuda
    from isaacgym_amd.play import EpisodeStats
    rows = num_agents * num_envs
    dones = ps.scripted_dones(STEPS, num_envs, num_agents, words=(1, 2, 1 << 32))
    rews = ps.rewards(STEPS, rows, seed=6 + num_envs, integer=integer)
    r, d = device_sequence(torch, rews, dones)
    st = EpisodeStats(num_envs, num_agents, NEVER, DEV)
    run_device(torch, st, r, d)
    first = st.state_bytes()
    shim = run_shim(rews, dones, num_agents, NEVER)
    got, want = st.read(), shim.read()
    assert first[0] == shim.state_bytes()[0] and first[1] == shim.state_bytes()[1]           # cur_reward, cur_steps: the same bits
    for k in ("games", "steps", "launches", "reward_min", "reward_max"):
        assert got[k] == want[k], k
    assert got["launches"] == STEPS and got["games"] > 0
    check_against_loop(got, first, rlgames_loop(rews, dones, num_agents, NEVER), num_agents, exact=integer, what="kernel vs loop")
    if integer:
        assert first[2] == shim.state_bytes()[2]                                             # the whole struct
    st.reset()                                                                               # ... and again from reset(): bitwise the same
    run_device(torch, st, r, d)
    assert st.state_bytes() == first
    tot = st.totals()                                                                        # the device views name the same words
    assert int(tot["games"]) == got["games"] and float(tot["per_agent"][num_agents - 1]["reward_sq"]) == got["reward_sq"][num_agents - 1]
    assert float(tot["reward_max"]) == got["reward_max"][0] and int(tot["launches"]) == STEPS


@pytest.mark.parametrize("num_agents,num_envs", [(1, 1), (1, 257), (2, 129), (1, 1000)])
def test_kernel_freeze(torch_cuda, num_agents, num_envs):
    torch = torch_cuda
    from isaacgym_amd.play import EpisodeStats
    rows = num_agents * num_envs
    dones = ps.scripted_dones(STEPS, num_envs, num_agents)
    rews = ps.rewards(STEPS, rows)
    games_num = max(rlgames_loop(rews, dones, num_agents, NEVER)["games"] // 2, 1)
    ref = rlgames_loop(rews, dones, num_agents, games_num)
    t_cross = ref["broke_at"]
    assert t_cross is not None and t_cross < STEPS - 10
    r, d = device_sequence(torch, rews, dones)
    st = EpisodeStats(num_envs, num_agents, games_num, DEV)
    run_device(torch, st, r, d, steps=t_cross + 1)
    frozen = st.state_bytes()
    got = st.read()
    check_against_loop(got, frozen, ref, num_agents, what="at the crossing")
    assert games_num <= got["games"] <= games_num + num_envs - 1
    for t in range(t_cross + 1, t_cross + 41):                                               # 40 further launches
        st.accumulate(r[t % STEPS], d[t % STEPS])
    torch.cuda.synchronize()
    assert st.state_bytes() == frozen
    assert st.read()["launches"] == t_cross + 1


def test_accumulate_refuses_wrong_tensors(torch_cuda):
    torch = torch_cuda
    from isaacgym_amd.play import EpisodeStats
    st = EpisodeStats(8, 2, 5, DEV)
    r, d = torch.zeros(16, device=DEV), torch.zeros(16, dtype=torch.int64, device=DEV)
    st.accumulate(r, d)
    for bad_r, bad_d in ((r[:8], d), (r, d.int()), (r.double(), d), (torch.zeros(32, device=DEV)[::2], d), (r.cpu(), d)):
        with pytest.raises(ValueError, match="accumulate"):
            st.accumulate(bad_r, bad_d)


# ------------------------------------------------------------------------------------------------------- the recorded bits
_TESTS = os.path.dirname(os.path.abspath(__file__))
DIRECT = [(1, 65), (2, 129), (1, 257)]                   # shapes at which the plain C entries are driven as well


@pytest.fixture(scope="module")
def digests():
    """(tools/play_state_digests.py as a module, the recorded cases of tests/golden/play_state_digests.json, its cases() by key)."""
    spec = importlib.util.spec_from_file_location("play_state_digests", os.path.join(_TESTS, "..", "tools", "play_state_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(_TESTS, "golden", "play_state_digests.json")) as fh:
        recorded = json.load(fh)
    cases = {key: (num_agents, num_envs, games_num, rews, dones) for key, num_agents, num_envs, games_num, rews, dones in tool.cases()}
    assert recorded["steps"] == STEPS and set(recorded["cases"]) == set(cases) and len(cases) == 2 * (len(SHAPES) + 2)
    return tool, recorded["cases"], cases


class PlainEntries:
    """ppenv_play_reset / ppenv_play_accumulate on the test's own tensors, with accumulate() and state_bytes() as EpisodeStats has them."""

    def __init__(self, torch, num_envs, num_agents, games_num):
        from isaacgym_amd import _lib
        self.check, self.L, self.stream = _lib.check, _lib.lib(), _lib.stream(torch.device(DEV))
        self.sizes, self.games_num = (num_envs, num_agents), games_num
        self.cur_reward = torch.full((num_envs * num_agents,), 7.0, dtype=torch.float32, device=DEV)      # garbage: the reset must clear it
        self.cur_steps = torch.full((num_envs,), 7, dtype=torch.int32, device=DEV)
        self.totals = torch.full((72,), 0x55, dtype=torch.uint8, device=DEV)
        self.partial = torch.zeros(self.L.ppenv_play_partial_bytes(num_envs), dtype=torch.uint8, device=DEV)
        self.check(self.L.ppenv_play_reset(*self.sizes, self.cur_reward.data_ptr(), self.cur_steps.data_ptr(), self.totals.data_ptr(), self.stream), self.L)

    def accumulate(self, rew, done):
        assert rew.is_contiguous() and done.is_contiguous() and rew.numel() == done.numel() == self.cur_reward.numel()
        self.check(self.L.ppenv_play_accumulate(rew.data_ptr(), done.data_ptr(), *self.sizes, self.games_num, self.cur_reward.data_ptr(),
                                                self.cur_steps.data_ptr(), self.totals.data_ptr(), self.partial.data_ptr(), self.stream), self.L)

    def state_bytes(self):
        return tuple(t.cpu().numpy().tobytes() for t in (self.cur_reward, self.cur_steps, self.totals))


@pytest.mark.parametrize("num_agents,num_envs", SHAPES + [(1, 1000), (2, 1000)])
def test_state_digests_are_the_recorded_ones(torch_cuda, digests, num_agents, num_envs):
    """Float rewards, never frozen and frozen half-way: sha256 of cur_reward, cur_steps and the totals after STEPS steps equal the digests
    recorded on an MI355X from the commit that still had a kernel family of its own for the single accounting.  EpisodeStats (the grouped
    entries with one group) and, at DIRECT, the plain C entries.  A digest that differs means the fp64 sum order moved: the file stays."""
    torch = torch_cuda
    from isaacgym_amd.play import EpisodeStats
    tool, recorded, cases = digests
    for name in ("never", "freeze"):
        key = f"{num_agents}x{num_envs}_{name}"
        A, N, games_num, rews, dones = cases[key]
        assert (A, N, games_num) == (num_agents, num_envs, recorded[key]["games_num"]), key
        want = {part: recorded[key][part] for part in tool.PARTS}
        st = EpisodeStats(num_envs, num_agents, games_num, DEV)
        assert tool.play(torch, st, rews, dones) == want, f"{key}: EpisodeStats"
        assert (st.read()["launches"] < STEPS) == (name == "freeze"), key                   # the freeze fell inside the run
        if (num_agents, num_envs) in DIRECT:
            assert tool.play(torch, PlainEntries(torch, num_envs, num_agents, games_num), rews, dones) == want, f"{key}: the plain C entries"


# ------------------------------------------------------------------------------------------------------- the Player
def make_plain(name, n, seed, episode_length=12):
    from isaacgym_amd import scene
    from isaacgym_amd.tasks import isaacgym_task_map
    cfg = scene.default_task_cfg(scene.TASK_VARIANTS[name])
    cfg["env"]["numEnvs"], cfg["seed"] = n, seed
    cfg["env"]["episodeLength"] = episode_length
    return isaacgym_task_map[name](cfg, DEV, DEV, -1, True, False, False)


def make_randomized(name, n, seed):
    """randomize: True with the golden yaml block, redrawn per env at its reset on the device (apply_at: "reset")."""
    import dr_shim_binding as drs
    from test_dr_reset_gpu import make_task
    return make_task(name, n, seed, drs.task_block(name), env={"episodeLength": 12}, frequency=5, apply_at="reset")


_CKPT = {}


@pytest.fixture(scope="module")
def checkpoint(torch_cuda, tmp_path_factory):
    """name -> a checkpoint file of a PPOTrainer-initialised network for that task (tr.save: rl_games' layout), written once."""
    def get(name):
        if name not in _CKPT:
            import isaacgym_amd
            from isaacgym_amd import ppo
            n = 64
            task = isaacgym_amd.make(seed=9, task=name, num_envs=n)
            rows = n * task.num_agents
            tr = ppo.PPOTrainer(task, ppo.PPOConfig(minibatch_size=32 * rows), seed=9)
            path = str(tmp_path_factory.mktemp("play") / f"{name}.pth")
            tr.save(path)
            _CKPT[name] = path
        return _CKPT[name]
    return get


def load_policy(path):
    from isaacgym_amd.policy import RLGamesPolicy
    return RLGamesPolicy.load(path, DEV)


def host_loop(torch, task, policy, n_games, deterministic=True, seed=0, max_steps=400):
    """rl_games' BasePlayer.run on the live task, with its per-step host read: the shape of test_play_host.rlgames_loop (and its result
    dict), driven by the policy."""
    A = task.num_agents
    rows = task.num_envs * A
    task.reset_idx()
    policy._counter = 0
    obs = task.reset()["obs"]
    cr = torch.zeros(rows, dtype=torch.float32, device=DEV)
    steps = torch.zeros(rows, dtype=torch.int64, device=DEV)
    games = sum_steps = launches = 0
    returns = [[] for _ in range(A)]
    broke_at = None
    for t in range(max_steps):
        actions, _ = policy.act(obs, deterministic=deterministic, seed=seed)
        od, r, done, _ = task.step(actions)
        obs = od["obs"]
        cr += r
        steps += 1
        launches += 1
        all_done = done.nonzero(as_tuple=False).flatten()                      # the host read of every step
        done_idx = all_done[::A]
        games += len(done_idx)
        if len(done_idx) > 0:
            sum_steps += int(steps[done_idx].sum())
            for a in range(A):
                returns[a] += [float(x) for x in cr[done_idx + a].cpu().numpy()]
            cr[all_done] = 0.0
            steps[all_done] = 0
            if games >= n_games:
                broke_at = t
                break
    assert broke_at is not None, f"{games} of {n_games} games within {max_steps} steps"
    return dict(games=games, steps=sum_steps, launches=launches, returns=returns, cr=cr.cpu().numpy(),
                cur_steps=steps[::A].cpu().numpy().astype(np.int32), broke_at=broke_at)


def play_and_compare(torch, make, name, n, games_num, path, poll_every=64, **kw):
    from isaacgym_amd.play import Player
    pl = Player(make(name, n, 21), load_policy(path), games_num=games_num, poll_every=poll_every, max_steps=2000, **kw)
    res = pl.run()
    ref = host_loop(torch, make(name, n, 21), load_policy(path), games_num, deterministic=kw.get("deterministic", True), seed=kw.get("seed", 0))
    tot = pl.stats.read()
    check_against_loop(tot, pl.stats.state_bytes(), ref, pl.num_agents, what=f"Player vs host loop, {name}")
    assert res["games"] == ref["games"] >= games_num and res["av_steps"] == ref["steps"] / ref["games"]
    assert res["steps_played"] >= ref["launches"] and res["steps_played"] % poll_every == 0 and res["seconds"] > 0
    x0 = np.asarray(ref["returns"][0])
    assert res["av_reward"] == pytest.approx(x0.mean(), rel=1e-12, abs=1e-12)                 # agent 0's
    assert res["reward_std"] == pytest.approx(x0.std(), rel=1e-6, abs=1e-9)
    assert (res["reward_min"], res["reward_max"]) == (x0.min(), x0.max())
    return pl, res, ref


def test_player_matches_host_synchronised_loop(torch_cuda, checkpoint):
    pl, res, ref = play_and_compare(torch_cuda, make_plain, TT, 130, 200, checkpoint(TT))
    assert len(res["per_agent"]) == 1 and ref["launches"] < 64                               # the poll came after the crossing: frozen since


def test_polling_does_not_change_the_result(torch_cuda, checkpoint):
    from isaacgym_amd.play import Player
    states, played = [], []
    for poll in (1, 7, 64):
        pl = Player(make_plain(TT, 130, 21), load_policy(checkpoint(TT)), games_num=200, poll_every=poll, max_steps=2000)
        pl.run()
        states.append(pl.stats.state_bytes())
        played.append(pl.steps_played)
    assert states[0] == states[1] == states[2]
    assert played[0] <= played[1] <= played[2] == 64 and played[0] < 64 and played[1] % 7 == 0     # they stopped at different steps


def test_player_under_reset_time_randomisation(torch_cuda, checkpoint):
    pl, res, ref = play_and_compare(torch_cuda, make_randomized, TT, 130, 200, checkpoint(TT))
    assert pl.task.randomize and pl.task._dr_reset
    assert int(pl.task.env.reset_randomization.draws.sum()) > 130                            # envs did redraw at their resets
    plain = host_loop(torch_cuda, make_plain(TT, 130, 21), load_policy(checkpoint(TT)), 200)
    assert plain["returns"][0] != ref["returns"][0]                                          # ... and the play ran under the randomisation


def test_player_27dof(torch_cuda, checkpoint):
    pl, res, ref = play_and_compare(torch_cuda, make_plain, TA, 64, 64, checkpoint(TA), poll_every=16)
    assert pl.task.num_obs == 313 and res["games"] >= 64


def test_player_4_actor_counts_envs_and_reports_both_agents(torch_cuda, checkpoint):
    pl, res, ref = play_and_compare(torch_cuda, make_plain, T4, 64, 64, checkpoint(TT), poll_every=16)
    assert pl.num_agents == 2 and pl.stats.rows == 128
    assert res["games"] == ref["games"] <= 64 + 64 - 1                                       # envs, not rows (rows would give twice as many)
    assert len(res["per_agent"]) == 2 and res["per_agent"][0] != res["per_agent"][1]
    assert res["av_reward"] == res["per_agent"][0]["av_reward"]
    x1 = np.asarray(ref["returns"][1])
    assert res["per_agent"][1]["av_reward"] == pytest.approx(x1.mean(), rel=1e-12, abs=1e-12)


def test_stochastic_play(torch_cuda, checkpoint):
    torch = torch_cuda
    from isaacgym_amd.play import Player

    def play(**kw):
        pl = Player(make_plain(TT, 130, 21), load_policy(checkpoint(TT)), games_num=200, max_steps=2000, **kw)
        res = pl.run()
        return pl, res
    det = play()[1]["av_reward"]
    a, ra = play(deterministic=False, seed=5)
    b, rb = play(deterministic=False, seed=5)
    assert a.stats.state_bytes() == b.stats.state_bytes()
    p6, r6 = play(deterministic=False, seed=5, sigma=-6.0)
    p1, r1 = play(deterministic=False, seed=5, sigma=-1.0)
    assert float(p6.policy.sigma[0]) == pytest.approx(np.exp(-6.0), rel=1e-6) and float(p1.policy.sigma[0]) == pytest.approx(np.exp(-1.0), rel=1e-6)
    d6, d1 = abs(r6["av_reward"] - det), abs(r1["av_reward"] - det)
    print(f"stochastic play: |av - deterministic av| sigma=-6: {d6:.6g}, sigma=-1: {d1:.6g}, deterministic av {det:.6g}")
    if d6 == 0.0 and d1 == 0.0:
        assert not torch.equal(p6.actions, p1.actions)
    else:
        assert d6 < d1
    # the stochastic player against the host loop with the same seed
    play_and_compare(torch, make_plain, TT, 130, 200, checkpoint(TT), deterministic=False, seed=5)


def test_cli(torch_cuda, checkpoint, capsys):
    from isaacgym_amd import play
    res = play.main(["--task", TT, "--checkpoint", checkpoint(TT), "--num-envs", "130", "--games", "50", "--poll-every", "16", "--seed", "3"])
    out = capsys.readouterr().out
    assert res["games"] >= 50 and res["steps_played"] % 16 == 0
    lines = out.splitlines()
    assert any(l.startswith("reward: ") and " steps: " in l for l in lines)
    assert any(l.startswith("av reward: ") and " av steps: " in l for l in lines), out
