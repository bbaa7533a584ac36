"""Training under control latency on the MI355X (RolloutCollector / PPOTrainer(action_delay=, obs_delay=); include/ppenv_train_delay.h).

The collector against the rule in numpy (train_delay_shim_binding.NumpyLine with scene.latency_draws) fed what on_step sees — the raw
observations, the policy's actions, the dones — across horizon boundaries and resets, bitwise; then what the trainer promises: zero delay is
the trainer without the arguments, a delayed run is reproducible and different, the checkpoint carries the ranges.  The tasks run with
env.episodeLength 12.  Need a real MI355X."""
import numpy as np
import pytest

import train_delay_shim_binding as td
from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper, a fixture)

pytestmark = pytest.mark.gpu

TT, T4 = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
H = 8
SEED = 21


def trainer(name, num_envs, seed=SEED, **kw):
    from isaacgym_amd import ppo
    return ppo.PPOTrainer(make_plain(name, num_envs, seed), ppo.PPOConfig(horizon_length=H, minibatch_size=256), seed=seed, **kw)


def u32(t):
    """A float32 device tensor's words as uint32 numpy."""
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- the collector
@pytest.mark.parametrize("name, num_envs", [(TT, 64), (T4, 32)], ids=["tilt", "four-actor"])
def test_collector_follows_the_rule_across_horizons_and_resets(torch_cuda, name, num_envs):
    torch = torch_cuda
    from isaacgym_amd import scene
    tr = trainer(name, num_envs, action_delay=(0, 2), obs_delay=1)
    col, A = tr.col, tr.env.num_agents
    rows = num_envs * A
    assert (col.action_delay, col.obs_delay) == ((0, 2), (1, 1)) and tr.latency() == dict(control_dt=tr.env.control_dt, action_delay=[0, 2], obs_delay=[1, 1])
    assert col.applied.shape == (rows, tr.num_actions) and col.raw_obs.shape == (rows, tr.num_obs)
    assert (col.act_line.lo, col.act_line.hi, col.act_line.channel, col.obs_line.lo, col.obs_line.hi, col.obs_line.channel) == (0, 2, 0, 1, 1, 1)
    seed = scene.stream_seed(SEED, scene.STREAM_LATENCY)
    assert col.act_line.seed == col.obs_line.seed == seed
    ref_act = td.NumpyLine(rows, tr.num_actions, 0, 2, A, seed, 0, td.COMMAND)
    ref_obs = td.NumpyLine(rows, tr.num_obs, 1, 1, A, seed, 0, td.SENSING)
    # obs[0] of the very first horizon: the initial observation (still in raw_obs), pushed with no done
    assert np.array_equal(u32(col.obs[0]), ref_obs.push(u32(col.raw_obs), None))
    seen = []

    def on_step():
        t = len(seen) % H
        seen.append(tuple(x.clone() for x in (col.raw_obs, col.applied, col.actions[t], col.dones[t], col.obs[t + 1], col.act_line.delays, col.obs_line.delays,
                                              col.act_line.episode)))
    col.on_step = on_step
    last_obs = None
    for h in range(3):
        if last_obs is not None:
            assert torch.equal(col.obs[0], last_obs)                                           # the delayed observation is carried over
        col.collect()
        last_obs = col.obs[H].clone()
        col.next_horizon()
    assert len(seen) == 3 * H
    done_prev, restarts, delays_seen = None, 0, set()
    for k, (raw_obs, applied, actions, dones, obs_next, d_act, d_obs, episode) in enumerate(seen):
        dn = dones.cpu().numpy()
        assert np.array_equal(u32(applied), ref_act.push(u32(actions), done_prev)), k           # the done the PREVIOUS env step returned
        assert np.array_equal(u32(obs_next), ref_obs.push(u32(raw_obs), dn)), k                 # this step's done
        assert np.array_equal(d_act.cpu().numpy(), ref_act.delay) and np.array_equal(episode.cpu().numpy(), ref_act.episode), k
        assert (d_obs == 1).all()
        d = d_act.cpu().numpy().reshape(-1, A)
        assert (d == d[:, :1]).all()                                                           # both rows of an env hold the env's delay
        delays_seen |= set(d.ravel().tolist())
        restarts += int((dn.reshape(-1, A)[:, 0] != 0).sum())
        done_prev = dn
    assert restarts >= num_envs                                                                # 24 steps of 12-step episodes: every env restarted
    assert delays_seen == {0, 1, 2}
    # the table is what latency_draws predicts for every env's running episode
    e = ref_act.episode.reshape(-1, A)[:, 0]
    assert np.array_equal(ref_act.delay.reshape(-1, A)[:, 0], scene.latency_draws(seed, np.arange(num_envs), e - 1, 0, 0, 2))


# ---------------------------------------------------------------------------------------------------------------------- the trainer
def learned_state(tr):
    """Parameters, moments and the scaler's current row, cloned."""
    return [t.detach().clone() for t in tr.learner.parameters() + [tr.logstd] + tr.opt.exp_avg + tr.opt.exp_avg_sq + [tr.opt.state[tr.opt.cur]]]


def same(torch, a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32) if x.is_floating_point() else x,
                                                                       y.view(torch.int32) if y.is_floating_point() else y) for x, y in zip(a, b))


def run_epochs(torch, epochs=2, **kw):
    tr = trainer(TT, 64, **kw)
    stats = [tr.train_epoch() for _ in range(epochs)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values()])
    return tr, learned_state(tr), vals


@pytest.fixture(scope="module")
def plain_run(torch_cuda):
    """Two epochs of a trainer built WITHOUT the arguments: (trainer, its learned state, every stat of both epochs)."""
    return run_epochs(torch_cuda)


def test_zero_delay_is_the_trainer_without_the_arguments(torch_cuda, plain_run):
    torch = torch_cuda
    tr0, state0, vals0 = plain_run
    tr, state, vals = run_epochs(torch, action_delay=0, obs_delay=(0, 0))
    assert same(torch, state, state0) and torch.equal(vals, vals0)
    for t in (tr, tr0):
        assert t.col.act_line is None and t.col.obs_line is None and t.col.applied is None and t.col.raw_obs is None       # no line is allocated
        assert t.latency() == dict(control_dt=t.env.control_dt, action_delay=[0, 0], obs_delay=[0, 0])


def test_a_delayed_run_is_reproducible_and_differs_from_the_plain_one(torch_cuda, plain_run):
    torch = torch_cuda
    _, state0, _ = plain_run
    tr_a, a, vals_a = run_epochs(torch, action_delay=1)
    tr_b, b, vals_b = run_epochs(torch, action_delay=1)
    assert same(torch, a, b) and torch.equal(vals_a, vals_b)
    assert not same(torch, a, state0)
    assert torch.isfinite(vals_a).all()
    assert tr_a.col.act_line is not None and tr_a.col.obs_line is None and tr_a.col.raw_obs is None
    # applied[t] is the previous step's action wherever the row's age says the episode has one
    col, seen = tr_a.col, []

    def on_step():
        t = len(seen)
        seen.append((col.actions[t].clone(), col.applied.clone(), col.act_line.age.clone()))
    col.on_step = on_step
    prev = col.actions[H - 1].clone()                                                          # the last action of the horizon before
    col.collect()
    old = 0
    for actions, applied, age in seen:
        has_prev = age >= 2                                                                   # the age AFTER the push: this sample was not the episode's first
        assert torch.equal(applied[has_prev], prev[has_prev]) and torch.equal(applied[~has_prev], actions[~has_prev])
        old += int(has_prev.sum())
        prev = actions
    assert 0 < old < H * 64                                                                   # both kinds of row were met


def test_checkpoints_carry_the_latency_and_old_ones_load(torch_cuda, tmp_path):
    torch = torch_cuda
    from isaacgym_amd.policy import RLGamesPolicy
    tr = trainer(TT, 64, action_delay=(1, 3), obs_delay=2)
    tr.train_epoch()
    path, old = str(tmp_path / "lat.pth"), str(tmp_path / "old.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["latency"] == {"action_delay": [1, 3], "obs_delay": [2, 2]}
    fresh = trainer(TT, 64, action_delay=(1, 3), obs_delay=2)
    assert fresh.loaded_latency is None
    fresh.load(path)
    assert fresh.loaded_latency == ck["latency"] and fresh.epoch == 1
    assert same(torch, learned_state(fresh), learned_state(tr))
    assert fresh.latency()["action_delay"] == [1, 3]                                           # the trainer keeps the delays it was built with
    del ck["latency"]                                                                         # a file from before the key
    torch.save(ck, old)
    fresh.load(old)
    assert fresh.loaded_latency is None and fresh.epoch == 1
    for p in (path, old):
        policy = RLGamesPolicy.load(p, DEV)
        a, v = policy.act(tr.col.obs[0], deterministic=True)
        assert a.shape == (64, tr.num_actions) and torch.isfinite(a).all() and torch.isfinite(v).all()
    fresh.train_epoch()                                                                       # a resumed run goes on
