"""Training with an observation and action history on the MI355X (PPOTrainer(history=); RolloutCollector(history=);
include/ppenv_history.h): every row of the collector's wide horizon is history.reference applied to the row before it, under a sensing
and a command delay line, on the 7-dof and the 4-actor task; the run is finite and learns; without the argument the trainer is bitwise
the trainer from before; the checkpoint carries the record, refuses another one and serves RLGamesPolicy; privileged columns start at W.
64 actor rows, horizon 4, minibatches of 64 rows, two mini-epochs, 5-step games.  Need a real MI355X."""
import numpy as np
import pytest

from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper, a fixture)
from test_ppo_latency_gpu import learned_state, same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TT, T4 = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1"
H, SEED = 4, 21
LATENCY = dict(obs_delay=1, action_delay=(0, 2))


def trainer(name, num_envs=64, seed=SEED, **kw):
    """init_scale 512: the yaml's loss scale per row at 64-row minibatches (65536 / 8192 = 8 per row)."""
    from isaacgym_amd import ppo
    cfg = ppo.PPOConfig(horizon_length=H, minibatch_size=64, mini_epochs=2, init_scale=512.0)
    return ppo.PPOTrainer(make_plain(name, num_envs, seed, 5), cfg, seed=seed, **kw)


def check_horizon(tr, first):
    """Every row t + 1 of the horizon is the reference applied to row t, the observation row t + 1 begins with, actions[t] and dones[t]."""
    from isaacgym_amd import history
    col, rec, A = tr.col, tr.history(), tr.env.num_agents
    n, a, ho, ha = rec["num_obs"], rec["num_actions"], rec["obs"], rec["actions"]
    obs, actions, dones = col.obs.cpu().numpy(), col.actions.cpu().numpy(), col.dones.cpu().numpy()
    if first:                                                  # row 0 of the first horizon: pushed with no previous row
        assert np.array_equal(obs[0].view(np.int32), history.reference(None, obs[0][:, :n], None, None, n, a, ho, ha, A).view(np.int32))
    for t in range(H):
        want = history.reference(obs[t], obs[t + 1][:, :n], actions[t], dones[t], n, a, ho, ha, A)
        assert np.array_equal(obs[t + 1].view(np.int32), want.view(np.int32)), t
    return obs, dones


def epochs(torch, tr, count):
    stats = [tr.train_epoch() for _ in range(count)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values() if v.dim() == 0])
    assert bool(torch.isfinite(vals).all())
    return vals


@pytest.mark.parametrize("name, num_envs", [(TT, 64), (T4, 32)], ids=["7dof", "4actor"])
def test_wide_horizon_follows_the_rule_trains_and_its_checkpoint_carries_the_record(torch_cuda, tmp_path, name, num_envs):
    torch = torch_cuda
    from isaacgym_amd import history
    from isaacgym_amd.policy import RLGamesPolicy
    tr = trainer(name, num_envs, history=(2, 2), **LATENCY)
    n, a = tr.env.obs_buf.shape[1], tr.num_actions
    rec = tr.history()
    W = 3 * n + 2 * a
    assert rec == dict(obs=2, actions=2, num_obs=n, num_actions=a, width=W) == history.parse((2, 2), n, a)
    assert tr.num_obs == W and tr.base_num_obs == n and tr.rows == 64
    col = tr.col
    assert col.obs.shape == (H + 1, 64, W) and col.history.num_agents == tr.env.num_agents and col.seen_obs.shape == col.raw_obs.shape == (64, n)
    assert col.cur_obs is None and tr.learner.net.num_obs == W and tr.learner.net.w[0].shape[-1] == (W + 63) // 64 * 64
    assert tr.learner.rms.num_obs == W
    tr.collect()
    obs0, dones0 = check_horizon(tr, first=True)
    col.next_horizon()
    tr.collect()
    obs1, dones1 = check_horizon(tr, first=False)
    assert np.array_equal(obs1[0].view(np.int32), obs0[H].view(np.int32))                       # row 0 of the second horizon is row H of the first
    both = np.concatenate([dones0, dones1])
    assert both.any() and not both.all()                                                        # resets and carried rows were both checked
    col.next_horizon()
    before = learned_state(tr)
    epochs(torch, tr, 2)
    assert not same(torch, learned_state(tr), before)
    assert float(tr.learner.rms.count) > 1
    path = str(tmp_path / "nn" / "run.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["history"] == rec and ck["model"]["a2c_network.actor_mlp.0.weight"].shape[1] == W == ck["model"]["a2c_network.critic_mlp.0.weight"].shape[1]
    assert ck["model"]["running_mean_std.running_mean"].shape == (W,)
    pol = RLGamesPolicy.load(path, DEV)
    assert pol.history == rec and pol.base_num_obs == n and pol.net.num_obs == W
    act, _ = pol.act(col.obs[0].clone(), deterministic=True)                                    # the wide rows are what it serves
    assert act.shape == (64, a) and bool(torch.isfinite(act).all()) and float(act.abs().max()) <= 1.0
    if name == TT:
        other = trainer(name, num_envs, history=(2, 1), **LATENCY)
        with pytest.raises(ValueError, match=r"history: the checkpoint was trained with history \{'obs': 2, 'actions': 2.* this trainer has history \{'obs': 2, 'actions': 1"):
            other.load(path)
        plain = trainer(name, num_envs, **LATENCY)
        with pytest.raises(ValueError, match="this trainer has no history"):
            plain.load(path)
        tr.load(path)                                                                            # its own record: accepted


def test_without_the_argument_the_trainer_is_bitwise_the_trainer_from_before(torch_cuda):
    torch = torch_cuda
    runs = []
    for kw in ({}, dict(history=None), dict(history=(0, 0))):
        tr = trainer(TT, **kw)
        vals = epochs(torch, tr, 2)
        assert tr.history() is None and tr.col.history is None and tr.col.cur_obs is None and tr.col.seen_obs is None and tr.num_obs == tr.base_num_obs
        assert "history" not in tr.state_dict()
        runs.append((learned_state(tr), vals, [getattr(tr.learner.rms, k).clone() for k in ("running_mean", "running_var", "count", "mean", "inv_std")]))
    for state, vals, rms in runs[1:]:
        assert same(torch, state, runs[0][0]) and torch.equal(vals, runs[0][1])
        assert all(torch.equal(x, y) for x, y in zip(rms, runs[0][2]))                          # (fp64 and 0-dim tensors among them: compared as values, none is NaN)


def test_history_without_a_sensing_line_steps_into_cur_obs(torch_cuda):
    torch = torch_cuda
    tr = trainer(TT, history=(1, 0))
    n = tr.base_num_obs
    assert tr.num_obs == 2 * n and tr.col.cur_obs.shape == (64, n) and tr.col.raw_obs is None and tr.col.seen_obs is None
    tr.collect()
    check_horizon(tr, first=True)
    assert torch.equal(tr.col.obs[H][:, :n], tr.col.cur_obs)
    epochs(torch, tr, 1)


def test_privileged_columns_start_at_the_wide_width_and_raw_obs_stays_narrow(torch_cuda):
    torch = torch_cuda
    tr = trainer(TT, history=(2, 2), critic_inputs=("raw_obs",), **LATENCY)
    n, W = tr.base_num_obs, tr.num_obs
    assert W == 3 * n + 2 * tr.num_actions and tr.critic_inputs() == dict(names=["raw_obs"], columns=[n], P=n)
    assert tr.col.priv.shape == (H + 1, 64, n) and tr.learner.num_priv == n and tr.learner.net.w[0].shape[-1] == (W + n + 63) // 64 * 64
    actor0, critic0 = tr.learner.layer_weights(0)
    assert actor0.shape[1] == W and critic0.shape[1] == W + n
    assert bool((tr.learner.w32[0][0][:, W:] == 0).all())                                         # the actor reads no privileged column
    tr.collect()
    check_horizon(tr, first=True)
    assert torch.equal(tr.col.priv[H], tr.col.raw_obs)
    tr.col.next_horizon()
    epochs(torch, tr, 1)
    from isaacgym_amd import collector
    with pytest.raises(ValueError, match="history: .* but the network was built with num_obs"):
        collector.RolloutCollector(tr.env, tr.roll_net, horizon=H, history=(1, 1))
