"""Training under sensor noise and dropouts on the MI355X (RolloutCollector / PPOTrainer(obs_noise=, obs_drop=, action_noise=, action_drop=,
sensor_columns=); include/ppenv_sensor.h).

The collector against isaacgym_amd.sensor.reference fed what on_step sees — the clean observations, the policy's actions, the dones —
across horizon boundaries and resets, with the level draws scene.sensor_draws predicts, alone and in front of a delay line and a history;
then what the trainer promises: zero levels are the trainer without the arguments, the raw_obs critic input stays clean, the checkpoint
carries the record.  64 envs, horizon 8, minibatch 64 * 8, env.episodeLength 12.  Need a real MI355X."""
import numpy as np
import pytest

import sensor_shim_binding as sb
import train_delay_shim_binding as td
from test_play_gpu import make_plain, torch_cuda        # noqa: F401  (a helper, a fixture)
from test_ppo_latency_gpu import learned_state, same, u32
from test_rng_streams_gpu import E_MEASURED

pytestmark = pytest.mark.gpu

TT, T4 = "HumanoidPingpongTiltG1", "Humanoid12PingpongTiltG1"
DEV = "cuda:0"
N, H, SEED = 64, 8, 21
BALL = "ball_pos,ball_vel"
NOISY = dict(obs_noise=(0.0, 0.02), obs_drop=0.2, action_noise=0.05, action_drop=(0.0, 0.6),
             sensor_columns=dict(obs_noise_columns=BALL, obs_drop_columns=BALL, action_drop_columns="0:4"))


def trainer(name=TT, seed=SEED, **kw):
    from isaacgym_amd import ppo
    rows = N * (2 if name == T4 else 1)
    return ppo.PPOTrainer(make_plain(name, N, seed), ppo.PPOConfig(horizon_length=H, minibatch_size=rows * H), seed=seed, **kw)


@pytest.mark.parametrize("name, extra", [(TT, {}), (T4, {}), (TT, dict(obs_delay=1)), (TT, dict(history=(1, 1)))], ids=["tilt", "four-actor", "obs-delay", "history"])
def test_collector_follows_the_reference_across_horizons_and_resets(torch_cuda, name, extra):
    torch = torch_cuda
    from isaacgym_amd import scene, sensor
    tr = trainer(name, **NOISY, **extra)
    col, A = tr.col, tr.env.num_agents
    rows, n_obs, n_act = N * A, tr.base_num_obs, tr.num_actions
    seed = scene.stream_seed(SEED, scene.STREAM_SENSOR)
    assert col.obs_sensor.seed == col.act_sensor.seed == seed and (col.obs_sensor.draw, col.obs_sensor.channel, col.act_sensor.channel) == (1, 1, 0)
    assert tr.sensor() == dict(obs_noise=[0.0, 0.02], obs_drop=[0.2, 0.2], action_noise=[0.05, 0.05], action_drop=[0.0, 0.6],
                               columns=dict(obs_noise_columns=BALL, obs_drop_columns=BALL, action_noise_columns=None, action_drop_columns="0:4"))
    assert col.raw_obs.shape == (rows, n_obs) and col.applied.shape == (rows, n_act) and (col.sensed_obs is None) == (not extra)
    ball = sensor.columns(tr.task, BALL, n_obs)
    ref_obs = sensor.reference(rows, n_obs, A, sigma=(0.0, 0.02), drop=0.2, columns=ball, hold_columns=ball, seed=seed, channel=sensor.SENSING)
    ref_act = sensor.reference(rows, n_act, A, sigma=0.05, drop=(0.0, 0.6), hold_columns=sensor.hold_columns(None, "0:4", n_act, sensor.COMMAND), seed=seed,
                               channel=sensor.COMMAND)
    ref_line = td.NumpyLine(rows, n_obs, 1, 1, A, scene.stream_seed(SEED, scene.STREAM_LATENCY), 0, td.SENSING) if "obs_delay" in extra else None
    sensed = lambda row: col.obs[row] if not extra else col.sensed_obs                         # where the sensing sensor wrote

    def check_obs(k, raw, done, sensed_now, row_now):
        ref_obs.push(raw.cpu().numpy(), done)
        sb.compare(u32(sensed_now), dict(out=ref_obs.out.view(np.uint32), s=ref_obs.s, mag=ref_obs.mag), 4 * E_MEASURED, (name, k))
        if ref_line is not None:                                                               # the sensor comes first: the line delays what it delivered
            assert np.array_equal(u32(row_now), ref_line.push(u32(sensed_now), done)), k
        if "history" in extra:                                                                 # o_0 of the wide row is what the sensor delivered
            assert np.array_equal(u32(row_now[:, :n_obs]), u32(sensed_now)), k
    # obs[0] of the very first horizon: the initial observation (still in raw_obs), pushed with no done
    check_obs(-1, col.raw_obs, None, sensed(0), col.obs[0])
    seen = []

    def on_step():
        t = len(seen) % H
        seen.append(tuple(x.clone() for x in (col.raw_obs, sensed(t + 1), col.obs[t + 1], col.actions[t], col.applied, col.dones[t], col.obs_sensor.sigma,
                                              col.obs_sensor.drop, col.obs_sensor.episode, col.act_sensor.drop)))
    col.on_step = on_step
    for h in range(3):
        col.collect()
        col.next_horizon()
    assert len(seen) == 3 * H
    done_prev, restarts, dropped, sigmas = None, 0, 0, set()
    r = np.arange(rows)
    for k, (raw, sensed_now, row_now, actions, applied, dones, sg, dp, episode, act_dp) in enumerate(seen):
        dn = dones.cpu().numpy()
        ref_act.push(actions.cpu().numpy(), done_prev)                                         # the done the PREVIOUS env step returned
        sb.compare(u32(applied), dict(out=ref_act.out.view(np.uint32), s=ref_act.s, mag=ref_act.mag), 4 * E_MEASURED, (name, "applied", k))
        assert not np.array_equal(u32(applied), u32(actions))                                  # the stored actions stay the policy's own
        check_obs(k, raw, dn, sensed_now, row_now)                                             # this step's done
        clean = np.r_[0:74]
        if not extra:
            assert np.array_equal(u32(row_now)[:, clean], u32(raw)[:, clean]), k               # the encoders' columns are copied bit for bit
        for agent in range(A):                                                                 # the levels are what scene.sensor_draws predicts
            rr = r[agent::A]
            want_sg, want_dp = scene.sensor_draws(seed, rr // A, episode.cpu().numpy()[rr] - 1, sensor.SENSING, (0.0, 0.02), (0.2, 0.2), num_agents=A, agent=agent)
            assert np.array_equal(sg.cpu().numpy()[rr], want_sg) and np.array_equal(dp.cpu().numpy()[rr], want_dp), (k, agent)
        assert np.array_equal(act_dp.cpu().numpy(), ref_act.drop) and np.array_equal(episode.cpu().numpy(), ref_obs.episode), k
        sigmas |= set(sg.cpu().numpy().tolist())
        restarts += int((dn.reshape(-1, A)[:, 0] != 0).sum())
        dropped += int(ref_obs.dropped.sum())
        done_prev = dn
    assert restarts >= N and len(sigmas) > N and 0.1 * rows * 3 * H < dropped < 0.3 * rows * 3 * H


@pytest.fixture(scope="module")
def plain_run(torch_cuda):
    tr = trainer()
    stats = [tr.train_epoch() for _ in range(2)]
    return tr, learned_state(tr), torch_cuda.stack([v.detach().double() for s in stats for v in s.values()])


def test_zero_levels_are_the_trainer_without_the_arguments(torch_cuda, plain_run):
    torch = torch_cuda
    tr0, state0, vals0 = plain_run
    tr = trainer(obs_noise=0, obs_drop=(0.0, 0.0), action_noise=0.0, action_drop="0", sensor_columns=dict(obs_noise_columns="ball_pos"))
    stats = [tr.train_epoch() for _ in range(2)]
    vals = torch.stack([v.detach().double() for s in stats for v in s.values()])
    assert same(torch, learned_state(tr), state0) and torch.equal(vals, vals0)                 # weights, moments, statistics: bitwise
    if tr.learner.rms is not None:
        assert same(torch, [tr.learner.rms.mean, tr.learner.rms.inv_std], [tr0.learner.rms.mean, tr0.learner.rms.inv_std])
    for t in (tr, tr0):
        c = t.col
        assert c.obs_sensor is None and c.act_sensor is None and c.raw_obs is None and c.applied is None and c.sensed_obs is None and c.delayed is None
        assert t.sensor() is None and "sensor" not in t.state_dict()


def test_a_noisy_run_is_reproducible_and_differs_from_the_plain_one(torch_cuda, plain_run):
    torch = torch_cuda
    _, state0, _ = plain_run
    runs = []
    for _ in range(2):
        tr = trainer(**NOISY)
        stats = [tr.train_epoch() for _ in range(2)]
        runs.append((learned_state(tr), torch.stack([v.detach().double() for s in stats for v in s.values()])))
    assert same(torch, runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.isfinite(runs[0][1]).all()
    assert not same(torch, runs[0][0], state0)


def test_the_raw_obs_critic_input_stays_clean(torch_cuda):
    torch = torch_cuda
    tr = trainer(obs_delay=1, critic_inputs=("raw_obs",), obs_noise=0.05, obs_drop=0.3)
    col, seen = tr.col, []

    def on_step():
        t = len(seen)
        seen.append((col.raw_obs.clone(), col.priv[t + 1].clone(), col.sensed_obs.clone()))
    col.on_step = on_step
    col.collect()
    assert len(seen) == H
    for raw, priv, sensed in seen:
        assert np.array_equal(u32(priv), u32(raw)) and not np.array_equal(u32(sensed), u32(raw))
    col.on_step = None
    tr.train_epoch()                                                                          # the critic trains on the clean columns


def test_checkpoints_carry_the_record_and_old_ones_load(torch_cuda, tmp_path):
    torch = torch_cuda
    tr = trainer(**NOISY)
    tr.train_epoch()
    path, old = str(tmp_path / "sensor.pth"), str(tmp_path / "old.pth")
    tr.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["sensor"] == tr.sensor() and ck["sensor"]["obs_noise"] == [0.0, 0.02] and ck["sensor"]["columns"]["action_drop_columns"] == "0:4"
    fresh = trainer(**NOISY)
    assert fresh.loaded_sensor is None
    fresh.load(path)
    assert fresh.loaded_sensor == ck["sensor"] and fresh.epoch == 1 and same(torch, learned_state(fresh), learned_state(tr))
    del ck["sensor"]                                                                          # a file without the record
    torch.save(ck, old)
    fresh.load(old)
    assert fresh.loaded_sensor is None and fresh.epoch == 1
    plain = trainer()
    plain.load(path)                                                                          # a record, not a contract: a trainer without sensors loads it
    assert plain.sensor() is None and plain.loaded_sensor == ck_sensor(path, torch)
    from isaacgym_amd.policy import RLGamesPolicy
    a, v = RLGamesPolicy.load(path, DEV).act(tr.col.obs[0], deterministic=True)                # play does not read the record
    assert a.shape == (N, tr.num_actions) and torch.isfinite(a).all()
    fresh.train_epoch()                                                                       # a resumed run goes on


def ck_sensor(path, torch):
    return torch.load(path, map_location="cpu", weights_only=True)["sensor"]
