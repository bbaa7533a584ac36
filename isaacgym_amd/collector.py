"""A rollout horizon collected natively (the data format on the learner's side of the path).

rl_games' a2c agent plays `horizon_length` steps per epoch and keeps every per-step tensor in an experience buffer laid out
[horizon, num_actors, ...] (cfg/train/HumanoidPingpongTiltG1PPO.yaml:73 horizon_length: 32; a2c_common.py play_steps: obses, actions,
neglogpacs, values, rewards, dones, then discount_values for returns / advantages).  With PyTorch that is a dozen small indexing
kernels per step next to the forward.  Here every producer writes STRAIGHT into its horizon-major slice:

    the env step    (ppenv_ta_step)           obs[t + 1], rewards[t], dones[t]
    the heads launch (ppenv_mlp_heads_sample) mu | value [t], actions[t], neglogp[t]
    ppenv_gae                                 advantages, returns over the finished horizon

so a horizon costs exactly the launches of `horizon` rollout steps, one bootstrap forward and one GAE launch — no copies, no host
synchronisation.  The learner (rl_games / PyTorch autograd) consumes the buffers as they are.  Works with TAEnv (the 27-DoF task of
BASELINE config 5: ppenv_ta_step takes its output pointers per call) and with PPEnv (the 7-dof tasks: ppenv_step_into; the 4-actor
variant has two actor rows per env).
"""
import ctypes as C

import torch

from . import _lib
from . import history as history_mod
from . import sensor as sensor_mod
from .latency import COMMAND, SENSING, DelayLine, delay_range


def gae(rewards, values, dones, gamma=0.99, tau=0.95, reward_scale=1.0, advantages=None, returns=None):
    """ppenv_gae on torch tensors: rewards [H, N] fp32, values [H + 1, N] (any row stride: a column view of the heads' output),
    dones [H, N] int64 -> (advantages, returns) [H, N]."""
    h, n = rewards.shape
    assert values.shape[0] == h + 1 and values.shape[1] == n and dones.dtype == torch.int64 and rewards.is_contiguous() and dones.is_contiguous()
    adv = torch.empty_like(rewards) if advantages is None else advantages
    ret = torch.empty_like(rewards) if returns is None else returns
    _lib.check(_lib.lib().ppenv_gae(rewards.data_ptr(), values.data_ptr(), values.stride(1), values.stride(0), dones.data_ptr(), h, n, gamma, tau,
                                    reward_scale, adv.data_ptr(), ret.data_ptr(), _lib.stream(rewards)))
    return adv, ret


class RolloutCollector:
    """`collect()` plays `horizon` steps of env + policy and leaves the horizon in `obs [H+1, N, num_obs]`, `actions [H, N, A]`,
    `neglogp [H, N]`, `mu [H+1, N, A]`, `values [H+1, N]`, `rewards [H, N]`, `dones [H, N]`, `advantages`, `returns [H, N]`.
    `seed` goes to the sampling launch as given (policy.sample_actions): with the env's own seed the exploration draw of step t would be
    the env's action noise of step t + 1 for the same row and action.  Pass policy.sampler_stream_seed(user seed), as PPOTrainer does.

    action_delay, obs_delay: control latency in whole control steps, an int K or a (lo, hi) pair drawn anew per env at every episode start
    (latency.DelayLine; include/ppenv_train_delay.h, keyed by `latency_seed` — a STREAM seed, scene.stream_seed(seed, STREAM_LATENCY) —
    and `env_id_offset`).  The order is the Player's: obs_seen = obs_line.push(obs, done_prev), a = policy(obs_seen), a_applied =
    act_line.push(a, done_prev), env.step(a_applied).  With a sensing line (`obs_line`) the env step writes `raw_obs` [N, num_obs] and the
    line pushes it, with this step's dones, straight into obs[t + 1]; obs[0] of the first horizon is the initial observation pushed with no
    done, and the bootstrap forward reads the delayed obs[H].  With a command line (`act_line`) actions[t] — the policy's own clamped
    action, which the learner's ratio is evaluated on — is pushed into `applied` [N, A] with the done the previous env step returned
    (dones[t - 1]; at t = 0 the previous horizon's dones[H - 1], still in the buffer; before any step none), and the env consumes
    `applied`.  A path whose hi is 0 is not built — no allocation, no launch, the attribute is None — so the default collector is the
    collector without the feature.

    obs_noise, action_noise (an amplitude S, or a (lo, hi) range), obs_drop, action_drop (a probability, or a range): sensor noise and sample
    dropouts, the levels drawn anew per row at every episode start on the device (sensor.SensorLine with draw = 1; include/ppenv_sensor.h,
    keyed by `sensor_seed` — a STREAM seed, scene.stream_seed(seed, STREAM_SENSOR) — and `env_id_offset`; scene.sensor_draws predicts
    them).  sensor_columns: dict(obs_noise_columns=, obs_drop_columns=, action_noise_columns=, action_drop_columns=) of column specs
    (sensor.columns / sensor.hold_columns; `task` names the observation's column groups).  The order is the Player's: sensed =
    obs_sensor.push(obs, done_prev); seen = obs_line.push(sensed, ...); (history); a = policy(...); delayed = act_line.push(a, ...);
    a_applied = act_sensor.push(delayed, done_prev); env.step(a_applied).  With a sensing sensor line (`obs_sensor`) the env writes the
    clean `raw_obs`, which stays the `raw_obs` critic input, and the line's output goes to the next stage's input (`sensed_obs`) or, where
    it is the last stage, straight into obs[t + 1]: `out` is the caller's pointer, no copy.  The command line (`act_sensor`) writes
    `applied`; actions[t] stays the policy's own.  A path whose amplitude and dropout ranges are both (0, 0) is not built — no
    allocation, no launch, the attribute is None.

    serve: what keeps the env's serve override buffer — a serve.ServePlan or a curriculum.ServeCurriculum set on `env` — an object with
    step(t, rew_t, reset_t), called right after the env step of row t with rewards[t] (unscaled) and dones[t]: one launch, no copy.  A
    plan runs its apply(dones[t]); a curriculum also credits the games that ended and stages row t for the trainer's fold().  None (the
    default): no call.

    randomizer: what keeps the env's randomisation tables — a dr.ResetRandomizer (a reset-time plan) or an adr.AutoRandomizer — likewise an
    object with step(t, rew_t, reset_t), called right after serve.step with the same rows.  It is independent of `serve`: a serve
    curriculum and ADR can run together.  None (the default): no call.

    critic_input: source names (critic_input.NAMES: "tables", "latency", "raw_obs"; a tuple or the CLI's comma-separated text) of the
    privileged critic inputs of a num_priv > 0 network (include/ppenv_critic_input.h).  The collector then keeps `priv` [H+1, N, P] fp32 and
    every forward reads priv[t] beside obs[t].  Row t + 1 is gathered — one launch, straight into the slice — after the env step, the
    delay-line pushes and the serve / randomizer hooks of step t, so it shows the tables and delays the env will play step t + 1 with; row
    0 is gathered once at construction; next_horizon() carries row H to row 0.  None or empty (the default): nothing is allocated or
    launched, and `priv` and `critic_input` are None.

    history: an observation and action history for the policy's input (history.parse: (Ho, Ha), dict(obs=, actions=) or the CLI's text;
    include/ppenv_history.h).  `obs` is then [H+1, N, W], W = (Ho + 1) * num_obs + Ha * A, and `net` must have been built with num_obs = W.
    The env step writes a contiguous [N, num_obs] buffer — `cur_obs`, or with a sensing line `raw_obs` as before, the line's output then
    going to `seen_obs` [N, num_obs] — and one more launch builds obs[t + 1] from obs[t], that observation, actions[t] and dones[t]
    (history.HistoryStack.push), after the delay-line pushes and before the serve, randomizer and critic-input hooks.  Row 0 of the first
    horizon is pushed with no previous row: every env starts.  next_horizon() is unchanged, and the `raw_obs` critic input keeps width
    num_obs.  Not with a fuse_input network, whose layer 1 reads the env's observation in place.  None (the default): nothing is
    allocated or launched, and `history`, `cur_obs` and `seen_obs` are None."""

    def __init__(self, env, net, horizon=32, gamma=0.99, tau=0.95, reward_scale=0.01, sigma=None, seed=0, action_delay=0, obs_delay=0,
                 latency_seed=0, env_id_offset=0, serve=None, randomizer=None, critic_input=None, history=None, obs_noise=0.0, obs_drop=0.0, action_noise=0.0,
                 action_drop=0.0, sensor_columns=None, sensor_seed=0, task=None):
        self.action_delay, self.obs_delay = delay_range("action_delay", action_delay), delay_range("obs_delay", obs_delay)
        self.sensor_levels = dict(obs_noise=sensor_mod.sigma_range("obs_noise", obs_noise), obs_drop=sensor_mod.drop_range("obs_drop", obs_drop),
                                  action_noise=sensor_mod.sigma_range("action_noise", action_noise), action_drop=sensor_mod.drop_range("action_drop", action_drop))
        names = tuple(f"{axis}_columns" for axis in sensor_mod.AXES)
        unknown = [k for k in (sensor_columns or {}) if k not in names]
        if unknown:
            raise ValueError(f"sensor_columns: unknown key {unknown[0]!r}; the keys are {', '.join(names)}")
        self.sensor_columns = {k: (sensor_columns or {}).get(k) for k in names}
        self.env, self.net, self.h = env, net, int(horizon)
        self.gamma, self.tau, self.reward_scale, self.seed = float(gamma), float(tau), float(reward_scale), int(seed)   # yaml:55-59: scale_value 0.01, gamma 0.99, tau 0.95
        n, dev, a = env.num_rows, env.device, net.num_actions        # actor rows: A * N for the 4-actor variant
        z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
        num_obs = env.obs_buf.shape[1]
        self.history = self.cur_obs = self.seen_obs = None
        record = history_mod.parse(history, num_obs, a)
        if record is not None:
            if getattr(net, "fuse_input", False):
                raise ValueError("history: not with a fuse_input network, whose layer 1 reads the env's observation in place")
            if net.num_obs != record["width"]:
                raise ValueError(f"history: {record['obs']} observations + {record['actions']} actions back make rows of {record['width']} columns, but the "
                                 f"network was built with num_obs={net.num_obs}")
            self.history = history_mod.HistoryStack(n, num_obs, a, record["obs"], record["actions"], dev, env.num_agents)
        self.obs = z(self.h + 1, n, num_obs if record is None else record["width"])
        self.head = z(self.h + 1, n, a + 1)                     # mu | value, as the heads launch writes them
        self.mu, self.values = self.head[:, :, :a], self.head[:, :, a]
        self.actions, self.neglogp = z(self.h, n, a), z(self.h, n)
        self.rewards, self.dones = z(self.h, n), z(self.h, n, dt=torch.int64)
        self.advantages, self.returns = z(self.h, n), z(self.h, n)
        self.sigma = (torch.ones(a, device=dev) if sigma is None else sigma.to(dev, torch.float32)).contiguous()
        self.counter = 0
        self.serve = serve
        self.randomizer = randomizer
        self.on_step = None                   # called with no arguments right after every env.step of collect() (render.TrainingCapture.on_step)
        self.act_line = self.obs_line = self.applied = self.raw_obs = None
        self.obs_sensor = self.act_sensor = self.sensed_obs = self.delayed = None
        self._done_prev = None                # the dones of the last env step (a row of `dones`); None before any step
        line = lambda width, rng, channel: DelayLine(n, width, rng[0], rng[1], dev, env.num_agents, latency_seed, env_id_offset, channel)

        def sensor_line(path, width, channel):
            scale = sensor_mod.columns(task, self.sensor_columns[f"{path}_noise_columns"], width, channel, name=f"{path}_noise_columns")
            hold = sensor_mod.hold_columns(task, self.sensor_columns[f"{path}_drop_columns"], width, channel, name=f"{path}_drop_columns")
            sg, dp = self.sensor_levels[f"{path}_noise"], self.sensor_levels[f"{path}_drop"]
            if sg[1] == 0.0 and dp[1] == 0.0:
                return None
            return sensor_mod.SensorLine(n, width, dev, num_agents=env.num_agents, sigma=sg, drop=dp, columns=scale, hold_columns=hold, seed=sensor_seed,
                                         env_id_offset=env_id_offset, channel=channel)
        self.obs_sensor, self.act_sensor = sensor_line("obs", num_obs, sensor_mod.SENSING), sensor_line("action", a, sensor_mod.COMMAND)
        if self.action_delay[1] > 0:
            self.act_line = line(a, self.action_delay, COMMAND)
        if self.act_line is not None or self.act_sensor is not None:
            self.applied = z(n, a)
        if self.act_line is not None and self.act_sensor is not None:
            self.delayed = z(n, a)                              # the command line's output, the command sensor's input
        if self.obs_delay[1] > 0:
            self.obs_line = line(num_obs, self.obs_delay, SENSING)
        if self.obs_line is not None or self.obs_sensor is not None:
            self.raw_obs = z(n, num_obs)
            if self.obs_line is not None and self.history is not None:
                self.seen_obs = z(n, num_obs)
            if self.obs_sensor is not None and (self.obs_line is not None or self.history is not None):
                self.sensed_obs = z(n, num_obs)
        elif self.history is not None:
            self.cur_obs = z(n, num_obs)
        self._env_obs = self.raw_obs if self.raw_obs is not None else self.cur_obs      # where the env step writes; None: straight into obs[t + 1]
        (self.obs[0] if self._env_obs is None else self._env_obs).copy_(env.obs_buf)
        self._observe(0, None, None, None)
        self.critic_input = self.priv = None
        if critic_input:
            from .critic_input import CriticInput
            self.critic_input = CriticInput(env, self, critic_input)
            if self.critic_input.P != getattr(net, "num_priv", 0):
                raise ValueError(f"critic_input: {self.critic_input.P} privileged columns, but the network was built with num_priv={getattr(net, 'num_priv', 0)}")
            self.priv = z(self.h + 1, n, self.critic_input.P)
            self.critic_input.gather(self.priv[0])

    def _observe(self, row, done, prev, action):
        """The env's buffer (`_env_obs`) holds a new observation -> obs[row]: the sensing sensor's push, then the sensing line's, then the
        history's, where there is one; the last stage writes obs[row] itself.  done: the dones of the step that wrote it; prev, action:
        obs[row - 1] and the actions that step took.  All None for the first row.  With no stage the env wrote obs[row] itself and nothing
        is launched."""
        seen = self._env_obs
        if self.obs_sensor is not None:
            seen = self.obs_sensor.push(seen, done, self.obs[row] if self.sensed_obs is None else self.sensed_obs)
        if self.obs_line is not None:
            seen = self.obs_line.push(seen, done, self.obs[row] if self.history is None else self.seen_obs)
        if self.history is not None:
            self.history.push(seen, action, done, prev, self.obs[row])

    def _forward(self, t, **kw):
        if self.priv is None:
            return self.net.forward(self.obs[t], head_out=self.head[t], **kw)
        return self.net.forward(self.obs[t], head_out=self.head[t], priv=self.priv[t], **kw)

    @torch.no_grad()
    def collect(self):
        """One horizon.  Row 0 of `obs` is the observation the previous horizon ended on."""
        for t in range(self.h):
            self.counter += 1
            self._forward(t, sample=dict(actions=self.actions[t], sigma=self.sigma, seed=self.seed, counter=self.counter, neglogp=self.neglogp[t]))
            act = self.actions[t]
            if self.act_line is not None:
                act = self.act_line.push(act, self._done_prev, self.applied if self.act_sensor is None else self.delayed)
            if self.act_sensor is not None:
                act = self.act_sensor.push(act, self._done_prev, self.applied)
            self.env.step(act, obs=self.obs[t + 1] if self._env_obs is None else self._env_obs, rew=self.rewards[t], reset=self.dones[t])
            self._observe(t + 1, self.dones[t], self.obs[t], self.actions[t])
            if self.serve is not None:
                self.serve.step(t, self.rewards[t], self.dones[t])
            if self.randomizer is not None:
                self.randomizer.step(t, self.rewards[t], self.dones[t])
            if self.critic_input is not None:
                self.critic_input.gather(self.priv[t + 1])
            self._done_prev = self.dones[t]
            if self.on_step is not None:
                self.on_step()
        self._forward(self.h)                                                      # bootstrap value of the last observation
        gae(self.rewards, self.values, self.dones, self.gamma, self.tau, self.reward_scale, self.advantages, self.returns)
        return self

    def next_horizon(self):
        """Carry the last observation over as row 0 of the next horizon (one [N, num_obs] copy per horizon)."""
        self.obs[0].copy_(self.obs[self.h])
        if self.priv is not None:
            self.priv[0].copy_(self.priv[self.h])
