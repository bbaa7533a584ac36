"""The play loop: Player drives task.step under one policy (or one per cell) and the accounting objects after it."""
import math
import time

import numpy as np
import torch

from .. import scene, sensor
from .._lib import TAOutcome
from .accounting import ACT_THRESHOLDS, ActuatorStats, Delay, EpisodeStats, GroupStats, PairStats, _read_structs
from .report import actuator_summary, group_summary, outcomes_dict, pair_summary, sum_act_totals, sum_totals, summarize
from .sweep import SENSOR_AXES, baseline_cells, cell_delays, cell_sensors


def actuator_limits(task):
    """The joints' limits from the numbers the step kernels themselves run with -> (float32 [D, 4]: lower, upper, effort, vel_limit; the D
    joint names): the env's joint_limits() (scene.joint_limits, scene.ta_joint_limits)."""
    return task.env.joint_limits()


def control_dt_of(task):
    """Seconds per control step (the env's control_dt: controlFrequencyInv already folded in)."""
    return task.env.control_dt


class Player:
    """rl_games' BasePlayer.run on a task from isaacgym_amd.make(...) (any of the five registry names; the 4-actor task has two rows per
    env) under an RLGamesPolicy.  The defaults are rl_games' player defaults.
    sigma: train.py:214's override — the policy's log-std is filled with it, so sigma = exp(x) (rl_games' _override_sigma for a fixed
    sigma); it matters only with deterministic=False.
    outcomes: the 27-dof task's five head-counts (task.enable_outcomes(); the other tasks raise ValueError), zeroed by start() and latched
    on the device after every env step under the totals' freeze rule: run()'s `outcomes` are those of the step the totals stopped at,
    whatever poll_every is.
    sweep: a Sweep of G cells — the envs are split into G equal groups, group g plays under cell g's tables (start() hands
    sweep.tables(...) to task.env.set_randomization before the first reset, so every counted episode runs whole under its cell), and
    games_num is PER GROUP: each group freezes on its own.  run() ends at the first poll that finds every group frozen, returns the usual
    dict summed over the groups plus `groups` (one group_summary per cell, in cell order) and leaves the task as it found it: the
    randomisation cleared and the envs' episode counters (the RNG key of their serves) put back, so what is played on the task afterwards is
    what would have been played without the sweep.  Groups see different, identically distributed serves (the RNG is keyed by the global
    env id): compare cells by `reward_stderr`.
    A sweep with serve axes, or paired=True, also sets a serve plan (task.set_serve_plan) in start(), before the reset: episode m of env e
    since start() is serve(e, m) of the plan, and task.step launches the plan's apply after every env step; end_sweep() clears it.  With
    paired=True env i of every group is served the same sequence of balls — with no serve axis, from the configured ranges — so groups
    whose cells are equal are bitwise replicas of each other under deterministic play; `reward_stderr` stays the unpaired one, conservative
    for differences between paired cells; the sampler's exploration noise (deterministic=False) is keyed by row and is not paired.
    Refused with a sweep: a task with `randomize: True` (its tables are the sweep's) and
    outcomes=True (the 27-dof counts are cross-env windows and cannot be split by group).
    paired_diff: with a paired sweep, a PairStats (include/ppenv_play_pair.h) records the first pair_episodes episodes of EVERY env —
    default ceil(games_num / S), S the envs per cell — in one more launch per control step, and run() ends at the first poll at which every
    group is frozen AND every cell has all S * pair_episodes pairs (or at max_steps).  The group totals freeze on their own, so `groups`
    and the summed figures are byte for byte those of the run without paired_diff; only steps_played and seconds may grow.  The result
    gains `paired_diff` = dict(episodes, complete, cells=[pair_summary of cell g against cell baseline[g]]); baseline: one cell index for
    all cells, or one per cell.  A cell against itself gives diff 0.0 and diff_stderr 0.0.
    policy: one RLGamesPolicy, or a sequence of len(sweep) of them — cell g is then played by policy[g] on its rows
    [A * S * g, A * S * (g + 1)); consecutive cells holding the same object are forwarded in one act().  `policy` stays the first one,
    `policies` is the list; sigma is applied to each, start() zeroes each one's draw counter.  Under deterministic=False the exploration
    noise is keyed by row and by each policy's own counter: it is NOT paired, neither across cells nor across checkpoints.
    actuators: True, or a dict overriding some of the thresholds effort_frac 0.98, vel_frac 0.98, limit_margin 0.02 rad, action_clip = the
    task's clipActions — an ActuatorStats (include/ppenv_play_act.h) reads, after every env step and in two more launches, the env's own
    joint positions / velocities / drive torques and the policy's raw actions where they lie, and sums per joint and per cell how the
    return was earned: torque against the effort limit, speed against the velocity limit, position against the joint limits, mechanical
    energy per game.  It counts the same games under the same freeze as the totals.  The result gains `actuators` (read_actuators());
    every other key, `groups` included, is what it is without the option, and what is played does not change.
    action_delay, obs_delay: control latency in whole control steps (0 .. 15), for every env — or, with a sweep, for the cells that do not
    name the axis of that name.  Per control step: obs_seen = obs_line.push(obs, done_prev); a = policy.act(obs_seen); a_applied =
    act_line.push(a, done_prev); task.step(a_applied), done_prev being the done the previous task.step returned (None right after start()):
    the env consumes the command of action_delay steps ago and the policy sees the observation of obs_delay steps ago, both held at the
    episode's first sample until there is one that old, nothing carried across a reset (Delay; include/ppenv_play_delay.h).  A line whose
    delays are all zero is not built — no allocation, no launch — so the defaults are today's player byte for byte.  `actions` stays the
    policy's raw output (the actuator report's clip share reads it), `applied_actions` is what the env consumed, `policy_obs` what the
    policy saw.  The lines sit between the policy and the task and compose with everything above, a `randomize: True` task included.  With
    a line in use the result gains `latency` = dict(control_dt, action_delay=[per cell], obs_delay=[per cell]).
    obs_noise, action_noise (an amplitude >= 0), obs_drop, action_drop (a probability 0 .. 1): sensor noise and sample dropouts, for every
    env — or, with a sweep, for the cells that do not name the axis of that name (SENSOR_AXES).  Two sensor lines (sensor.SensorLine;
    include/ppenv_sensor.h) sit beside the delay lines, the sensing one BEFORE the delay and the command one AFTER it:
    sensed = obs_sensor.push(obs, done_prev); seen = obs_line.push(sensed, ...); (history); a = policy.act(...); delayed =
    act_line.push(a, ...); a_applied = act_sensor.push(delayed, done_prev); task.step(a_applied) — the env's own clamp still applies.
    Row r of a line adds level[r] * col_scale[c] * N(0, 1) to column c and, with probability drop[r] per control step (never on an episode's
    first sample), delivers in its hold columns what it delivered last; the draws are keyed (seed, env, episode, step).  *_noise_columns
    gives col_scale and *_drop_columns the hold columns, as sensor.columns / sensor.hold_columns parse them ("ball_pos=1,ball_vel=4,60:67=0.5";
    default every column, scale 1; the command path takes `all` and ranges).  With sweep.paired the lines get key_period = the envs per
    cell: env i of every cell sees the same standard normals and the same drop draws, so cells of equal values stay bitwise replicas.  A
    line whose amplitudes and dropout probabilities are all zero is not built — no allocation, no launch — so the defaults are the player
    without the feature byte for byte.  `policy_obs` / `applied_actions` keep their meaning: what the policy saw, what the env consumed.
    With a line in use the result gains `sensor` = dict(obs_noise=[per cell], obs_drop=[...], action_noise=[...], action_drop=[...],
    columns={the four specs}).  The levels are fixed per cell: a policy trained under per-episode drawn levels is evaluated on a grid.
    A policy with an observation and action history (policy.history: the checkpoint decides, there is no argument here; include/
    ppenv_history.h) is accepted when its base_num_obs is the task's num_obs and its network is history["width"] wide.  The player then
    keeps one history.HistoryStack per distinct record over ALL rows, and per control step: seen = obs_line.push(...) or the raw obs;
    wide = stack.advance(seen, the policy output of the previous step, done_prev); act on wide.  start() resets the stacks, so the first
    push starts every row.  With per-cell policies each run of cells reads its own record's rows of `wide`, or `seen` — a history
    checkpoint plays A/B against one without.  `policy_obs` stays what the policy saw: with mixed records, the widest.  The result gains
    `history`, the record (or None) of each distinct policy.  Without such a policy nothing is built and the player is today's byte for byte.
    Without a sweep the player is ONE cell, `{}`, over all envs — the actuators, the delays and the result are assembled over `_cells`
    either way — but it is not a one-cell Sweep: its `stats` is an EpisodeStats (the outcome latch needs its one struct), its totals are
    that struct's own, and start() / end_sweep() leave the task's randomisation and serve plan alone."""

    def __init__(self, task, policy, games_num=2000, deterministic=True, seed=0, poll_every=64, max_steps=108000, sigma=None, recorder=None,
                 outcomes=False, sweep=None, paired_diff=False, baseline=0, pair_episodes=None, actuators=False, action_delay=0, obs_delay=0,
                 obs_noise=0.0, obs_drop=0.0, action_noise=0.0, action_drop=0.0, obs_noise_columns=None, obs_drop_columns=None, action_noise_columns=None,
                 action_drop_columns=None):
        for name, v in (("games_num", games_num), ("poll_every", poll_every), ("max_steps", max_steps)):
            if int(v) != v or int(v) < 1:
                raise ValueError(f"{name}: {v!r} is not a positive integer")
        if sweep is not None:
            if outcomes:
                raise ValueError("outcomes=True with a sweep: the 27-dof outcome counts are cross-env reset windows and cannot be split by group")
            if task.randomize:
                raise ValueError("a sweep on a task with randomize: True: the sweep sets the task's randomisation tables itself; set task.randomize=False")
        per_cell = isinstance(policy, (list, tuple))
        if per_cell and (sweep is None or len(policy) != len(sweep)):
            raise ValueError("a sequence of policies is one policy per cell of a sweep: " +
                             ("there is no sweep" if sweep is None else f"the sweep has {len(sweep)} cells, the sequence {len(policy)} policies"))
        if paired_diff:
            if sweep is None or not sweep.paired:
                raise ValueError("paired_diff=True needs a sweep with paired=True: without common serves, episode m of env i is a different ball in every cell")
            self._baseline = baseline_cells(baseline, len(sweep))
            if pair_episodes is not None and (int(pair_episodes) != pair_episodes or int(pair_episodes) < 1):
                raise ValueError(f"pair_episodes: {pair_episodes!r} is not a positive integer")
        self.policies = list(policy) if per_cell else [policy]
        rl, sim = torch.device(task.rl_device), torch.device(task.device)
        if rl != sim or sim.type != "cuda":
            raise ValueError(f"Player needs rl_device == sim_device on a GPU (no per-step copies): rl_device is {rl}, sim_device is {sim}")
        for p in self.policies:
            if torch.device(p.device) != sim:
                raise ValueError(f"the policy lives on {p.device}, the task on {sim}")
            hist = getattr(p, "history", None)
            if getattr(p, "base_num_obs", p.net.num_obs) != task.num_obs or p.net.num_actions != task.num_actions or \
                    p.net.num_obs != (task.num_obs if hist is None else hist["width"]):
                raise ValueError(f"the policy maps {getattr(p, 'base_num_obs', p.net.num_obs)} observations to {p.net.num_actions} actions, the task has "
                                 f"{task.num_obs} and {task.num_actions}" + ("" if hist is None else f" (history {hist}: a network of {p.net.num_obs} columns)"))
        self.task, self.policy = task, self.policies[0]
        self.games_num, self.poll_every, self.max_steps = int(games_num), int(poll_every), int(max_steps)
        self.deterministic, self.seed = bool(deterministic), int(seed)
        self.num_agents = A = int(task.num_agents)
        self._distinct = list({id(p): p for p in self.policies}.values())
        if sigma is not None:
            for p in self._distinct:
                p.sigma.fill_(math.exp(float(sigma)))
        self.sweep = sweep
        self._cells = sweep.cells if sweep is not None else [{}]
        self._tables = self._episode0 = self._serve_cells = None
        if sweep is not None:
            self._tables = sweep.tables(task.env.DR_TABLE_ROWS, task.num_envs)     # (refuses a number of envs that is no multiple of the cells)
            if sweep.needs_serve_plan:
                self._serve_cells = sweep.serve_cells(task.env.serve_defaults())
        G = len(self._cells)
        S = task.num_envs // G                                                 # group g is envs [g * S, (g + 1) * S), rows [A * S * g, A * S * (g + 1))
        self.stats = EpisodeStats(S, A, self.games_num, sim) if sweep is None else GroupStats(S, G, A, self.games_num, sim)
        self.pairs = None
        if paired_diff:
            self.pair_episodes = int(pair_episodes) if pair_episodes is not None else -(-self.games_num // S)
            self.pairs = PairStats(S, G, A, self.pair_episodes, self._baseline, sim)
        self.act = None
        if actuators:
            if actuators is not True and not isinstance(actuators, dict):
                raise ValueError(f"actuators: True, or a dict of thresholds ({', '.join(ACT_THRESHOLDS)}, action_clip), not {actuators!r}")
            thr = dict(ACT_THRESHOLDS, action_clip=float(task.clip_actions))
            given = actuators if isinstance(actuators, dict) else {}
            unknown = [k for k in given if k not in thr]
            if unknown:
                raise ValueError(f"actuators: unknown threshold {unknown[0]!r}; the thresholds are {', '.join(thr)}")
            thr.update({k: float(v) for k, v in given.items()})
            self._act_limits, self._act_names = actuator_limits(task)
            self.act = ActuatorStats(S, G, len(self._act_names), self.games_num, self._act_limits, thr, sim, num_agents=A)
            self._act_inputs = task.env.joint_views()                     # the 27-dof AoS tensors, the 7-dof SoA planes: [N, D] views
        self._cell_delays = cell_delays(self._cells, action_delay, obs_delay)
        per_row = {axis: np.repeat(np.asarray(per, np.int32), A * S) for axis, per in self._cell_delays.items()}
        rows = A * S * G
        # a line whose delays are all zero is not built: that path is the player without the feature
        self._act_line = Delay(rows, task.num_actions, per_row["action_delay"], sim, A) if per_row["action_delay"].any() else None
        self._obs_line = Delay(rows, task.num_obs, per_row["obs_delay"], sim, A) if per_row["obs_delay"].any() else None
        # a sensor line whose amplitude and dropout tables are all zero is not built either
        self._cell_sensors = cell_sensors(self._cells, obs_noise, obs_drop, action_noise, action_drop)
        self._sensor_columns = dict(obs_noise_columns=obs_noise_columns, obs_drop_columns=obs_drop_columns, action_noise_columns=action_noise_columns,
                                    action_drop_columns=action_drop_columns)
        self.sensor_seed = scene.stream_seed(self.seed, scene.STREAM_SENSOR)
        self._obs_sensor, self._act_sensor = (self._sensor_line(path, width, channel, A * S, S if sweep is not None and sweep.paired else 0)
                                              for path, width, channel in (("obs", task.num_obs, sensor.SENSING), ("action", task.num_actions, sensor.COMMAND)))
        self._done_prev = None
        # one stack per distinct history record, each over all rows: a policy without a history builds none
        self._stacks, self._wide = {}, {}
        for p in self.policies:
            hist = getattr(p, "history", None)
            if hist is not None and self._key(p) not in self._stacks:
                from ..history import HistoryStack
                self._stacks[self._key(p)] = HistoryStack(rows, task.num_obs, task.num_actions, hist["obs"], hist["actions"], sim, A)
        self._runs = self._cell_actions = None
        if per_cell:                                                     # runs of consecutive cells that hold the same object: (policy, first row, end row)
            w, runs = A * S, []
            for g, p in enumerate(self.policies):
                if runs and runs[-1][0] is p:
                    runs[-1][2] = w * (g + 1)
                else:
                    runs.append([p, w * g, w * (g + 1)])
            self._runs = [tuple(r) for r in runs]
        if recorder is not None and recorder.renderer.task is not task:
            raise ValueError("the recorder renders another task")
        self.recorder = recorder
        self.outcome = self._latched = None
        if outcomes:
            self.outcome = task.enable_outcomes()
            self._latched = torch.zeros_like(self.outcome)
        self.steps_played = 0
        self.actions = self.applied_actions = self.policy_obs = None
        self._obs = None

    def _sensor_line(self, path, width, channel, rows_per_cell, key_period):
        """The sensor line of one path ("obs" or "action") over all rows, or None where every cell's amplitude and dropout are zero.  The
        column specs are parsed either way: a bad one is refused whether or not it is used."""
        scale = sensor.columns(self.task, self._sensor_columns[f"{path}_noise_columns"], width, channel, name=f"{path}_noise_columns")
        hold = sensor.hold_columns(self.task, self._sensor_columns[f"{path}_drop_columns"], width, channel, name=f"{path}_drop_columns")
        sigma, drop = (np.repeat(np.asarray(self._cell_sensors[f"{path}_{kind}"], np.float32), rows_per_cell) for kind in ("noise", "drop"))
        if not sigma.any() and not drop.any():
            return None
        return sensor.SensorLine(sigma.size, width, torch.device(self.task.device), num_agents=self.num_agents, sigma=sigma, drop=drop, columns=scale,
                                 hold_columns=hold, seed=self.sensor_seed, key_period=key_period, channel=channel)

    def sensors(self):
        """run()'s `sensor`: per cell (one entry without a sweep) the four levels, and the four column specs as given."""
        return dict(**{axis: list(per) for axis, per in self._cell_sensors.items()}, columns=dict(self._sensor_columns))

    @staticmethod
    def _key(policy):
        """Which stack a policy reads: (Ho, Ha), or None for the plain observation."""
        hist = getattr(policy, "history", None)
        return None if hist is None else (hist["obs"], hist["actions"])

    def history(self):
        """run()'s `history`: the record of each distinct policy, None for one without."""
        return [None if getattr(p, "history", None) is None else dict(p.history) for p in self._distinct]

    def end_sweep(self):
        """The task as the sweep found it: the plain step kernel (clear_randomization), no serve plan, and the episode counters of before
        start().  run() calls it at its end, also on an exception; a caller that drives start() / step() itself calls it when done."""
        if self.sweep is None:
            return
        self.task.env.clear_randomization()
        if self._serve_cells is not None:
            self.task.clear_serve_plan()
        if self._episode0 is not None:
            self.task.env.episode.copy_(self._episode0)
            self._episode0 = None
        self._obs = None

    def start(self):
        """Every env to the start of an episode, the accounting to zero, the action-draw counter to zero (a run is a function of the seed)."""
        if self.sweep is not None:
            if self._episode0 is None:
                self._episode0 = self.task.env.episode.clone()
            if self.sweep.sets_randomization:
                self.task.env.set_randomization(**self._tables)       # before the reset: the first counted episode is already the cell's
            if self._serve_cells is not None:                         # fill = serve 0; the reset below consumes it and leaves count 1
                self.task.set_serve_plan(self._serve_cells, paired=self.sweep.paired)
        self.task.reset_idx()
        self.stats.reset()
        if self.outcome is not None:
            self.outcome.zero_()
            self._latched.zero_()
        if self.pairs is not None:
            self.pairs.reset()
        if self.act is not None:
            self.act.reset()
        for line in (self._act_line, self._obs_line, self._obs_sensor, self._act_sensor):
            if line is not None:
                line.reset()
        for stack in self._stacks.values():
            stack.reset()
        self._done_prev = None
        for p in self._distinct:
            p._counter = 0
        self._obs = self.task.reset()["obs"]
        self.steps_played = 0

    def _act_per_cell(self, obs):
        """Every run of cells under its own policy, into ONE [rows, num_actions] tensor: a policy owns its output buffer and may serve
        several runs, so each result is copied out before the next act().  A policy with a history reads its record's wide rows."""
        if self._cell_actions is None:
            self._cell_actions = torch.empty((obs.shape[0], self.task.num_actions), dtype=torch.float32, device=obs.device)
        for p, r0, r1 in self._runs:
            x = obs if self._key(p) is None else self._wide[self._key(p)]
            a, _ = p.act(x[r0:r1], deterministic=self.deterministic, seed=self.seed)
            self._cell_actions[r0:r1].copy_(a)
        return self._cell_actions

    def step(self):
        """One control step: (obs sensor -> obs line ->) policy (-> action line -> action sensor) -> task.step -> accumulate (-> record, with
        paired_diff).  No host read."""
        if self._obs is None:
            self.start()
        sensed = self._obs if self._obs_sensor is None else self._obs_sensor.push(self._obs, self._done_prev)
        seen = sensed if self._obs_line is None else self._obs_line.push(sensed, self._done_prev)
        self.policy_obs = seen
        if self._stacks:                                                  # self.actions: the policies' output of the previous step, not read on a start
            self._wide = {k: stack.advance(seen, self.actions, self._done_prev) for k, stack in self._stacks.items()}
            self.policy_obs = max(self._wide.values(), key=lambda w: w.shape[1])      # with mixed records: the widest (any is wider than `seen`)
        if self._runs is None:
            self.actions, _ = self.policy.act(self.policy_obs, deterministic=self.deterministic, seed=self.seed)
        else:
            self.actions = self._act_per_cell(seen)
        self.applied_actions = self.actions if self._act_line is None else self._act_line.push(self.actions, self._done_prev)
        if self._act_sensor is not None:
            self.applied_actions = self._act_sensor.push(self.applied_actions, self._done_prev)
        obs, rew, done, _ = self.task.step(self.applied_actions)
        self._done_prev = done
        if self.outcome is not None:
            self.stats.latch_outcome(self.outcome, self._latched)
        self.stats.accumulate(rew, done)
        if self.pairs is not None:
            self.pairs.record(rew, done)
        if self.act is not None:                                          # the env's own tensors and the policy's own output: no copy, no refresh
            self.act.accumulate(*self._act_inputs, self.actions, done)
        if self.recorder is not None:
            self.recorder.capture()
        self._obs = obs["obs"]
        self.steps_played += 1

    def read_outcomes(self):
        """One host copy of the LATCHED outcome struct -> outcomes_dict (None with outcomes off)."""
        if self._latched is None:
            return None
        return outcomes_dict(_read_structs(TAOutcome, self._latched, 1)[0])

    def read_actuators(self):
        """One host copy of the actuator totals -> run()'s `actuators`: dict(thresholds, joints = the names, control_dt, total =
        actuator_summary of every group summed, groups = one actuator_summary per cell with its `cell`); None with actuators off."""
        if self.act is None:
            return None
        per, dt = self.act.read(), control_dt_of(self.task)
        return dict(thresholds=dict(self.act.thresholds), joints=list(self._act_names), control_dt=dt,
                    total=actuator_summary(sum_act_totals(per), self._act_limits, self._act_names, dt),
                    groups=[dict(cell=dict(c), **actuator_summary(t, self._act_limits, self._act_names, dt)) for c, t in zip(self._cells, per)])

    def latency(self):
        """run()'s `latency`: the control dt in seconds and, per cell (one entry without a sweep), the two delays in control steps."""
        return dict(control_dt=control_dt_of(self.task), **{axis: list(per) for axis, per in self._cell_delays.items()})

    def run(self, on_poll=None):
        """Play until games_num games are counted (seen at a poll) or max_steps control steps.  on_poll(totals dict): called after every
        host read.  -> dict(games, av_reward, av_steps, reward_std, reward_min, reward_max, per_agent=[...], steps_played, seconds); with
        outcomes=True also `outcomes` (outcomes_dict of the latched struct).  With a sweep: until EVERY group has counted games_num games;
        on_poll gets the groups' totals summed (sum_totals), the result is summarize() of that sum plus `groups`.  With paired_diff:
        until also every cell has all its pairs; the result gains `paired_diff`."""
        try:
            self.start()
            t0 = time.perf_counter()
            full = self.pairs.envs_per_group * self.pairs.episodes if self.pairs is not None else 0
            while True:
                self.step()
                last = self.steps_played >= self.max_steps
                if last or self.steps_played % self.poll_every == 0:
                    per = self.stats.read_groups()
                    tot = per[0] if self.sweep is None else sum_totals(per)      # (not sum_totals of the one group: 0.0 + -0.0 is +0.0)
                    if on_poll is not None:
                        on_poll(tot)
                    frozen = all(t["games"] >= self.games_num for t in per)
                    if self.pairs is not None and (last or frozen):      # the reduce is idempotent: launched only where the answer is needed
                        pairs = self.pairs.read()
                        frozen = frozen and all(p["pairs"] == full for p in pairs)
                    if last or frozen:
                        break
            out = summarize(tot, self.num_agents)
            out.update(steps_played=self.steps_played, seconds=time.perf_counter() - t0)
            if self.sweep is not None:
                out["groups"] = [group_summary(cell, t, self.num_agents, self.games_num, self.sweep.paired) for cell, t in zip(self._cells, per)]
            if self.pairs is not None:
                out["paired_diff"] = dict(episodes=self.pair_episodes, complete=all(p["pairs"] == full for p in pairs),
                                          cells=[pair_summary(p["cell"], p["baseline"], p, self.num_agents) for p in pairs])
            if self.outcome is not None:
                out["outcomes"] = self.read_outcomes()
            if self.recorder is not None:
                out["captured_frames"] = self.recorder.captured
            if self.act is not None:
                out["actuators"] = self.read_actuators()
            if self._act_line is not None or self._obs_line is not None:
                out["latency"] = self.latency()
            if self._obs_sensor is not None or self._act_sensor is not None:
                out["sensor"] = self.sensors()
            if self._stacks:
                out["history"] = self.history()
            return out
        finally:
            self.end_sweep()
