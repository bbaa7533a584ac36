"""Play a checkpoint: the reference's `test=true` (train.py:210-215: `runner.run({'train': not cfg.test, 'play': cfg.test, 'checkpoint': ...,
'sigma': ...})`), on the native env and network, with the episode accounting on the device (C ABI: include/ppenv_play.h).

    Player(task, policy, games_num=2000).run()      games_num episodes of `task` under `policy` -> rl_games' numbers (average return,
                                                    average episode length) plus spread
    python -m isaacgym_amd.play --task ... --checkpoint runs/.../nn/<task>.pth [--capture out.gif --capture-envs 0,1 --capture-samples 2 --camera side --capture-deferred --capture-trajectory out.npz]
    python -m isaacgym_amd.play ... --sweep link_mass_scale=0.7:1.3:4 --sweep friction_scale=0.5,1.0 [--sweep-out cells.json]      one pass over the grid
    python -m isaacgym_amd.play ... --sweep serve_speed=7.5:9:4 --sweep friction_scale=0.5,1.0 --paired                            serves swept too, every cell playing the same balls
    python -m isaacgym_amd.play ... --sweep friction_scale=0.5,1.0 --paired --paired-diff --baseline 1 [--paired-out diff.json]    every cell minus cell 1, on the same balls
    python -m isaacgym_amd.play ... --against other.pth [--against third.pth] [--sweep friction_scale=0.5,1.0]                     checkpoints A/B on the same balls

    python -m isaacgym_amd.play ... --actuators --sweep link_mass_scale=0.7:1.3:3 [--actuators-out act.json]                       per cell, a per-joint table: torque, speed, limits, energy
    python -m isaacgym_amd.play ... --sweep action_delay=0,1,2,3 --paired --paired-diff --baseline 0 [--obs-delay 1]                  the return lost per control step of command latency

Semantics.  Restated from rl_games' published BasePlayer.run (rl_games is absent offline: parity unpinned, the same status as ppo.py):
per row a running return `cr += r` (fp32, the unscaled reward) and a running length; the rows whose `done` is set are finished games
(`all_done_indices[::num_agents]`: an env of the two-agent task counts once, on agent 0's row), their returns and lengths go into the
sums and the running values restart at zero; the loop ends after the step in which games_played >= games_num, every env that finished
in that step counted.  `av_reward` is agent 0's, as in rl_games.

rl_games reads `done.nonzero()` on the host every step.  Here `EpisodeStats.accumulate` does the accounting in two small launches per
control step and the host reads one 72-byte struct every `poll_every` steps, only to decide when to stop.  The result does not depend
on `poll_every`: once games_num games are counted the kernel changes nothing (the freeze, include/ppenv_play.h), so the totals are
those of the step at which the host-synchronised loop would have stopped.

The player drives `task.step(actions)` — the VecTask surface rl_games' player drives — so action clamping, clipObservations,
controlFrequencyInv and both domain-randomisation modes behave as for any caller; a task with `randomize: True` plays under its
randomisation (evaluation; PPOTrainer's refusal of such a task is about training below that surface and is untouched).

Sweeps.  `Player(task, policy, sweep=Sweep.grid({"link_mass_scale": [0.7, 1.3], "friction_scale": [0.5, 1.0]}))` plays the checkpoint under
every cell of a grid of physical-parameter scales in ONE pass: the envs are split into G equal groups (group g is envs [g * S, (g + 1) * S)),
each group runs whole episodes under its cell's per-env tables (the domain-randomisation tables of dr.Randomizable.set_randomization, set before
the first reset), and `GroupStats` keeps one totals struct and one freeze per group in the same two launches per control step, whatever G
is (include/ppenv_play_group.h; `EpisodeStats` is its one-group case, and `Player.run` is one loop over the per-group totals).  Unpaired
groups see DIFFERENT serves that are identically distributed — the env RNG is keyed by the global env id — which is why every group
reports `reward_stderr` = reward_std / sqrt(games): two cells differ when their averages differ by more than a few standard errors, not
when they differ at all.

Serve sweeps and paired groups.  The axes `serve_speed`, `serve_tilt`, `serve_tilt_z` (degrees) and, on the 27-dof task, `ball_y`, `ball_z`
sweep what the task is about — the served ball: a value is a number (pinned) or, in the Python API, a `(lo, hi)` range; what a cell does not
name is the task's configured range.  They ride on a SERVE PLAN (include/ppenv_serve.h; VecTask.set_serve_plan): start() sets it before the
first reset, so episode m of env e since start() is serve(e, m) of the plan's own random stream, and one more small launch per control step
keeps every env's next serve on the device.  `Sweep(..., paired=True)` / `--paired` keys those draws by the env's index WITHIN its group:
env i of every group is served the same sequence of balls (common random numbers), the serve noise two cells share cancels in their
difference, and groups whose cells are equal are bitwise replicas of each other under deterministic play.  `reward_stderr` stays the
unpaired one, so it is conservative for differences between paired cells.  The sampler's exploration noise (`--stochastic`) is keyed by
row and is not paired.

Paired differences and checkpoint A/B.  `Player(..., sweep=Sweep(..., paired=True), paired_diff=True, baseline=0)` records the return of
the first M episodes of every env on the device (include/ppenv_play_pair.h) and reports, per cell, the mean of
return(cell, env i, episode m) - return(baseline, env i, episode m) over the pairs (i, m) with ITS OWN standard error — the error bar
pairing was built to shrink.  `policy` may be a sequence, one policy per cell: two checkpoints play the same balls in one run
(`--against other.pth`), the cells being checkpoints x sweep cells and the baseline of each the same physics under `--checkpoint`.

Actuator usage.  `Player(..., actuators=True)` / `--actuators` answers how the return is earned on the robot: per joint and per cell the mean,
rms and peak drive torque against the effort limit, the peak speed against the velocity limit, the share of samples at a position limit,
the mechanical energy of a game (the reward's power term sum |tau * qd|, times the control dt) and the share of raw actions at clipActions.
`ActuatorStats` (include/ppenv_play_act.h) reads the env's own joint tensors and the policy's own action tensor where they lie — the 7-dof
SoA planes, the 27-dof AoS rows — in two launches per control step, under the totals' freeze; an env that has just finished is not
sampled (its tensors already hold the next episode's reset state), so a game of L steps gives L - 1 samples.

Control latency.  `Player(..., action_delay=K, obs_delay=K)` / `--action-delay`, `--obs-delay` and the sweep axes `action_delay`, `obs_delay`
(whole control steps, 0 .. 15) put a delay line between the policy and the task: per control step obs_seen = obs_line.push(obs, done_prev),
a = policy.act(obs_seen), a_applied = act_line.push(a, done_prev), task.step(a_applied).  `Delay` (include/ppenv_play_delay.h, which carries
the rule in full — this build's own specification: the reference delays nothing and no oracle pins it) is a per-row ring on the device, one
launch per push: from sample d of an episode on every output is exactly d control steps old, before that the episode's first sample is held
(no artificial neutral command), and nothing is carried across a reset.  A line whose delays are all zero is not built, so the defaults are
the player without the feature byte for byte.  The result gains `latency` = dict(control_dt, action_delay=[per cell], obs_delay=[per cell]).

Out of scope: latency during training (the trainer and its collector are untouched), delays drawn per episode, action hold / policy decimation,
per-cell observation or action noise, a VecTask-level latency setting; sweeping noise amplitudes or gravity (one by-value constant per simulation: several passes), per-group outcome counts,
paired sampler noise, anything in the trainer; capturing the play loop in a HIP graph (VecTask.step cannot be captured); multi-rank play; the rl_games
`Runner` / `player_factory` shim (rl_games itself is absent); mp4 output (a run is captured to GIF / PNG / npy: `Player(recorder=...)`,
`--capture`, isaacgym_amd.render); the observer, PBT and W&B hooks.
"""
import argparse
import ctypes as C
import itertools
import json
import math
import re
import time

import numpy as np
import torch

from . import _lib, serve
from ._lib import MAX_AGENTS, PlayTotals     # PPENV_PLAY_MAX_AGENTS and the ctypes mirror of ppenv_play_totals (bound in _lib.load)
from ._lib import PlayPairTotals             # ... and of pp_play_pair_totals
from ._lib import TA_OUTCOME_NAMES, TAOutcome
from .dr import TABLE_NAMES

# the reference's five prints (TA:1164-1168), in its order and wording
OUTCOME_PRINTS = (("fall_down", "the sum of the huamnoid which fall down:"), ("closer", "the sum of the envs which are closer to the paddle:"),
                  ("hit_paddle", "the sum of the envs which hit the paddle:"), ("cross_net", "the sum of the envs which cross the net:"),
                  ("hit_table", "the sum of the envs which hit the table:"))


def outcomes_dict(t):
    """A host copy of pp_ta_outcome (TAOutcome) -> dict(windows, envs, the five counts by name, <name>_rate = count / envs — None while
    no window was counted — and last_envs, last_<name>: the most recent window alone)."""
    envs = int(t.envs)
    out = dict(windows=int(t.windows), envs=envs, last_envs=int(t.last_envs))
    for k, name in enumerate(TA_OUTCOME_NAMES):
        out[name] = int(t.count[k])
        out[f"{name}_rate"] = int(t.count[k]) / envs if envs > 0 else None
        out[f"last_{name}"] = int(t.last[k])
    return out


def outcome_lines(o):
    """The reference's five lines for an outcomes dict, as rates of the envs over all windows."""
    return [f"{text} {o[name + '_rate']} of the envs ({o[name]} / {o['envs']} in {o['windows']} windows)" for name, text in OUTCOME_PRINTS]


def totals_dict(t, num_agents=MAX_AGENTS):
    """PlayTotals -> a Python dict (the per-agent fields as lists of num_agents)."""
    return dict(games=int(t.games), steps=int(t.steps), launches=int(t.launches), reward=list(t.reward)[:num_agents],
                reward_sq=list(t.reward_sq)[:num_agents], reward_min=list(t.reward_min)[:num_agents], reward_max=list(t.reward_max)[:num_agents])


def summarize(totals, num_agents=1):
    """The result-dict arithmetic from a totals dict (EpisodeStats.read()): rl_games' av reward = sum_rewards / games_played (agent 0's)
    and av steps = sum_steps / games_played, plus the population standard deviation sqrt(max(E[x^2] - E[x]^2, 0)), minimum and maximum of
    the games' returns; `per_agent`: the four reward figures for each agent.  With no game counted the averages are nan."""
    g = int(totals["games"])
    per_agent = []
    for a in range(num_agents):
        if g > 0:
            mean = totals["reward"][a] / g
            std = math.sqrt(max(totals["reward_sq"][a] / g - mean * mean, 0.0))
        else:
            mean = std = float("nan")
        per_agent.append(dict(av_reward=mean, reward_std=std, reward_min=float(totals["reward_min"][a]), reward_max=float(totals["reward_max"][a])))
    out = dict(games=g, av_steps=totals["steps"] / g if g > 0 else float("nan"))
    out.update(per_agent[0])
    out["per_agent"] = per_agent
    return out


MAX_GROUPS = 1024                          # PP_PLAY_GROUP_MAX


class GroupStats:
    """pp_play_group_accumulate / pp_play_group_reset (include/ppenv_play_group.h) on torch tensors: `groups` populations of
    `envs_per_group` envs, group g being envs [g * S, (g + 1) * S) of the task, each with its own totals struct and its own freeze at
    games_num; `cur_reward` [num_envs * num_agents] f32, `cur_steps` [num_envs] i32 and the `groups` totals structs, all on `device`; two
    launches per accumulate whatever the group count.  Group g's totals and its slices of cur_reward / cur_steps are byte for byte those of
    an EpisodeStats(envs_per_group, num_agents, games_num) fed the group's slices.  Nothing here synchronises except read()."""

    def __init__(self, envs_per_group, groups, num_agents, games_num, device):
        self.envs_per_group, self.groups, self.num_agents, self.games_num = int(envs_per_group), int(groups), int(num_agents), int(games_num)
        if self.envs_per_group < 1 or not 1 <= self.groups <= MAX_GROUPS or self.num_agents not in (1, 2) or self.games_num < 1 or \
                self.envs_per_group * self.groups * self.num_agents > 2 ** 31 - 1:
            raise ValueError(f"{type(self).__name__}: envs_per_group {envs_per_group} (>= 1), groups {groups} (1..{MAX_GROUPS}), num_agents {num_agents} "
                             f"(1 or 2), games_num {games_num} (>= 1), at most 2^31 - 1 rows")
        self.device = torch.device(device)
        self.num_envs = self.envs_per_group * self.groups
        self.rows = self.num_envs * self.num_agents
        L = self.L = _lib.lib()
        dev = self.device
        self.cur_reward = torch.zeros(self.rows, dtype=torch.float32, device=dev)
        self.cur_steps = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self._totals = torch.zeros(self.groups * C.sizeof(PlayTotals), dtype=torch.uint8, device=dev)
        self._partial = torch.zeros(int(L.pp_play_group_partial_bytes(self.envs_per_group, self.groups)), dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        _lib.check(self.L.pp_play_group_reset(self.envs_per_group, self.groups, self.num_agents, self.cur_reward.data_ptr(), self.cur_steps.data_ptr(),
                                              self._totals.data_ptr(), _lib.stream(self.device)), self.L)

    def accumulate(self, rew, done):
        """One control step of every group, after the env step: rew [rows] f32, done [rows] int64 (VecTask.step's rew_buf / reset_buf — all
        groups' rows, in env order — or a [rows] slice of larger buffers), contiguous, on this device.  Two launches, no synchronisation."""
        if rew.dtype != torch.float32 or done.dtype != torch.int64 or rew.numel() != self.rows or done.numel() != self.rows or \
                not rew.is_contiguous() or not done.is_contiguous() or rew.device != self.device or done.device != self.device:
            raise ValueError(f"{type(self).__name__}.accumulate: rew must be float32 and done int64, contiguous [{self.rows}] on {self.device}")
        _lib.check(self.L.pp_play_group_accumulate(rew.data_ptr(), done.data_ptr(), self.envs_per_group, self.groups, self.num_agents, self.games_num,
                                                   self.cur_reward.data_ptr(), self.cur_steps.data_ptr(), self._totals.data_ptr(),
                                                   self._partial.data_ptr(), _lib.stream(self.device)), self.L)

    def read_groups(self):
        """One host copy of the `groups` structs (groups x 72 bytes; the stream is waited for) -> a list of totals_dict, in group order."""
        raw, n = self._totals.cpu().numpy().tobytes(), C.sizeof(PlayTotals)
        return [totals_dict(PlayTotals.from_buffer_copy(raw[g * n:(g + 1) * n]), self.num_agents) for g in range(self.groups)]

    read = read_groups

    def state_bytes(self):
        """cur_reward, cur_steps and the `groups` totals structs as host bytes (the tests compare them)."""
        return self.cur_reward.cpu().numpy().tobytes(), self.cur_steps.cpu().numpy().tobytes(), self._totals.cpu().numpy().tobytes()

    def group_state_bytes(self, g):
        """Group g's part of state_bytes(): what EpisodeStats.state_bytes() gives for that group's envs alone."""
        cr, cs, tot = self.state_bytes()
        S, A, n = self.envs_per_group, self.num_agents, C.sizeof(PlayTotals)
        return cr[4 * A * S * g:4 * A * S * (g + 1)], cs[4 * S * g:4 * S * (g + 1)], tot[n * g:n * (g + 1)]


class EpisodeStats(GroupStats):
    """The accounting of one population: GroupStats with one group of num_envs envs — the same kernels, the same bytes — whose read() is
    the one totals dict, plus the device views of the one struct and the outcome latch that follows its freeze."""

    def __init__(self, num_envs, num_agents, games_num, device):
        if int(num_envs) < 1 or int(num_agents) not in (1, 2) or int(games_num) < 1:
            raise ValueError(f"EpisodeStats: num_envs {num_envs} (>= 1), num_agents {num_agents} (1 or 2), games_num {games_num} (>= 1)")
        super().__init__(num_envs, 1, num_agents, games_num, device)
        o = PlayTotals
        self._counts = self._totals[:o.reward.offset].view(torch.int64)                           # games, steps, launches
        self._sums = self._totals[o.reward.offset:o.reward_min.offset].view(torch.float64)        # reward[2], reward_sq[2]
        self._ext = self._totals[o.reward_min.offset:].view(torch.float32)                        # reward_min[2], reward_max[2]

    def totals(self):
        """The totals as 0-dim device tensors (views: they change in place with every accumulate): games, steps, launches, agent 0's
        reward / reward_sq / reward_min / reward_max, and the same four per agent under `per_agent`."""
        A = MAX_AGENTS
        agents = [dict(reward=self._sums[a], reward_sq=self._sums[A + a], reward_min=self._ext[a], reward_max=self._ext[A + a])
                  for a in range(self.num_agents)]
        return dict(games=self._counts[0], steps=self._counts[1], launches=self._counts[2], per_agent=agents, **agents[0])

    def read(self):
        """One host copy of the struct (the stream is waited for) -> totals_dict."""
        return self.read_groups()[0]

    def latch_outcome(self, live, latched):
        """pp_ta_outcome_latch (include/ppenv_ta_outcome.h): latched = live (two pp_ta_outcome tensors) while the totals are not frozen.  One
        launch, before the accumulate of the same control step: `latched` then stops with the totals."""
        _lib.check(self.L.pp_ta_outcome_latch(live.data_ptr(), self._totals.data_ptr(), self.games_num, latched.data_ptr(), _lib.stream(self.device)),
                   self.L)


def pair_totals_dict(t, num_agents=MAX_AGENTS):
    """PlayPairTotals -> a Python dict (the per-agent sums as lists of num_agents; the struct's `cell` and `base` are cell_sum and base_sum)."""
    return dict(pairs=int(t.pairs), steps_diff=int(t.steps_diff), diff=list(t.diff)[:num_agents], diff_sq=list(t.diff_sq)[:num_agents],
                cell_sum=list(t.cell)[:num_agents], base_sum=list(t.base)[:num_agents])


def pair_summary(cell, baseline, totals, num_agents=1):
    """One entry of run()'s paired_diff["cells"] from a pair_totals_dict: over the n = pairs pairs (env i, episode m) both cells played,
    diff = sum(d) / n with d = return(cell) - return(baseline), diff_stderr = sqrt((sum(d^2) - sum(d)^2 / n) / (n - 1) / n) — the standard
    error of the mean of the paired differences, nan for n < 2 — cell_mean and base_mean the two means over the SAME pairs (not the
    av_reward of `groups`, which is over the first games to finish), steps_diff the mean difference of the episode lengths; agent 0's
    figures at the top, all agents' under per_agent.  With no pair the means are nan."""
    n = int(totals["pairs"])
    per_agent = []
    for a in range(num_agents):
        sd, sq = totals["diff"][a], totals["diff_sq"][a]
        mean = sd / n if n > 0 else float("nan")
        stderr = math.sqrt(max(sq - sd * sd / n, 0.0) / (n - 1) / n) if n >= 2 else float("nan")
        per_agent.append(dict(diff=mean, diff_stderr=stderr, cell_mean=totals["cell_sum"][a] / n if n > 0 else float("nan"),
                              base_mean=totals["base_sum"][a] / n if n > 0 else float("nan")))
    out = dict(cell=int(cell), baseline=int(baseline), pairs=n)
    out.update(per_agent[0])
    out["steps_diff"] = totals["steps_diff"] / n if n > 0 else float("nan")
    out["per_agent"] = per_agent
    return out


class PairStats:
    """pp_play_pair_reset / _record / _reduce (include/ppenv_play_pair.h) on torch tensors: for `groups` cells of `envs_per_group` envs
    that are served the same balls, the returns and lengths of the first `episodes` episodes of every env, and read(): per cell the fp64
    sums of the paired difference against cell baseline[g].  baseline: one cell index for all cells, or a sequence of `groups` of them.
    One launch per record(), nothing here synchronises except read() (one more launch and one host copy of groups x 80 bytes)."""

    def __init__(self, envs_per_group, groups, num_agents, episodes, baseline, device):
        self.envs_per_group, self.groups, self.num_agents, self.episodes = S, G, A, M = int(envs_per_group), int(groups), int(num_agents), int(episodes)
        if S < 1 or not 1 <= G <= MAX_GROUPS or A not in (1, 2) or M < 1 or S * G * M * A > 2 ** 31 - 1:
            raise ValueError(f"PairStats: envs_per_group {envs_per_group} (>= 1), groups {groups} (1..{MAX_GROUPS}), num_agents {num_agents} (1 or 2), "
                             f"episodes {episodes} (>= 1), at most 2^31 - 1 table entries")
        self.baseline = baseline_cells(baseline, G)
        self.device = dev = torch.device(device)
        self.num_envs, self.rows = S * G, S * G * A
        self.L = _lib.lib()
        self.cur_reward = torch.zeros(self.rows, dtype=torch.float32, device=dev)
        self.cur_steps = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self.count = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self.ret = torch.zeros((G, S, M, A), dtype=torch.float32, device=dev)
        self.len = torch.zeros((G, S, M), dtype=torch.int32, device=dev)
        assert self.ret.numel() * 4 == self.L.pp_play_pair_ret_bytes(S, G, A, M) and self.len.numel() * 4 == self.L.pp_play_pair_len_bytes(S, G, A, M)
        self._baseline = torch.tensor(self.baseline, dtype=torch.int32, device=dev)
        self._out = torch.zeros(G * C.sizeof(PlayPairTotals), dtype=torch.uint8, device=dev)
        self.reset()

    def _sizes(self):
        return self.envs_per_group, self.groups, self.num_agents, self.episodes

    def _state(self):
        return self.cur_reward.data_ptr(), self.cur_steps.data_ptr(), self.count.data_ptr(), self.ret.data_ptr(), self.len.data_ptr()

    def reset(self):
        _lib.check(self.L.pp_play_pair_reset(*self._sizes(), *self._state(), _lib.stream(self.device)), self.L)

    def record(self, rew, done):
        """One control step, after the env step: rew [rows] f32, done [rows] int64 as for GroupStats.accumulate.  One launch."""
        if rew.dtype != torch.float32 or done.dtype != torch.int64 or rew.numel() != self.rows or done.numel() != self.rows or \
                not rew.is_contiguous() or not done.is_contiguous() or rew.device != self.device or done.device != self.device:
            raise ValueError(f"PairStats.record: rew must be float32 and done int64, contiguous [{self.rows}] on {self.device}")
        _lib.check(self.L.pp_play_pair_record(rew.data_ptr(), done.data_ptr(), *self._sizes(), *self._state(), _lib.stream(self.device)), self.L)

    def reduce(self):
        """The reduce launch alone: the `groups` structs as host bytes (the stream is waited for)."""
        _lib.check(self.L.pp_play_pair_reduce(*self._sizes(), self._baseline.data_ptr(), self.count.data_ptr(), self.ret.data_ptr(), self.len.data_ptr(),
                                              self._out.data_ptr(), _lib.stream(self.device)), self.L)
        return self._out.cpu().numpy().tobytes()

    def read(self):
        """-> a list of pair_totals_dict, in cell order, each with its `cell` and `baseline` index."""
        raw, n = self.reduce(), C.sizeof(PlayPairTotals)
        return [dict(pair_totals_dict(PlayPairTotals.from_buffer_copy(raw[g * n:(g + 1) * n]), self.num_agents), cell=g, baseline=self.baseline[g])
                for g in range(self.groups)]

    def state_bytes(self):
        """cur_reward, cur_steps, count, ret and len as host bytes (the tests compare them)."""
        return tuple(t.cpu().numpy().tobytes() for t in (self.cur_reward, self.cur_steps, self.count, self.ret, self.len))


def baseline_cells(baseline, groups):
    """An int (one baseline cell for all) or a sequence of `groups` cell indices -> the list of `groups` indices; ValueError for an
    index outside 0 .. groups - 1 or a sequence of another length."""
    if isinstance(baseline, (int, np.integer)):
        cells = [int(baseline)] * groups
    else:
        cells = list(baseline)
        if len(cells) != groups or any(not isinstance(b, (int, np.integer)) for b in cells):
            raise ValueError(f"baseline: one cell index, or a sequence of {groups} of them (one per cell), not {baseline!r}")
        cells = [int(b) for b in cells]
    bad = [b for b in cells if not 0 <= b < groups]
    if bad:
        raise ValueError(f"baseline: cell {bad[0]} is outside 0..{groups - 1}")
    return cells


ACT_THRESHOLDS = dict(effort_frac=0.98, vel_frac=0.98, limit_margin=0.02)     # Player(actuators=True)'s; action_clip is the task's clipActions
ACT_INT_FIELDS, ACT_SUM_FIELDS, ACT_MAX_FIELDS = ("c_effort", "c_vel", "c_limit", "c_clip"), ("abs_tau", "tau_sq", "power"), ("max_abs_tau", "max_abs_vel", "max_exc")


def act_totals_dict(group, joints):
    """A PlayActGroup and its D PlayActJoint -> a Python dict: games, samples, launches, energy, energy_sq and, per joint field, a list of D."""
    out = dict(games=int(group.games), samples=int(group.samples), launches=int(group.launches), energy=float(group.energy), energy_sq=float(group.energy_sq))
    for k in ACT_INT_FIELDS:
        out[k] = [int(getattr(j, k)) for j in joints]
    for k in ACT_SUM_FIELDS + ACT_MAX_FIELDS:
        out[k] = [float(getattr(j, k)) for j in joints]
    return out


def sum_act_totals(per_group):
    """A list of act_totals_dict -> one over all groups: counts and sums added in group order, the maxima merged."""
    D = len(per_group[0]["abs_tau"])
    out = dict(games=0, samples=0, launches=0, energy=0.0, energy_sq=0.0, **{k: [0] * D for k in ACT_INT_FIELDS}, **{k: [0.0] * D for k in ACT_SUM_FIELDS},
               max_abs_tau=[0.0] * D, max_abs_vel=[0.0] * D, max_exc=[-math.inf] * D)
    for t in per_group:
        for k in ("games", "samples", "launches", "energy", "energy_sq"):
            out[k] += t[k]
        for d in range(D):
            for k in ACT_INT_FIELDS + ACT_SUM_FIELDS:
                out[k][d] += t[k][d]
            for k in ACT_MAX_FIELDS:
                out[k][d] = max(out[k][d], t[k][d])
    return out


def actuator_summary(totals, limits, names, control_dt):
    """One entry of run()'s actuators["total"] / ["groups"] from an act_totals_dict.  With n = games and s = samples (a game of L control
    steps gives L - 1): energy_per_game [J] = control_dt * energy / n, energy_stderr = control_dt * sqrt((energy_sq - energy^2 / n) / (n - 1) / n)
    (nan for n < 2), mean_power [W] = energy / s — the power term sum_d |tau * qd| averaged over the samples — and `per_joint`, one dict per
    joint: tau_mean_abs, tau_rms, tau_peak [N m], tau_peak_frac = tau_peak / effort, vel_peak [rad / s], vel_peak_frac = vel_peak / vel_limit,
    excursion_max [rad] = the largest of max(lower - q, q - upper) (positive: beyond the limit; -inf with no sample), power_mean [W], and the
    rates over the samples at_effort, at_vel_limit, at_pos_limit, action_clip.  The per-sample figures are nan with no sample."""
    n, s, nan = int(totals["games"]), int(totals["samples"]), float("nan")
    e, esq, dt = totals["energy"], totals["energy_sq"], float(control_dt)
    out = dict(games=n, samples=s, energy_per_game=dt * e / n if n > 0 else nan,
               energy_stderr=dt * math.sqrt(max(esq - e * e / n, 0.0) / (n - 1) / n) if n >= 2 else nan, mean_power=e / s if s > 0 else nan)
    rate = (lambda v: v / s) if s > 0 else (lambda v: nan)
    out["per_joint"] = [dict(joint=names[d], tau_mean_abs=rate(totals["abs_tau"][d]), tau_rms=math.sqrt(rate(totals["tau_sq"][d])) if s > 0 else nan,
                             tau_peak=totals["max_abs_tau"][d], tau_peak_frac=totals["max_abs_tau"][d] / float(limits[d][2]), at_effort=rate(totals["c_effort"][d]),
                             vel_peak=totals["max_abs_vel"][d], vel_peak_frac=totals["max_abs_vel"][d] / float(limits[d][3]), at_vel_limit=rate(totals["c_vel"][d]),
                             at_pos_limit=rate(totals["c_limit"][d]), excursion_max=totals["max_exc"][d], power_mean=rate(totals["power"][d]),
                             action_clip=rate(totals["c_clip"][d])) for d in range(len(names))]
    return out


def actuator_table(entry, title=""):
    """The CLI's table for one entry of actuators["groups"] (or its total): a head line, then one row per joint."""
    lines = [f"actuators {title}: games {entry['games']} samples {entry['samples']} energy/game {entry['energy_per_game']:.6g} +- {entry['energy_stderr']:.3g} J "
             f"mean power {entry['mean_power']:.6g} W",
             f"  {'joint':<28}{'|tau| mean':>11}{'rms':>9}{'peak':>9}{'/effort':>8}{'at eff':>8}{'vel peak':>10}{'/limit':>8}{'at vel':>8}{'at pos':>8}"
             f"{'exc max':>9}{'power':>9}{'act clip':>9}"]
    for j in entry["per_joint"]:
        lines.append(f"  {j['joint']:<28}{j['tau_mean_abs']:>11.4g}{j['tau_rms']:>9.4g}{j['tau_peak']:>9.4g}{j['tau_peak_frac']:>8.3f}{j['at_effort']:>8.3f}"
                     f"{j['vel_peak']:>10.4g}{j['vel_peak_frac']:>8.3f}{j['at_vel_limit']:>8.3f}{j['at_pos_limit']:>8.3f}{j['excursion_max']:>9.3g}"
                     f"{j['power_mean']:>9.4g}{j['action_clip']:>9.3f}")
    return "\n".join(lines)


def actuator_limits(task):
    """The joints' limits from the numbers the step kernels themselves run with -> (float32 [D, 4]: lower, upper, effort, vel_limit; the D
    joint names): the env's joint_limits() (scene.joint_limits, scene.ta_joint_limits)."""
    return task.env.joint_limits()


def control_dt_of(task):
    """Seconds per control step (the env's control_dt: controlFrequencyInv already folded in)."""
    return task.env.control_dt


class ActuatorStats:
    """pp_play_act_reset / pp_play_act_accumulate (include/ppenv_play_act.h) on torch tensors: per joint, torque / speed / position / power /
    action usage of `groups` populations of `envs_per_group` envs with `num_dofs` joints each, folded into per-group totals when an env
    finishes a game, each group freezing on its own at games_num.  limits: [D, 4] (lower, upper, effort, vel_limit); thresholds:
    dict(effort_frac, vel_frac, limit_margin, action_clip).  Two launches per accumulate, nothing here synchronises except read() /
    state_bytes()."""

    def __init__(self, envs_per_group, groups, num_dofs, games_num, limits, thresholds, device, num_agents=1):
        self.envs_per_group, self.groups, self.num_dofs, self.games_num, self.num_agents = S, G, D, _, A = \
            int(envs_per_group), int(groups), int(num_dofs), int(games_num), int(num_agents)
        if S < 1 or not 1 <= G <= MAX_GROUPS or A not in (1, 2) or not 1 <= D <= _lib.PLAY_ACT_MAX_DOF or D % A or self.games_num < 1 or S * G * A > 2 ** 31 - 1:
            raise ValueError(f"ActuatorStats: envs_per_group {envs_per_group} (>= 1), groups {groups} (1..{MAX_GROUPS}), num_agents {num_agents} (1 or 2), "
                             f"num_dofs {num_dofs} (1..{_lib.PLAY_ACT_MAX_DOF}, a multiple of num_agents), games_num {games_num} (>= 1), at most 2^31 - 1 rows")
        lim = np.ascontiguousarray(limits, np.float32)
        if lim.shape != (D, 4):
            raise ValueError(f"ActuatorStats: limits must be [{D}, 4] (lower, upper, effort, vel_limit), not {list(lim.shape)}")
        self.thresholds = {k: float(thresholds[k]) for k in ("effort_frac", "vel_frac", "limit_margin", "action_clip")}
        self._thr = _lib.PlayActThresholds(**self.thresholds)
        self.device = dev = torch.device(device)
        self.num_envs = S * G
        L = self.L = _lib.lib()
        self.limits = lim
        self._limits = torch.from_numpy(lim).to(dev)
        self._state = torch.zeros(int(L.pp_play_act_state_bytes(S, G, D)), dtype=torch.uint8, device=dev)
        self._group = torch.zeros(G * C.sizeof(_lib.PlayActGroup), dtype=torch.uint8, device=dev)
        self._joint = torch.zeros(G * D * C.sizeof(_lib.PlayActJoint), dtype=torch.uint8, device=dev)
        self._partial = torch.zeros(int(L.pp_play_act_partial_bytes(S, G, D)), dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        _lib.check(self.L.pp_play_act_reset(self.envs_per_group, self.groups, self.num_dofs, self._state.data_ptr(), self._group.data_ptr(),
                                            self._joint.data_ptr(), _lib.stream(self.device)), self.L)

    def _input(self, name, t):
        """A float32 tensor holding value (e, d) -> PlayActInput: a [N, D] view with ANY strides (env.dof_pos.T, dof_states[..., 0]) is
        taken by its strides; a contiguous tensor of N * D elements in another shape (the [A * N, D / A] actions) is read row-major."""
        N, D = self.num_envs, self.num_dofs
        if t is None:
            return _lib.PlayActInput(None, 0, 0)
        if t.dtype != torch.float32 or t.device != self.device or t.numel() != N * D or not (tuple(t.shape) == (N, D) or t.is_contiguous()):
            raise ValueError(f"ActuatorStats.accumulate: {name} must be float32 on {self.device}, a [{N}, {D}] view or contiguous with {N * D} elements")
        es, ds = t.stride() if tuple(t.shape) == (N, D) else (D, 1)
        return _lib.PlayActInput(t.data_ptr(), es, ds)

    def accumulate(self, q, qd, tau, action, done):
        """One control step, after the env step: joint positions, velocities, drive torques and (or None) the policy's raw actions as
        tensors holding value (env, dof) — see _input — and done [num_agents * N] int64 (VecTask.step's reset_buf).  Two launches, no
        synchronisation, no copy."""
        if done.dtype != torch.int64 or done.numel() != self.num_envs * self.num_agents or not done.is_contiguous() or done.device != self.device:
            raise ValueError(f"ActuatorStats.accumulate: done must be int64, contiguous [{self.num_envs * self.num_agents}] on {self.device}")
        ins = _lib.PlayActInputs(self._input("q", q), self._input("qd", qd), self._input("tau", tau), self._input("action", action))
        _lib.check(self.L.pp_play_act_accumulate(C.byref(ins), done.data_ptr(), self.envs_per_group, self.groups, self.num_agents, self.num_dofs, self.games_num,
                                                 self._limits.data_ptr(), C.byref(self._thr), self._state.data_ptr(), self._group.data_ptr(),
                                                 self._joint.data_ptr(), self._partial.data_ptr(), _lib.stream(self.device)), self.L)

    def read(self):
        """One host copy of the totals (the stream is waited for) -> a list of act_totals_dict, in group order."""
        _, graw, jraw = self.state_bytes(state=False)
        D, ng, nj = self.num_dofs, C.sizeof(_lib.PlayActGroup), C.sizeof(_lib.PlayActJoint)
        return [act_totals_dict(_lib.PlayActGroup.from_buffer_copy(graw[g * ng:(g + 1) * ng]),
                                [_lib.PlayActJoint.from_buffer_copy(jraw[(g * D + d) * nj:(g * D + d + 1) * nj]) for d in range(D)]) for g in range(self.groups)]

    def state_bytes(self, state=True):
        """The running state, the G group structs and the G * D joint structs as host bytes (the tests compare them)."""
        return (self._state.cpu().numpy().tobytes() if state else b"", self._group.cpu().numpy().tobytes(), self._joint.cpu().numpy().tobytes())

    def partial_bytes(self):
        """The last launch's per-chunk partials as host bytes: G * parts group structs, then G * parts * D joint structs."""
        return self._partial.cpu().numpy().tobytes()


DELAY_MAX, DELAY_MAX_WIDTH = _lib.PLAY_DELAY_MAX, _lib.PLAY_DELAY_MAX_WIDTH


class Delay:
    """pp_play_delay_reset / pp_play_delay_push (include/ppenv_play_delay.h) on torch tensors: a delay line of whole control steps for a
    [rows, width] float32 tensor, row r delayed by delays[r] (an int array [rows], 0 .. 15) — push(x, done) stores this control step's
    sample and returns the one delays[r] steps old of the same episode, or the episode's first sample while there is none that old;
    `done` ([rows] int64, the done the previous env step returned, or None right after reset()) marks the sample as the first of a new
    episode of its env (agent 0's word, as everywhere in this module).  It owns the ring [max(delays) + 1, rows, width], the ages and the
    output; x is not modified.  One launch per push, nothing here synchronises."""

    def __init__(self, rows, width, delays, device, num_agents=1):
        self.rows, self.width, self.num_agents = R, W, A = int(rows), int(width), int(num_agents)
        if R < 1 or A not in (1, 2) or R % A or not 1 <= W <= DELAY_MAX_WIDTH:
            raise ValueError(f"Delay: rows {rows} (>= 1, a multiple of num_agents), num_agents {num_agents} (1 or 2), width {width} (1..{DELAY_MAX_WIDTH})")
        d = np.asarray(delays)
        if d.shape != (R,) or d.dtype.kind not in "iu" or int(d.min()) < 0 or int(d.max()) > DELAY_MAX:
            raise ValueError(f"Delay: delays must be an integer array [{R}] of whole control steps 0..{DELAY_MAX}, not {d.dtype} {list(d.shape)}" +
                             (f" with values {int(d.min())}..{int(d.max())}" if d.size and d.dtype.kind in "iu" else ""))
        self.delays = np.ascontiguousarray(d, np.int32)
        self.depth = int(self.delays.max()) + 1                       # every delay < depth: what pp_play_delay_push leaves to its caller
        self.device = dev = torch.device(device)
        L = self.L = _lib.lib()
        self._delay = torch.from_numpy(self.delays).to(dev)
        self.age = torch.zeros(R, dtype=torch.int32, device=dev)
        self.ring = torch.zeros((self.depth, R, W), dtype=torch.float32, device=dev)
        assert self.ring.numel() * 4 == L.pp_play_delay_ring_bytes(R, W, self.depth)
        self.out = torch.zeros((R, W), dtype=torch.float32, device=dev)
        self.reset()

    def reset(self):
        _lib.check(self.L.pp_play_delay_reset(self.rows, self.age.data_ptr(), _lib.stream(self.device)), self.L)

    def push(self, x, done=None):
        """x: float32 [rows, width] on this device, unit stride along the row and a row stride >= width (a contiguous tensor, or the first
        `width` columns of a wider one).  -> the [rows, width] output tensor (this object's: the next push overwrites it)."""
        R, W = self.rows, self.width
        if x.dtype != torch.float32 or x.device != self.device or tuple(x.shape) != (R, W) or (W > 1 and x.stride(1) != 1) or (R > 1 and x.stride(0) < W):
            raise ValueError(f"Delay.push: x must be float32 [{R}, {W}] on {self.device} with unit stride along the row and a row stride >= {W}")
        if done is not None and (done.dtype != torch.int64 or done.numel() != R or not done.is_contiguous() or done.device != self.device):
            raise ValueError(f"Delay.push: done must be int64, contiguous [{R}] on {self.device}, or None")
        _lib.check(self.L.pp_play_delay_push(x.data_ptr(), x.stride(0) if R > 1 else W, _lib.ptr(done), R, self.num_agents, W, self.depth, self._delay.data_ptr(),
                                             self.age.data_ptr(), self.ring.data_ptr(), self.out.data_ptr(), W, _lib.stream(self.device)), self.L)
        return self.out


_AXIS = re.compile(r"^([A-Za-z_]\w*)(?:\[(\d+)\])?$")


SERVE_AXES = serve.AXES_27DOF              # serve_speed, serve_tilt, serve_tilt_z; ball_y, ball_z (27-dof task only)
DELAY_AXES = ("action_delay", "obs_delay")  # control latency in whole control steps: the command path, the sensing path


def delay_steps(axis, v):
    """A latency value -> the int 0 .. DELAY_MAX; 2.0 (the CLI's float parse) is 2.  Anything else — a fraction, a (lo, hi) range, a
    value outside the range — raises ValueError naming the axis."""
    try:
        ok = not isinstance(v, (bool, tuple, list, str)) and float(v) == int(v) and 0 <= int(v) <= DELAY_MAX
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"sweep axis {axis!r}: a delay is a number of whole control steps 0..{DELAY_MAX}, not {v!r}")
    return int(v)


def _axis(axis):
    """'name' or 'name[row]' -> (table name, row or None), or (serve axis, None), or (latency axis, None); a name that is none of these
    raises ValueError."""
    if isinstance(axis, str) and (axis in SERVE_AXES or axis in DELAY_AXES):
        return axis, None
    m = _AXIS.match(axis) if isinstance(axis, str) else None
    if m is None or m.group(1) not in TABLE_NAMES:
        raise ValueError(f"sweep axis {axis!r}: an axis is one of {', '.join(TABLE_NAMES)}, or one row of a table as name[row], or a serve axis: "
                         f"{', '.join(SERVE_AXES)}, or a latency axis in whole control steps: {', '.join(DELAY_AXES)}")
    return m.group(1), None if m.group(2) is None else int(m.group(2))


class Sweep:
    """G cells of physical parameters, one per group of envs.  A cell maps an axis to one scalar scale; an axis is a table of
    dr.Randomizable.set_randomization (`friction_scale`: every row of it) or one row of one (`dof_stiffness_scale[5]`, which wins over
    the plain axis of the same table in that row).  What a cell does not name stays 1.0.
    A SERVE axis (SERVE_AXES: serve_speed, serve_tilt, serve_tilt_z in degrees; ball_y, ball_z on the 27-dof task) maps to a number — the
    quantity is pinned, and may be negative — or a (lo, hi) range it is drawn from; what a cell does not name is the task's configured range.
    A LATENCY axis (DELAY_AXES: action_delay, obs_delay) maps to a whole number of control steps 0 .. 15 — how old the command the env
    consumes, or the observation the policy sees, is (Delay; Player) — and is seen by neither tables() nor serve_cells(); what a cell does
    not name is the Player's keyword (default 0).
    paired: env i of every group is served the same sequence of balls (a serve plan keyed by the index within the group), with or
    without a serve axis."""

    def __init__(self, cells, paired=False):
        self.cells = [dict(c) for c in cells]
        self.paired = bool(paired)
        if not 1 <= len(self.cells) <= MAX_GROUPS:
            raise ValueError(f"a sweep has 1..{MAX_GROUPS} cells, not {len(self.cells)}")
        for cell in self.cells:
            for axis, v in cell.items():
                if _axis(axis)[0] in SERVE_AXES:
                    lo, hi = serve.value_range(axis, v)
                    cell[axis] = lo if lo == hi else (lo, hi)
                    continue
                if axis in DELAY_AXES:
                    cell[axis] = delay_steps(axis, v)
                    continue
                cell[axis] = float(v)
                if not math.isfinite(cell[axis]) or cell[axis] < 0.0:
                    raise ValueError(f"sweep axis {axis!r}: the scale {v!r} is not a finite number >= 0")

    def __len__(self):
        return len(self.cells)

    @classmethod
    def grid(cls, axes, paired=False):
        """{axis: values, ...} -> the Cartesian product, the last axis fastest."""
        names = list(axes)
        values = [list(axes[k]) for k in names]
        if not names or any(len(v) == 0 for v in values):
            raise ValueError("Sweep.grid: at least one axis, and at least one value per axis")
        return cls([dict(zip(names, combo)) for combo in itertools.product(*values)], paired=paired)

    @classmethod
    def parse(cls, specs, paired=False):
        """The CLI form, one 'AXIS=SPEC' per axis -> Sweep.grid: SPEC is `lo:hi:count` (an inclusive linspace) or a comma list taken as given
        (on a serve axis: pinned values)."""
        axes = {}
        for spec in specs:
            axis, eq, text = str(spec).partition("=")
            axis = axis.strip()
            try:
                if not eq or not text.strip():
                    raise ValueError("no '=' or nothing after it")
                if ":" in text:
                    lo, hi, count = text.split(":")
                    if int(count) < 1:
                        raise ValueError("count < 1")
                    values = [float(v) for v in np.linspace(float(lo), float(hi), int(count))]
                else:
                    values = [float(v) for v in text.split(",")]
            except ValueError as e:
                raise ValueError(f"--sweep {spec!r}: expected AXIS=lo:hi:count or AXIS=v0,v1,... ({e})") from None
            if axis in axes:
                raise ValueError(f"--sweep {spec!r}: the axis {axis!r} is given twice")
            _axis(axis)
            axes[axis] = values
        return cls.grid(axes, paired=paired)

    def serve_cells(self, defaults):
        """The per-group cells of the serve plan for a task whose serve axes and configured ranges are `defaults` ({axis: (lo, hi)}: the env's
        serve_defaults()) -> one {axis: (lo, hi)} per cell, or None when no cell names a serve axis and `paired` is false (no plan is needed).
        A serve axis the task does not have (ball_y, ball_z on a 7-dof task) raises ValueError naming the axes it has."""
        named = [{a: v for a, v in cell.items() if a in SERVE_AXES} for cell in self.cells]
        if not self.paired and not any(named):
            return None
        return serve.resolve_cells(named, defaults, tuple(defaults))

    def _envs_per_cell(self, num_envs):
        G, N = len(self.cells), int(num_envs)
        if N < G or N % G:
            below = N // G * G
            raise ValueError(f"a sweep of {G} cells needs a multiple of {G} envs, not {N}: the nearest are " +
                             (f"{below} and {below + G}" if below > 0 else f"{G}"))
        return N // G

    def cell_delays(self, action_delay=0, obs_delay=0):
        """-> {axis: [per cell, the cell's value or the keyword's]} for the two latency axes."""
        default = dict(action_delay=delay_steps("action_delay", action_delay), obs_delay=delay_steps("obs_delay", obs_delay))
        return {axis: [int(cell.get(axis, default[axis])) for cell in self.cells] for axis in DELAY_AXES}

    def delays(self, num_envs, num_agents, action_delay=0, obs_delay=0):
        """The per-row delays of this sweep for num_envs envs of num_agents rows each -> {axis: int32 [num_agents * num_envs]} for both
        latency axes; cell g fills the rows [A * S * g, A * S * (g + 1)), with the keyword's value where it does not name the axis."""
        S, A = self._envs_per_cell(num_envs), int(num_agents)
        return {axis: np.repeat(np.asarray(per, np.int32), A * S) for axis, per in self.cell_delays(action_delay, obs_delay).items()}

    def tables(self, rows_by_name, num_envs):
        """The per-env tables of this sweep for an environment of num_envs envs whose tables have rows_by_name rows (its DR_TABLE_ROWS; 0: a
        per-env scalar) -> {name: float32 array [rows, N] or [N]} for the tables some cell names; cell g fills columns [g * S, (g + 1) * S)."""
        N = int(num_envs)
        S = self._envs_per_cell(N)
        out = {}
        for plain in (True, False):                                  # the whole-table axes first, then the single rows over them
            for g, cell in enumerate(self.cells):
                for axis, v in cell.items():
                    name, row = _axis(axis)
                    if (row is None) != plain or name in SERVE_AXES or name in DELAY_AXES:
                        continue
                    if name not in rows_by_name:
                        raise ValueError(f"sweep axis {axis!r}: this environment's tables are {', '.join(rows_by_name)}")
                    rows = int(rows_by_name[name])
                    if name not in out:
                        out[name] = np.ones((rows, N) if rows else (N,), np.float32)
                    if row is None:
                        out[name][..., g * S:(g + 1) * S] = v
                    elif row >= rows:
                        raise ValueError(f"sweep axis {axis!r}: {name} has " + (f"{rows} rows (0..{rows - 1})" if rows else "no rows (one scale per env: name it plainly)") +
                                         f"; the tables and their rows are {dict(rows_by_name)}")
                    else:
                        out[name][row, g * S:(g + 1) * S] = v
        return out


def sum_totals(per_group):
    """A list of totals dicts (GroupStats.read()) -> one totals dict over all groups: counts and sums added in group order (`launches` too:
    group-steps), the extrema merged."""
    A = len(per_group[0]["reward"])
    out = dict(games=0, steps=0, launches=0, reward=[0.0] * A, reward_sq=[0.0] * A, reward_min=[math.inf] * A, reward_max=[-math.inf] * A)
    for t in per_group:
        for k in ("games", "steps", "launches"):
            out[k] += t[k]
        for a in range(A):
            out["reward"][a] += t["reward"][a]
            out["reward_sq"][a] += t["reward_sq"][a]
            out["reward_min"][a] = min(out["reward_min"][a], t["reward_min"][a])
            out["reward_max"][a] = max(out["reward_max"][a], t["reward_max"][a])
    return out


def group_summary(cell, totals, num_agents, games_num, paired=False):
    """One entry of run()'s `groups`: the cell, summarize() of the group's totals, reward_stderr = reward_std / sqrt(games) (nan with no
    game; the UNPAIRED standard error, conservative for a difference of paired cells), complete = games >= games_num and `paired`."""
    out = dict(cell=dict(cell), paired=bool(paired))
    out.update(summarize(totals, num_agents))
    g = out["games"]
    out["reward_stderr"] = out["reward_std"] / math.sqrt(g) if g > 0 else float("nan")
    out["complete"] = g >= int(games_num)
    return out


def cell_text(cell):
    return " ".join(f"{k}={v:g}" if not isinstance(v, (tuple, list)) else f"{k}={v[0]:g}..{v[1]:g}" for k, v in cell.items()) or "(plain)"


def group_line(g):
    """The CLI's line for one entry of `groups`."""
    return (f"cell {cell_text(g['cell'])}: games {g['games']} av reward {g['av_reward']:.6g} +- {g['reward_stderr']:.3g} av steps {g['av_steps']:.6g} "
            f"min {g['reward_min']:.6g} max {g['reward_max']:.6g}" + ("" if g["complete"] else " (incomplete)"))


def pair_line(p, groups, full):
    """The CLI's line for one entry of paired_diff["cells"]; groups: the result's `groups` (the cells' texts), full: the S * M pairs a
    complete cell has."""
    return (f"cell {p['cell']} {cell_text(groups[p['cell']]['cell'])}: vs cell {p['baseline']}: pairs {p['pairs']} diff {p['diff']:.6g} +- {p['diff_stderr']:.3g} "
            f"(cell {p['cell_mean']:.6g}, base {p['base_mean']:.6g}) steps diff {p['steps_diff']:.6g}" + ("" if p["pairs"] == full else " (incomplete)"))


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
    a line in use the result gains `latency` = dict(control_dt, action_delay=[per cell], obs_delay=[per cell])."""

    def __init__(self, task, policy, games_num=2000, deterministic=True, seed=0, poll_every=64, max_steps=108000, sigma=None, recorder=None,
                 outcomes=False, sweep=None, paired_diff=False, baseline=0, pair_episodes=None, actuators=False, action_delay=0, obs_delay=0):
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
            if p.net.num_obs != task.num_obs or p.net.num_actions != task.num_actions:
                raise ValueError(f"the policy maps {p.net.num_obs} observations to {p.net.num_actions} actions, the task has "
                                 f"{task.num_obs} and {task.num_actions}")
        self.task, self.policy = task, self.policies[0]
        self.games_num, self.poll_every, self.max_steps = int(games_num), int(poll_every), int(max_steps)
        self.deterministic, self.seed = bool(deterministic), int(seed)
        self.num_agents = int(task.num_agents)
        self._distinct = list({id(p): p for p in self.policies}.values())
        if sigma is not None:
            for p in self._distinct:
                p.sigma.fill_(math.exp(float(sigma)))
        self.sweep = sweep
        self._tables = self._episode0 = self._serve_cells = None
        if sweep is None:
            self.stats = EpisodeStats(task.num_envs, self.num_agents, self.games_num, sim)
        else:
            self._tables = sweep.tables(task.env.DR_TABLE_ROWS, task.num_envs)
            if sweep.paired or any(a in SERVE_AXES for cell in sweep.cells for a in cell):
                self._serve_cells = sweep.serve_cells(task.env.serve_defaults())
            self.stats = GroupStats(task.num_envs // len(sweep), len(sweep), self.num_agents, self.games_num, sim)
        self.pairs = None
        if paired_diff:
            S = task.num_envs // len(sweep)
            self.pair_episodes = int(pair_episodes) if pair_episodes is not None else -(-self.games_num // S)
            self.pairs = PairStats(S, len(sweep), self.num_agents, self.pair_episodes, self._baseline, sim)
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
            G = 1 if sweep is None else len(sweep)
            self.act = ActuatorStats(task.num_envs // G, G, len(self._act_names), self.games_num, self._act_limits, thr, sim, num_agents=self.num_agents)
            self._act_inputs = task.env.joint_views()                     # the 27-dof AoS tensors, the 7-dof SoA planes: [N, D] views
        rows = task.num_envs * self.num_agents
        if sweep is None:
            self._cell_delays = {axis: [delay_steps(axis, v)] for axis, v in (("action_delay", action_delay), ("obs_delay", obs_delay))}
            per_row = {axis: np.full(rows, per[0], np.int32) for axis, per in self._cell_delays.items()}
        else:
            self._cell_delays = sweep.cell_delays(action_delay, obs_delay)
            per_row = sweep.delays(task.num_envs, self.num_agents, action_delay, obs_delay)
        # a line whose delays are all zero is not built: that path is the player without the feature
        self._act_line = Delay(rows, task.num_actions, per_row["action_delay"], sim, self.num_agents) if per_row["action_delay"].any() else None
        self._obs_line = Delay(rows, task.num_obs, per_row["obs_delay"], sim, self.num_agents) if per_row["obs_delay"].any() else None
        self._done_prev = None
        self._runs = self._cell_actions = None
        if per_cell:                                                     # runs of consecutive cells that hold the same object: (policy, first row, end row)
            w, runs = self.num_agents * (task.num_envs // len(sweep)), []
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
            latency = any(a in DELAY_AXES for cell in self.sweep.cells for a in cell)
            if self._tables or (self._serve_cells is None and not latency):      # (a sweep of serves or of latency alone keeps the plain step kernel)
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
        for line in (self._act_line, self._obs_line):
            if line is not None:
                line.reset()
        self._done_prev = None
        for p in self._distinct:
            p._counter = 0
        self._obs = self.task.reset()["obs"]
        self.steps_played = 0

    def _act_per_cell(self, obs):
        """Every run of cells under its own policy, into ONE [rows, num_actions] tensor: a policy owns its output buffer and may serve
        several runs, so each result is copied out before the next act()."""
        if self._cell_actions is None:
            self._cell_actions = torch.empty((obs.shape[0], self.task.num_actions), dtype=torch.float32, device=obs.device)
        for p, r0, r1 in self._runs:
            a, _ = p.act(obs[r0:r1], deterministic=self.deterministic, seed=self.seed)
            self._cell_actions[r0:r1].copy_(a)
        return self._cell_actions

    def step(self):
        """One control step: (obs line ->) policy (-> action line) -> task.step -> accumulate (-> record, with paired_diff).  No host read."""
        if self._obs is None:
            self.start()
        self.policy_obs = self._obs if self._obs_line is None else self._obs_line.push(self._obs, self._done_prev)
        if self._runs is None:
            self.actions, _ = self.policy.act(self.policy_obs, deterministic=self.deterministic, seed=self.seed)
        else:
            self.actions = self._act_per_cell(self.policy_obs)
        self.applied_actions = self.actions if self._act_line is None else self._act_line.push(self.actions, self._done_prev)
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
        return outcomes_dict(TAOutcome.from_buffer_copy(self._latched.cpu().numpy().tobytes()))

    def read_actuators(self):
        """One host copy of the actuator totals -> run()'s `actuators`: dict(thresholds, joints = the names, control_dt, total =
        actuator_summary of every group summed, groups = one actuator_summary per cell with its `cell`); None with actuators off."""
        if self.act is None:
            return None
        per, dt = self.act.read(), control_dt_of(self.task)
        cells = self.sweep.cells if self.sweep is not None else [{}]
        return dict(thresholds=dict(self.act.thresholds), joints=list(self._act_names), control_dt=dt,
                    total=actuator_summary(sum_act_totals(per), self._act_limits, self._act_names, dt),
                    groups=[dict(cell=dict(c), **actuator_summary(t, self._act_limits, self._act_names, dt)) for c, t in zip(cells, per)])

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
                    tot = per[0] if self.sweep is None else sum_totals(per)
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
                out["groups"] = [group_summary(cell, t, self.num_agents, self.games_num, self.sweep.paired) for cell, t in zip(self.sweep.cells, per)]
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
            return out
        finally:
            self.end_sweep()


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m isaacgym_amd.play", description="play a checkpoint (rl_games' player) on the native env and network")
    ap.add_argument("--task", default="HumanoidPingpongTiltNESSparse27DOFG1")
    ap.add_argument("--checkpoint", required=True, help="nn/<task>.pth as python -m isaacgym_amd.ppo (or rl_games) writes it")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--games", type=int, default=2000, help="rl_games' games_num")
    ap.add_argument("--stochastic", action="store_true", help="draw the actions from Normal(mu, sigma) instead of playing mu")
    ap.add_argument("--sigma", type=float, default=None, help="override the log-std with this value (train.py:214); sigma = exp(value)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cfg-dir", default=None, help="a reference cfg/ directory to compose the task yaml from")
    ap.add_argument("--poll-every", type=int, default=64, help="control steps between two host reads of the totals")
    ap.add_argument("--max-steps", type=int, default=108000)
    ap.add_argument("--outcomes", action="store_true", help="27-dof task: print the reference's five outcome counts (TA:1164-1168) as rates of the envs")
    ap.add_argument("--sweep", action="append", default=None, metavar="AXIS=SPEC", help="play under a grid of physical-parameter scales in one pass (repeatable: "
                    "one axis each; the envs are split into one group per cell and --games is per cell): AXIS is dof_stiffness_scale, dof_damping_scale, "
                    "link_mass_scale, restitution_scale or friction_scale, or one row of a table as NAME[ROW], or a serve axis: serve_speed, serve_tilt, "
                    "serve_tilt_z (degrees; may be negative), ball_y, ball_z (27-dof task), or a latency axis in whole control steps (0..15): action_delay, "
                    "obs_delay; SPEC is lo:hi:count (inclusive) or v0,v1,...")
    ap.add_argument("--paired", action="store_true", help="with --sweep: env i of every cell is served the same sequence of balls (common random numbers), "
                    "so the serve noise cancels in the difference of two cells")
    ap.add_argument("--sweep-out", default=None, metavar="FILE.json", help="with --sweep: write the per-cell results (the result's `groups`) to FILE.json")
    ap.add_argument("--paired-diff", action="store_true", help="with --sweep ... --paired: per cell, the mean of return(cell) - return(baseline cell) over the "
                    "same balls (env i, episode m of both cells), with its own standard error")
    ap.add_argument("--baseline", type=int, default=None, metavar="INDEX", help="with --paired-diff: the baseline cell, in the order the cells are printed (default 0)")
    ap.add_argument("--paired-out", default=None, metavar="FILE.json", help="with --paired-diff or --against: write the result's `paired_diff` to FILE.json")
    ap.add_argument("--against", action="append", default=None, metavar="PATH", help="another checkpoint to play on the same balls (repeatable): the cells become "
                    "checkpoints x sweep cells, --checkpoint's first (without --sweep: one cell per checkpoint); implies --paired and --paired-diff, the "
                    "baseline of every cell being the same sweep cell under --checkpoint; --num-envs must be a multiple of the cell count")
    ap.add_argument("--actuators", action="store_true", help="per joint and per cell: torque against the effort limit, speed against the velocity limit, "
                    "position against the joint limits, mechanical energy per game and raw actions at clipActions, summed on the device; one table per cell")
    ap.add_argument("--actuators-out", default=None, metavar="FILE.json", help="with --actuators: write the result's `actuators` to FILE.json")
    ap.add_argument("--effort-frac", type=float, default=None, help=f"with --actuators: at the effort limit means |tau| >= this x effort (default {ACT_THRESHOLDS['effort_frac']})")
    ap.add_argument("--vel-frac", type=float, default=None, help=f"with --actuators: at the velocity limit means |qd| >= this x the limit (default {ACT_THRESHOLDS['vel_frac']})")
    ap.add_argument("--limit-margin", type=float, default=None, help="with --actuators: at a position limit means within this many rad of it, or beyond "
                    f"(default {ACT_THRESHOLDS['limit_margin']})")
    ap.add_argument("--action-delay", type=int, default=0, metavar="K", help=f"control latency of the command path: the env consumes the action of K control steps "
                    f"ago (0..{DELAY_MAX}; the episode's first action is held until there is one that old); with --sweep, the value of the cells that do not "
                    "name action_delay")
    ap.add_argument("--obs-delay", type=int, default=0, metavar="K", help=f"control latency of the sensing path: the policy sees the observation of K control "
                    f"steps ago (0..{DELAY_MAX}); with --sweep, the value of the cells that do not name obs_delay")
    ap.add_argument("--capture", default=None, metavar="FILE", help="record the run to FILE: .gif, .png (numbered files) or .npy (isaacgym_amd.render)")
    ap.add_argument("--capture-envs", default="0", help="comma-separated env ids to draw, side by side (at most 16)")
    ap.add_argument("--capture-len", type=int, default=300, help="frames kept: the last this many")
    ap.add_argument("--capture-every", type=int, default=2, help="control steps between two frames")
    ap.add_argument("--capture-size", default="640x480", help="WIDTHxHEIGHT of one env's picture")
    ap.add_argument("--capture-fps", type=float, default=30.0)
    ap.add_argument("--capture-samples", type=int, default=1, choices=(1, 2, 4), help="rays per pixel and axis: 2 is 2 x 2 supersampling, 4 is 4 x 4")
    ap.add_argument("--capture-deferred", action="store_true", help="record the posed primitives while playing and cast all rays in one batched launch at the "
                    "end (render.Trajectory): the same file, byte for byte")
    ap.add_argument("--capture-trajectory", default=None, metavar="FILE.npz", help="also save the recording as data (records deferred): "
                    "python -m isaacgym_amd.render replay draws it again at any size, sample count and camera")
    ap.add_argument("--camera", choices=("side", "follow"), default="side", help="side: table and humanoid(s); follow: the reference viewer's follow-cam")
    args = ap.parse_args(argv)
    if args.sweep_out and not args.sweep:
        ap.error("--sweep-out needs --sweep")
    if args.paired and not args.sweep:
        ap.error("--paired needs --sweep")
    if not args.actuators:
        for flag, v in (("--actuators-out", args.actuators_out), ("--effort-frac", args.effort_frac), ("--vel-frac", args.vel_frac),
                        ("--limit-margin", args.limit_margin)):
            if v is not None:
                ap.error(f"{flag} needs --actuators")
    if args.against:
        if args.baseline is not None:
            ap.error("--baseline does not go with --against: the baseline of every cell is the same sweep cell under --checkpoint")
        if args.outcomes:
            ap.error("--against plays the checkpoints as the cells of a sweep, and --outcomes cannot be split by cell")
    else:
        if args.paired_diff and not (args.sweep and args.paired):
            ap.error("--paired-diff needs --sweep ... --paired: without common serves, episode m of env i is a different ball in every cell")
        if args.baseline is not None and not args.paired_diff:
            ap.error("--baseline needs --paired-diff")
        if args.paired_out and not args.paired_diff:
            ap.error("--paired-out needs --paired-diff or --against")
    for flag, axis in (("--action-delay", "action_delay"), ("--obs-delay", "obs_delay")):
        if not 0 <= getattr(args, axis) <= DELAY_MAX:
            ap.error(f"{flag} is a number of whole control steps 0..{DELAY_MAX}")
    if args.sweep:
        try:
            Sweep.parse(args.sweep)
        except ValueError as e:
            ap.error(str(e))
    return args


def latency_line(lat):
    """The CLI's head line for run()'s `latency`: per axis the cells' delays in control steps and in milliseconds."""
    ms = 1000.0 * lat["control_dt"]
    return f"latency: control dt {ms:.6g} ms; " + "; ".join(
        f"{axis} {','.join(str(k) for k in lat[axis])} steps = {','.join(f'{k * ms:.6g}' for k in lat[axis])} ms" for axis in DELAY_AXES)


def actuator_option(args):
    """Player's `actuators` from the --actuators, --effort-frac, --vel-frac and --limit-margin options: False, True, or the dict of the
    thresholds that were given."""
    if not getattr(args, "actuators", False):
        return False
    given = {k: getattr(args, k, None) for k in ACT_THRESHOLDS}
    return {k: v for k, v in given.items() if v is not None} or True


def make_renderer(task, args):
    """The Renderer of the --capture-envs, --capture-size, --capture-samples (default 1) and --camera options."""
    from . import render
    try:
        width, height = (int(v) for v in args.capture_size.lower().split("x"))
        envs = [int(v) for v in args.capture_envs.split(",")]
    except ValueError as e:
        raise SystemExit(f"--capture-size is WIDTHxHEIGHT and --capture-envs a comma-separated list of env ids: {e}")
    renderer = render.Renderer(task, envs=envs, width=width, height=height, samples=getattr(args, "capture_samples", 1))
    if args.camera == "follow":
        renderer.set_camera(render.Camera.follow_root(renderer.scene))
    return renderer


def make_recorder(task, args):
    """The Recorder of the --capture* options."""
    from . import render
    deferred = bool(getattr(args, "capture_deferred", False) or getattr(args, "capture_trajectory", None))
    return render.Recorder(make_renderer(task, args), length=args.capture_len, every=args.capture_every, deferred=deferred)


def main(argv=None):
    args = parse_args(argv)
    import isaacgym_amd
    from .policy import RLGamesPolicy
    task_cfg = None
    if args.cfg_dir:
        from . import cfgyaml
        task_cfg = cfgyaml.compose(args.task, args.cfg_dir, overrides={"num_envs": args.num_envs})["task"]
    task = isaacgym_amd.make(seed=args.seed, task=args.task, num_envs=args.num_envs, cfg=task_cfg)
    policy = RLGamesPolicy.load(args.checkpoint, task.device)
    recorder = make_recorder(task, args) if args.capture or args.capture_trajectory else None
    sweep = Sweep.parse(args.sweep, paired=getattr(args, "paired", False)) if getattr(args, "sweep", None) else None
    against = getattr(args, "against", None) or []
    paired_diff, baseline = bool(getattr(args, "paired_diff", False)), getattr(args, "baseline", None) or 0
    if against:                           # checkpoints x sweep cells, checkpoint-major; cell (k, c) against (0, c)
        paths = [args.checkpoint] + list(against)
        cells = sweep.cells if sweep is not None else [{}]
        nets = [policy] + [RLGamesPolicy.load(p, task.device) for p in against]
        policy = [net for net in nets for _ in cells]
        baseline = [c for _ in nets for c in range(len(cells))]
        sweep, paired_diff = Sweep(cells * len(nets), paired=True), True
        for k, p in enumerate(paths):
            print(f"checkpoint {k}: {p}", flush=True)
    pl = Player(task, policy, games_num=args.games, deterministic=not args.stochastic, seed=args.seed, poll_every=args.poll_every,
                max_steps=args.max_steps, sigma=args.sigma, recorder=recorder, outcomes=args.outcomes, sweep=sweep, paired_diff=paired_diff,
                baseline=baseline, actuators=actuator_option(args), action_delay=getattr(args, "action_delay", 0), obs_delay=getattr(args, "obs_delay", 0))
    last = dict(games=0, steps=0, reward=[0.0])

    def on_poll(tot):                     # rl_games prints `reward: ... steps: ...` per finished batch: here, the games since the last poll
        n = tot["games"] - last["games"]
        if n > 0:
            print(f"reward: {(tot['reward'][0] - last['reward'][0]) / n} steps: {(tot['steps'] - last['steps']) / n}", flush=True)
        last.update(games=tot["games"], steps=tot["steps"], reward=list(tot["reward"]))
        if args.outcomes:
            o = pl.read_outcomes()
            if o["windows"] > 0:
                print("\n".join(outcome_lines(o)), flush=True)

    res = pl.run(on_poll=on_poll)
    print(f"av reward: {res['av_reward']} av steps: {res['av_steps']}")
    if "latency" in res:
        print(latency_line(res["latency"]))
    if args.outcomes:
        print("\n".join(outcome_lines(res["outcomes"])) if res["outcomes"]["windows"] > 0 else "no env has reset: no outcome window yet")
    for a, p in enumerate(res["per_agent"]):
        print(f"agent {a}: games {res['games']} reward std {p['reward_std']:.6g} min {p['reward_min']:.6g} max {p['reward_max']:.6g} (av {p['av_reward']:.6g})")
    per_ckpt = len(res.get("groups", ())) // (1 + len(against))               # with --against: cell index -> checkpoint index
    for i, g in enumerate(res.get("groups", ())):
        print((f"checkpoint {i // per_ckpt} " if against else "") + group_line(g))
    if "paired_diff" in res:
        for p in res["paired_diff"]["cells"]:
            print(pair_line(p, res["groups"], res["paired_diff"]["episodes"] * (task.num_envs // len(res["groups"]))))
    if "actuators" in res:
        for g in res["actuators"]["groups"]:
            print(actuator_table(g, "cell " + cell_text(g["cell"])))
        if getattr(args, "actuators_out", None):
            with open(args.actuators_out, "w") as fh:
                json.dump(res["actuators"], fh, indent=1)
            print(f"wrote {args.actuators_out}")
    if getattr(args, "sweep_out", None):
        with open(args.sweep_out, "w") as fh:                                  # (a cell's latency axes are in its `cell`, as ints)
            json.dump(res["groups"], fh, indent=1)
        print(f"wrote {args.sweep_out}")
    if getattr(args, "paired_out", None):
        with open(args.paired_out, "w") as fh:
            json.dump(dict(res["paired_diff"], latency=res["latency"]) if "latency" in res else res["paired_diff"], fh, indent=1)
        print(f"wrote {args.paired_out}")
    print(f"{res['steps_played']} control steps x {task.num_envs} envs in {res['seconds']:.3f} s", flush=True)
    if recorder is not None and args.capture_trajectory:
        print(f"saved {recorder.trajectory.save(args.capture_trajectory, fps=args.capture_fps)} (trajectory)", flush=True)
    if recorder is not None and args.capture:
        files = recorder.save(args.capture, fps=args.capture_fps)
        print(f"captured {res['captured_frames']} frames, kept the last {min(res['captured_frames'], recorder.length)}: {files[0]}" +
              (f" .. {files[-1]}" if len(files) > 1 else ""), flush=True)
    return res


if __name__ == "__main__":
    main()
