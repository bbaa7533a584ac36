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

The package, one concern per file: accounting (the device-side objects: GroupStats, EpisodeStats, PairStats, ActuatorStats, Delay), report
(host arithmetic and text, no device access), sweep (Sweep: the cells and their three kinds of axes), player (Player: the loop), cli
(the options, main).  Everything public is importable from here.

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

Training under latency is the trainer's: PPOTrainer(action_delay=, obs_delay=) with isaacgym_amd.latency.DelayLine (include/ppenv_train_delay.h),
fixed or drawn per episode, in this player's order — a fixed delay trains under exactly what the sweep axes above measure.

Observation and action history.  A checkpoint trained with PPOTrainer(history=) carries a "history" record (include/ppenv_history.h); there is no
play flag, the checkpoint decides.  The player then stacks the seen observations and the policy's own last actions on the device, one launch per
control step and distinct record (history.HistoryStack.advance, after the sensing line, before the policy), and the result gains `history`.
With --against a history checkpoint and a plain one play the same balls in one pass.  Without such a checkpoint nothing is built.

Sensor noise and dropouts.  `--obs-noise S --obs-drop P --action-noise S --action-drop P`, or the sweep axes obs_noise, obs_drop, action_noise,
action_drop (`--sweep obs_noise=0,0.01,0.02 --paired`): a sensor line on the sensing path and one on the command path (isaacgym_amd.sensor.SensorLine;
include/ppenv_sensor.h holds the rule) add per-cell Gaussian noise with a per-column scale and drop samples with a per-cell probability, holding
the last delivered values; `--obs-noise-columns "ball_pos=1,ball_vel=4"` and `--obs-drop-columns ball_pos,ball_vel` say which columns (the camera's,
say) — NAME[=SCALE] or LO:HI[=SCALE], default all.  One launch per line and control step, keyed (seed, env, episode, step): with --paired the cells
see the same standard normals and drop draws.  The sensing line comes before the observation delay, the command line after the action delay; the
env's own clamp still applies.  The result gains `sensor`, the summary a `sensor:` line, and --sweep-out / --paired-out carry the axes in each
`cell`.  A line whose levels are all zero is not built.  This is not the step kernels' by-value noise (one amplitude per simulation): those stay.

Out of scope: sensor levels drawn per episode in the player (fixed-level sweeps evaluate a policy trained under drawn ones, as with delays),
correlated or coloured noise, bias, drift, quantisation; delays drawn per episode in the player (fixed-delay sweeps evaluate a policy trained under them), action hold / policy decimation,
a VecTask-level latency setting; sweeping noise amplitudes or gravity (one by-value constant per simulation: several passes), per-group outcome counts,
paired sampler noise, anything in the trainer; capturing the play loop in a HIP graph (VecTask.step cannot be captured); multi-rank play; the rl_games
`Runner` / `player_factory` shim (rl_games itself is absent); mp4 output (a run is captured to GIF / PNG / npy: `Player(recorder=...)`,
`--capture`, isaacgym_amd.render); the observer, PBT and W&B hooks.
"""
from .. import serve                                                     # noqa: F401  (every name below is part of isaacgym_amd.play's surface)
from .._lib import MAX_AGENTS, PlayTotals     # PPENV_PLAY_MAX_AGENTS and the ctypes mirror of ppenv_play_totals (bound in _lib.load)
from .._lib import PlayPairTotals             # ... and of pp_play_pair_totals
from .._lib import TA_OUTCOME_NAMES, TAOutcome
from ..dr import TABLE_NAMES
from ..latency import DelayLine               # the trainer's line (delays drawn per episode), beside the player's Delay
from .accounting import ACT_THRESHOLDS, DELAY_MAX, DELAY_MAX_WIDTH, MAX_GROUPS, ActuatorStats, Delay, EpisodeStats, GroupStats, PairStats
from .cli import actuator_option, main, make_recorder, make_renderer, parse_args
from .player import Player, actuator_limits, control_dt_of
from .report import (ACT_INT_FIELDS, ACT_MAX_FIELDS, ACT_SUM_FIELDS, OUTCOME_PRINTS, act_totals_dict, actuator_summary, actuator_table, cell_text,
                     group_line, group_summary, latency_line, outcome_lines, outcomes_dict, pair_line, pair_summary, pair_totals_dict, sum_act_totals,
                     sensor_line, sum_totals, summarize, totals_dict)
from .sweep import DELAY_AXES, SENSOR_AXES, SERVE_AXES, Sweep, baseline_cells, delay_steps, sensor_level
