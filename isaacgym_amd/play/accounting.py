"""The player's device-side objects: the episode accounting (GroupStats, EpisodeStats), the paired statistics (PairStats), the actuator
usage (ActuatorStats) and the control-latency delay line (Delay), each a thin owner of torch tensors around its C ABI."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import PlayPairTotals, PlayTotals
from .report import act_totals_dict, pair_totals_dict, totals_dict

MAX_GROUPS = 1024                          # PP_PLAY_GROUP_MAX
ACT_THRESHOLDS = dict(effort_frac=0.98, vel_frac=0.98, limit_margin=0.02)     # Player(actuators=True)'s; action_clip is the task's clipActions
DELAY_MAX, DELAY_MAX_WIDTH = _lib.PLAY_DELAY_MAX, _lib.PLAY_DELAY_MAX_WIDTH


def _check_rew_done(owner, method, rew, done, rows, device, tail=""):
    """What every accounting launch asks of VecTask.step's rew_buf / reset_buf: rew float32, done int64, both contiguous with `rows`
    elements on `device`; rew None: done alone.  owner, method: whose check it is, for the message ('GroupStats.accumulate: ...')."""
    if rew is None:
        if done.dtype != torch.int64 or done.numel() != rows or not done.is_contiguous() or done.device != device:
            raise ValueError(f"{type(owner).__name__}.{method}: done must be int64, contiguous [{rows}] on {device}{tail}")
    elif rew.dtype != torch.float32 or done.dtype != torch.int64 or rew.numel() != rows or done.numel() != rows or \
            not rew.is_contiguous() or not done.is_contiguous() or rew.device != device or done.device != device:
        raise ValueError(f"{type(owner).__name__}.{method}: rew must be float32 and done int64, contiguous [{rows}] on {device}")


def _read_structs(T, buf, n):
    """A byte tensor holding n structs of the ctypes type T -> a list of n T, from one host copy (the stream is waited for)."""
    raw, size = buf.cpu().numpy().tobytes(), C.sizeof(T)
    return [T.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]


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
        _check_rew_done(self, "accumulate", rew, done, self.rows, self.device)
        _lib.check(self.L.pp_play_group_accumulate(rew.data_ptr(), done.data_ptr(), self.envs_per_group, self.groups, self.num_agents, self.games_num,
                                                   self.cur_reward.data_ptr(), self.cur_steps.data_ptr(), self._totals.data_ptr(),
                                                   self._partial.data_ptr(), _lib.stream(self.device)), self.L)

    def read_groups(self):
        """One host copy of the `groups` structs (groups x 72 bytes; the stream is waited for) -> a list of totals_dict, in group order."""
        return [totals_dict(t, self.num_agents) for t in _read_structs(PlayTotals, self._totals, self.groups)]

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
        A = _lib.MAX_AGENTS
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


class PairStats:
    """pp_play_pair_reset / _record / _reduce (include/ppenv_play_pair.h) on torch tensors: for `groups` cells of `envs_per_group` envs
    that are served the same balls, the returns and lengths of the first `episodes` episodes of every env, and read(): per cell the fp64
    sums of the paired difference against cell baseline[g].  baseline: one cell index for all cells, or a sequence of `groups` of them.
    One launch per record(), nothing here synchronises except read() (one more launch and one host copy of groups x 80 bytes)."""

    def __init__(self, envs_per_group, groups, num_agents, episodes, baseline, device):
        from .sweep import baseline_cells                                  # (sweep takes MAX_GROUPS and DELAY_MAX from this module)
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
        _check_rew_done(self, "record", rew, done, self.rows, self.device)
        _lib.check(self.L.pp_play_pair_record(rew.data_ptr(), done.data_ptr(), *self._sizes(), *self._state(), _lib.stream(self.device)), self.L)

    def _launch_reduce(self):
        _lib.check(self.L.pp_play_pair_reduce(*self._sizes(), self._baseline.data_ptr(), self.count.data_ptr(), self.ret.data_ptr(), self.len.data_ptr(),
                                              self._out.data_ptr(), _lib.stream(self.device)), self.L)

    def reduce(self):
        """The reduce launch alone: the `groups` structs as host bytes (the stream is waited for)."""
        self._launch_reduce()
        return self._out.cpu().numpy().tobytes()

    def read(self):
        """-> a list of pair_totals_dict, in cell order, each with its `cell` and `baseline` index."""
        self._launch_reduce()
        return [dict(pair_totals_dict(t, self.num_agents), cell=g, baseline=self.baseline[g])
                for g, t in enumerate(_read_structs(PlayPairTotals, self._out, self.groups))]

    def state_bytes(self):
        """cur_reward, cur_steps, count, ret and len as host bytes (the tests compare them)."""
        return tuple(t.cpu().numpy().tobytes() for t in (self.cur_reward, self.cur_steps, self.count, self.ret, self.len))


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
        _check_rew_done(self, "accumulate", None, done, self.num_envs * self.num_agents, self.device)
        ins = _lib.PlayActInputs(self._input("q", q), self._input("qd", qd), self._input("tau", tau), self._input("action", action))
        _lib.check(self.L.pp_play_act_accumulate(C.byref(ins), done.data_ptr(), self.envs_per_group, self.groups, self.num_agents, self.num_dofs, self.games_num,
                                                 self._limits.data_ptr(), C.byref(self._thr), self._state.data_ptr(), self._group.data_ptr(),
                                                 self._joint.data_ptr(), self._partial.data_ptr(), _lib.stream(self.device)), self.L)

    def read(self):
        """One host copy of the totals (the stream is waited for) -> a list of act_totals_dict, in group order."""
        G, D = self.groups, self.num_dofs
        groups, joints = _read_structs(_lib.PlayActGroup, self._group, G), _read_structs(_lib.PlayActJoint, self._joint, G * D)
        return [act_totals_dict(groups[g], joints[g * D:(g + 1) * D]) for g in range(G)]

    def state_bytes(self, state=True):
        """The running state, the G group structs and the G * D joint structs as host bytes (the tests compare them)."""
        return (self._state.cpu().numpy().tobytes() if state else b"", self._group.cpu().numpy().tobytes(), self._joint.cpu().numpy().tobytes())

    def partial_bytes(self):
        """The last launch's per-chunk partials as host bytes: G * parts group structs, then G * parts * D joint structs."""
        return self._partial.cpu().numpy().tobytes()


class Delay:
    """pp_play_delay_reset / pp_play_delay_push (include/ppenv_play_delay.h) on torch tensors: a delay line of whole control steps for a
    [rows, width] float32 tensor, row r delayed by delays[r] (an int array [rows], 0 .. 15) — push(x, done) stores this control step's
    sample and returns the one delays[r] steps old of the same episode, or the episode's first sample while there is none that old;
    `done` ([rows] int64, the done the previous env step returned, or None right after reset()) marks the sample as the first of a new
    episode of its env (agent 0's word, as everywhere in this package).  It owns the ring [max(delays) + 1, rows, width], the ages and the
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
        if done is not None:
            _check_rew_done(self, "push", None, done, R, self.device, tail=", or None")
        _lib.check(self.L.pp_play_delay_push(x.data_ptr(), x.stride(0) if R > 1 else W, _lib.ptr(done), R, self.num_agents, W, self.depth, self._delay.data_ptr(),
                                             self.age.data_ptr(), self.ring.data_ptr(), self.out.data_ptr(), W, _lib.stream(self.device)), self.L)
        return self.out
