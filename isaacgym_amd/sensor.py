"""Sensor noise and sample dropouts on the device: the sensor line (SensorLine; C ABI and the rule in full: include/ppenv_sensor.h), the
parsing of its arguments (an amplitude or probability S, a (lo, hi) range, the CLI's "S" or "LO:HI"; a column spec such as
"ball_pos=1,ball_vel=4,60:67=0.5"), and the rule restated in numpy (reference).  The rule is this build's own specification — the reference
adds no such noise and no oracle pins it.  play.Player(obs_noise=, obs_drop=, action_noise=, action_drop=) builds lines over a per-row table
(one value per sweep cell); RolloutCollector / PPOTrainer(obs_noise=, ...) build lines that draw their levels per episode on the device."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, scene

MAX_WIDTH = _lib.PLAY_DELAY_MAX_WIDTH
COMMAND, SENSING = 0, 1                    # PP_SENSOR_COMMAND, PP_SENSOR_SENSING
AXES = ("obs_noise", "obs_drop", "action_noise", "action_drop")

# The named column groups of the 80-wide observation row of the 7-dof and 4-actor tasks, from the row builder in
# isaacgym_amd/csrc/ppenv_device.h: write_obs_bodies (lines 1073-1084) stores the local body positions at 3 j and the local body velocities
# at 3 NB + 3 j, NB = 10 bodies; write_obs_tail (lines 1085-1097) stores the joint positions at 6 NB + d and the joint velocities at
# 6 NB + ND + d, ND = 7, then the local ball position at 6 NB + 2 ND .. + 2 and the local ball velocity at 6 NB + 2 ND + 3 .. + 5
# (80 = 30 + 30 + 7 + 7 + 3 + 3).  The 27-dof task's row builder (ppenv_ta_task.h) names no column groups: `all` and explicit ranges there.
OBS_GROUPS_7DOF = dict(body_pos=(0, 30), body_vel=(30, 60), dof_pos=(60, 67), dof_vel=(67, 74), ball_pos=(74, 77), ball_vel=(77, 80))
_VARIANTS_7DOF = ("T3", "TT", "TN", "T4")


def groups(task_or_variant, channel=SENSING):
    """The named column groups of a channel: a task object (its VARIANT), a variant string, or None -> {name: (lo, hi)}.  The command
    channel and the 27-dof task have none beyond `all`."""
    variant = getattr(task_or_variant, "VARIANT", task_or_variant)
    return dict(OBS_GROUPS_7DOF) if channel == SENSING and variant in _VARIANTS_7DOF else {}


def _parse(name, task_or_variant, spec, width, scales, channel):
    W = int(width)
    if not 1 <= W <= MAX_WIDTH:
        raise ValueError(f"{name}: width {width} is outside 1..{MAX_WIDTH}")
    named = groups(task_or_variant, channel)
    if named and W != scene.NUM_OBS:
        named = {}
    out = np.zeros(W, np.float32)
    text = "all" if spec is None or (isinstance(spec, str) and not spec.strip()) else spec
    if not isinstance(text, str):
        raise ValueError(f"{name}: a column spec is text such as 'ball_pos=1,60:67=0.5', not {spec!r}")
    for item in text.split(","):
        item = item.strip()
        what, eq, value = item.partition("=")
        what = what.strip()
        scale = 1.0
        if eq:
            if not scales:
                raise ValueError(f"{name}: {item!r}: these columns take no scale (NAME or LO:HI)")
            try:
                scale = float(value)
            except ValueError:
                scale = math.nan
            if not math.isfinite(scale) or scale < 0.0:
                raise ValueError(f"{name}: {item!r}: the scale {value.strip()!r} is not a finite number >= 0")
        if what == "all":
            lo, hi = 0, W
        elif what in named:
            lo, hi = named[what]
        elif ":" in what:
            try:
                lo, hi = (int(v.strip(), 10) for v in what.split(":"))
            except ValueError:
                raise ValueError(f"{name}: {item!r}: a range is LO:HI, two whole numbers") from None
            if not 0 <= lo < hi <= W:
                raise ValueError(f"{name}: {item!r}: the range {lo}:{hi} is not inside 0:{W} with LO < HI")
        else:
            raise ValueError(f"{name}: {item!r}: unknown column group {what!r}; the groups are {', '.join(['all'] + list(named))}, or a range LO:HI")
        out[lo:hi] = scale
    return out


def columns(task_or_variant, spec, width, channel=SENSING, name="columns"):
    """A column spec -> col_scale float32 [width].  spec: comma-separated NAME[=SCALE] or LO:HI[=SCALE] (HI exclusive; SCALE a finite
    number >= 0, default 1), applied left to right; NAME is `all` or one of groups(task_or_variant, channel).  None or "" is `all=1`;
    columns no item names get 0.  Anything else raises ValueError naming `name`."""
    return _parse(name, task_or_variant, spec, width, True, channel)


def hold_columns(task_or_variant, spec, width, channel=SENSING, name="hold_columns"):
    """The same parser without scales -> col_hold int32 [width]: 1 for the columns a dropout holds.  None or "" is `all`."""
    return (_parse(name, task_or_variant, spec, width, False, channel) != 0).astype(np.int32)


def check_specs(task_name, specs, flag=lambda key: key):
    """The four column specs dict(obs_noise_columns=, obs_drop_columns=, action_noise_columns=, action_drop_columns=) against the widths and
    column groups of the registered task `task_name`, before a task is built: a bad one raises ValueError naming flag(key).  A task name the
    registry does not know is left to make()."""
    variant = scene.TASK_VARIANTS.get(task_name)
    if variant is None:
        return
    widths = dict(obs=scene.TA_NUM_OBS if variant == "TA" else scene.NUM_OBS, action=scene.TA_NUM_DOF if variant == "TA" else scene.NUM_DOF)
    for path, channel in (("obs", SENSING), ("action", COMMAND)):
        columns(variant, specs.get(f"{path}_noise_columns"), widths[path], channel, name=flag(f"{path}_noise_columns"))
        hold_columns(variant, specs.get(f"{path}_drop_columns"), widths[path], channel, name=flag(f"{path}_drop_columns"))


def parse_range(name, value, top=math.inf):
    """An amplitude or probability argument -> (lo, hi), floats with 0 <= lo <= hi <= top, finite: a number S is (S, S); a (lo, hi) pair;
    the text "S" or "LO:HI" (the CLI's).  Anything else — negative, lo > hi, above top, not finite, a bool — raises ValueError naming
    `name`.  latency.delay_range's sibling."""
    def number(x):
        if isinstance(x, bool) or not isinstance(x, (int, float, str, np.integer, np.floating)):
            raise ValueError
        return float(x.strip()) if isinstance(x, str) else float(x)
    try:
        if isinstance(value, str):
            parts = value.split(":")
            if len(parts) not in (1, 2):
                raise ValueError
            lo, hi = (number(parts[0]),) * 2 if len(parts) == 1 else (number(parts[0]), number(parts[1]))
        elif isinstance(value, (tuple, list)):
            if len(value) != 2:
                raise ValueError
            lo, hi = number(value[0]), number(value[1])
        else:
            lo = hi = number(value)
        if not (0.0 <= lo <= hi <= top and math.isfinite(hi)):
            raise ValueError
    except (ValueError, TypeError, OverflowError):
        bound = "" if top == math.inf else f" <= {top:g}"
        raise ValueError(f"{name}: a number S or a range LO:HI / (lo, hi) with 0 <= lo <= hi{bound}, finite, not {value!r}") from None
    return lo, hi


def sigma_range(name, value):
    return parse_range(name, value)


def drop_range(name, value):
    return parse_range(name, value, 1.0)


def sensor_text(rec):
    """The record dict(obs_noise=[lo, hi], obs_drop=[lo, hi], action_noise=..., action_drop=..., columns={...}) -> the trainer's start-up line."""
    def one(r):
        lo, hi = r
        return f"{lo:.6g}" if lo == hi else f"{lo:.6g}..{hi:.6g}, drawn per episode"
    return "sensor: " + "; ".join(f"{axis} {one(rec[axis])}" for axis in AXES) + "".join(f"; {k} {v}" for k, v in rec.get("columns", {}).items() if v)


class SensorLine:
    """pp_sensor_reset / pp_sensor_push (include/ppenv_sensor.h) on torch tensors: additive Gaussian noise and sample dropouts for a
    [rows, width] float32 tensor.  Row r adds sigma[r] * col_scale[c] * N(0, 1) to column c, and with probability drop[r] per control step
    (never on an episode's first sample) delivers, in the col_hold columns, the values it delivered last instead.
    sigma, drop: a per-row array [rows] — the caller's table, never written by the kernel (draw = 0: play; the other of the two may then be
    one number for all rows) — or a number or a (lo, hi) range, drawn per row on the device at every episode start (draw = 1: training;
    scene.sensor_draws predicts the draws).
    columns: col_scale, a float array [width] >= 0 (sensor.columns(...)), default all ones; hold_columns: col_hold, an int array [width]
    of 0 / 1 (sensor.hold_columns(...)), default all ones.
    Every draw is keyed (seed, num_agents * (env_id_offset + env) + agent, the row's episode count, the step in the episode); with
    key_period = S env e is keyed as env e % S, so the S-env cells of a paired sweep see the same standard normals.  `seed` is a STREAM
    seed.  push(x, done, out) -> out; `done` ([rows] int64, the done the previous env step returned, or None right after reset()) marks the
    sample as the first of a new episode of its env (agent 0's word).  x is not modified and must not overlap out.  One launch per push,
    nothing here synchronises."""

    def __init__(self, rows, width, device, num_agents=1, sigma=0.0, drop=0.0, columns=None, hold_columns=None, seed=0, env_id_offset=0, key_period=0,
                 channel=SENSING):
        self.rows, self.width, self.num_agents = R, W, A = int(rows), int(width), int(num_agents)
        if R < 1 or A not in (1, 2) or R % A or not 1 <= W <= MAX_WIDTH:
            raise ValueError(f"SensorLine: rows {rows} (>= 1, a multiple of num_agents), num_agents {num_agents} (1 or 2), width {width} (1..{MAX_WIDTH})")
        if channel not in (COMMAND, SENSING):
            raise ValueError(f"SensorLine: channel {channel!r} is not 0 (the command path) or 1 (the sensing path)")
        self.seed, self.env_id_offset, self.key_period, self.channel = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_id_offset), int(key_period), int(channel)
        if not 0 <= self.env_id_offset <= 2 ** 31 - 1 - R // A:
            raise ValueError(f"SensorLine: env_id_offset {env_id_offset} (>= 0; the last env's id below 2^31)")
        if not 0 <= self.key_period <= 2 ** 31 - 1:
            raise ValueError(f"SensorLine: key_period {key_period} (0, or the envs per paired cell)")
        tables = [isinstance(v, (np.ndarray, torch.Tensor)) for v in (sigma, drop)]
        self.draw = 0 if any(tables) else 1                                # a per-row array makes both the caller's table: the other may be one number for all rows
        if not self.draw:
            if any(not t and (isinstance(v, (bool, tuple, list, str)) or v is None) for t, v in zip(tables, (sigma, drop))):
                raise ValueError("SensorLine: beside a per-row array the other of sigma / drop is a per-row array or one number, not a range (a table is never drawn)")
            sigma, drop = (v if t else np.full(R, float(v), np.float32) for t, v in zip(tables, (sigma, drop)))
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                       # tensors carry an index: compare like with like
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        if self.draw:
            self.sigma_range, self.drop_range = sigma_range("SensorLine: sigma", sigma), drop_range("SensorLine: drop", drop)
            self.sigma = torch.zeros(R, dtype=torch.float32, device=dev)
            self.drop = torch.zeros(R, dtype=torch.float32, device=dev)
        else:
            sg, dp = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float32).reshape(-1) for v in (sigma, drop))
            if sg.shape != (R,) or dp.shape != (R,) or not np.isfinite(sg).all() or (sg < 0).any() or not ((dp >= 0) & (dp <= 1)).all():
                raise ValueError(f"SensorLine: per-row tables are [{R}] arrays, sigma finite >= 0 and drop in [0, 1]")
            self.sigma_range, self.drop_range = (0.0, 0.0), (0.0, 0.0)
            self.sigma, self.drop = torch.from_numpy(sg.copy()).to(dev), torch.from_numpy(dp.copy()).to(dev)
        scale = np.ones(W, np.float32) if columns is None else np.asarray(columns, np.float32).reshape(-1)
        hold = np.ones(W, np.int32) if hold_columns is None else np.asarray(hold_columns).reshape(-1)
        if scale.shape != (W,) or not np.isfinite(scale).all() or (scale < 0).any():
            raise ValueError(f"SensorLine: columns is a [{W}] array of finite scales >= 0")
        if hold.shape != (W,) or not np.isin(hold, (0, 1)).all():
            raise ValueError(f"SensorLine: hold_columns is a [{W}] array of 0 / 1")
        self.col_scale, self.col_hold = torch.from_numpy(scale.copy()).to(dev), torch.from_numpy(hold.astype(np.int32)).to(dev)
        L = self.L = _lib.lib()
        self._consts = _lib.SensorConsts(self.sigma_range[0], self.sigma_range[1], self.drop_range[0], self.drop_range[1], self.draw, self.seed,
                                         self.env_id_offset, self.key_period, self.channel)
        self.age = torch.zeros(R, dtype=torch.int32, device=dev)
        self.episode = torch.zeros(R, dtype=torch.int32, device=dev)
        self.held = torch.zeros((R, W), dtype=torch.float32, device=dev)
        assert self.held.numel() * 4 == L.pp_sensor_held_bytes(R, W) and 4 * R == L.pp_sensor_table_bytes(R)
        self.reset()

    def reset(self):
        """age and episode to zero: every row's next sample is the first of its episode 0."""
        _lib.check(self.L.pp_sensor_reset(self.rows, self.age.data_ptr(), self.episode.data_ptr(), _lib.stream(self.device)), self.L)

    def _matrix(self, name, t):
        R, W = self.rows, self.width
        if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != (R, W) or (W > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < W):
            raise ValueError(f"SensorLine.push: {name} must be float32 [{R}, {W}] on {self.device} with unit stride along the row and a row stride >= {W}")
        return t.data_ptr(), t.stride(0) if R > 1 else W

    def push(self, x, done, out=None):
        """x, out: float32 [rows, width] on this device, unit stride along the row and a row stride >= width (contiguous tensors, or the
        first `width` columns of wider ones), not overlapping; out None: a buffer the line owns, overwritten by the next push.
        done: [rows] int64 contiguous, or None.  -> out."""
        if out is None:
            if getattr(self, "_out", None) is None:
                self._out = torch.empty((self.rows, self.width), dtype=torch.float32, device=self.device)
            out = self._out
        (px, ldx), (po, ldo) = self._matrix("x", x), self._matrix("out", out)
        if done is not None and (done.dtype != torch.int64 or done.numel() != self.rows or not done.is_contiguous() or done.device != self.device):
            raise ValueError(f"SensorLine.push: done must be int64, contiguous [{self.rows}] on {self.device}, or None")
        _lib.check(self.L.pp_sensor_push(px, ldx, _lib.ptr(done), self.rows, self.num_agents, self.width, C.byref(self._consts), self.col_scale.data_ptr(),
                                         self.col_hold.data_ptr(), self.sigma.data_ptr(), self.drop.data_ptr(), self.age.data_ptr(), self.episode.data_ptr(),
                                         self.held.data_ptr(), po, ldo, _lib.stream(self.device)), self.L)
        return out


class reference:
    """The header's rule in numpy, written from its words: uniforms bit for bit (scene.sensor_uniform), the level draws with
    scene.sensor_draws' arithmetic, Box-Muller in fp64.  One object is one channel; push(x, done) is one control step.
    sigma, drop: per-row float32 arrays (draw = 0) or (lo, hi) ranges (draw = 1).  x: float32 [rows, >= width] (only the first `width` columns
    are read).  push -> out float32 [rows, width]: a column whose s is zero is the input bit for bit, a noised one is
    float32(x + float64(s) * g) with g the fp64 Box-Muller normal.  After a push, beside the state (age, episode, sigma, drop, held):
    `dropped` bool [rows], and per delivered element `s` (the fp32 s it was noised with; 0: a copy), `g` (its fp64 standard normal) and
    `mag` (|x| + |s g| at the time it was produced) — for a held element, those of the sample it holds."""

    def __init__(self, rows, width, num_agents=1, sigma=0.0, drop=0.0, columns=None, hold_columns=None, seed=0, env_id_offset=0, key_period=0,
                 channel=SENSING):
        self.rows, self.width, self.A = R, W, A = int(rows), int(width), int(num_agents)
        self.seed, self.offset, self.period, self.channel = int(seed), int(env_id_offset), int(key_period), int(channel)
        self.draw = 0 if isinstance(sigma, np.ndarray) else 1
        if self.draw:
            self.sigma_range, self.drop_range = sigma_range("reference: sigma", sigma), drop_range("reference: drop", drop)
            self.sigma, self.drop = np.zeros(R, np.float32), np.zeros(R, np.float32)
        else:
            self.sigma, self.drop = np.array(sigma, np.float32).reshape(R), np.array(drop, np.float32).reshape(R)
        self.col_scale = np.ones(W, np.float32) if columns is None else np.asarray(columns, np.float32).reshape(W)
        self.col_hold = np.ones(W, bool) if hold_columns is None else np.asarray(hold_columns).reshape(W) != 0
        self.age, self.episode = np.zeros(R, np.int32), np.zeros(R, np.int32)
        self.held = np.zeros((R, W), np.float32)
        self._held_s, self._held_g, self._held_mag = np.zeros((R, W), np.float32), np.zeros((R, W)), np.zeros((R, W))
        r = np.arange(R, dtype=np.int64)
        e = r // A
        self.key = (A * (self.offset + (e % self.period if self.period else e)) + r % A) & 0xFFFFFFFF

    def reset(self):
        self.age[:] = 0
        self.episode[:] = 0

    def push(self, x, done=None):
        R, W, A, f32 = self.rows, self.width, self.A, np.float32
        x = np.ascontiguousarray(np.asarray(x)[:, :W], f32)
        a = self.age.astype(np.int64)
        if done is not None:
            a = np.where(np.repeat(np.asarray(done).reshape(-1, A)[:, 0] != 0, A), 0, a)
        first = a == 0
        n = np.where(first, self.episode, self.episode - 1).astype(np.int64)
        self.episode[first] += 1
        if self.draw and first.any():
            u0, u1 = (scene.sensor_uniform(self.seed, self.channel, scene.SENSOR_LEVEL, self.key[first], n[first], k) for k in (0, 1))
            (s_lo, s_hi), (d_lo, d_hi) = (tuple(f32(v) for v in rng) for rng in (self.sigma_range, self.drop_range))
            self.sigma[first] = s_lo + ((s_hi - s_lo) * u0).astype(f32)
            self.drop[first] = d_lo + ((d_hi - d_lo) * u1).astype(f32)
        u_drop = scene.sensor_uniform(self.seed, self.channel, scene.SENSOR_DROP, self.key, n, a)
        self.dropped = (a > 0) & (self.drop > 0) & (u_drop < self.drop)
        P = (W + 1) >> 1
        col = np.arange(W, dtype=np.int64)
        k = 2 * (a[:, None] * P + (col >> 1)[None, :])
        u1 = scene.sensor_uniform(self.seed, self.channel, scene.SENSOR_NOISE, self.key[:, None], n[:, None], k).astype(np.float64)
        u2 = scene.sensor_uniform(self.seed, self.channel, scene.SENSOR_NOISE, self.key[:, None], n[:, None], k + 1).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(np.maximum(u1, 2.0 ** -24)))
        g = np.where((col & 1)[None, :] != 0, rad * np.sin(2.0 * np.pi * u2), rad * np.cos(2.0 * np.pi * u2))
        s = (self.sigma[:, None] * self.col_scale[None, :]).astype(f32)
        with np.errstate(invalid="ignore"):
            sg = s.astype(np.float64) * g
            noised = (x.astype(np.float64) + sg).astype(f32)
            mag = np.abs(x.astype(np.float64)) + np.abs(sg)
        out = np.where(s == 0, x.view(np.uint32), noised.view(np.uint32)).view(f32)          # a copy moves bits: NaN payloads and -0.0 survive
        g = np.where(s == 0, 0.0, g)
        hold_read = self.dropped[:, None] & self.col_hold[None, :]
        hold_write = ~self.dropped[:, None] & self.col_hold[None, :]
        out = np.where(hold_read, self.held.view(np.uint32), out.view(np.uint32)).view(f32)
        self.s, self.g, self.mag = np.where(hold_read, self._held_s, s), np.where(hold_read, self._held_g, g), np.where(hold_read, self._held_mag, mag)
        self.held = np.where(hold_write, out.view(np.uint32), self.held.view(np.uint32)).view(f32)
        self._held_s, self._held_g, self._held_mag = (np.where(hold_write, new, old) for new, old in ((self.s, self._held_s), (self.g, self._held_g), (self.mag, self._held_mag)))
        self.age = (a + 1).astype(np.int32)
        self.out = out
        return out
