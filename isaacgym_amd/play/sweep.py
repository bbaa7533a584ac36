"""The cells of a sweep: what each group of envs plays under — table scales, serve axes, latency axes, sensor axes — classified once, at
construction."""
import itertools
import math
import re

import numpy as np

from .. import sensor, serve
from ..dr import TABLE_NAMES
from .accounting import DELAY_MAX, MAX_GROUPS

_AXIS = re.compile(r"^([A-Za-z_]\w*)(?:\[(\d+)\])?$")


SERVE_AXES = serve.AXES_27DOF              # serve_speed, serve_tilt, serve_tilt_z; ball_y, ball_z (27-dof task only)
DELAY_AXES = ("action_delay", "obs_delay")  # control latency in whole control steps: the command path, the sensing path
SENSOR_AXES = sensor.AXES                   # obs_noise, obs_drop, action_noise, action_drop: a noise amplitude (>= 0) or a dropout probability (0 .. 1)


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


def cell_delays(cells, action_delay=0, obs_delay=0):
    """cells: one dict per cell, its latency entries already whole steps ([{}]: a player without a sweep)
    -> {axis: [per cell, the cell's value or the keyword's]} for the two latency axes."""
    default = dict(action_delay=delay_steps("action_delay", action_delay), obs_delay=delay_steps("obs_delay", obs_delay))
    return {axis: [int(cell.get(axis, default[axis])) for cell in cells] for axis in DELAY_AXES}


def sensor_level(axis, v):
    """A sensor value -> the float: an amplitude >= 0 on a *_noise axis, a probability in [0, 1] on a *_drop axis, finite.  Anything else —
    negative, a (lo, hi) range, a bool — raises ValueError naming the axis."""
    top = 1.0 if axis.endswith("_drop") else math.inf
    try:
        ok = not isinstance(v, (bool, tuple, list, str)) and math.isfinite(float(v)) and 0.0 <= float(v) <= top
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"sweep axis {axis!r}: " + ("a dropout probability is a number in 0..1" if top == 1.0 else "a noise amplitude is a finite number >= 0") + f", not {v!r}")
    return float(v)


def cell_sensors(cells, obs_noise=0.0, obs_drop=0.0, action_noise=0.0, action_drop=0.0):
    """cells: one dict per cell, its sensor entries already floats ([{}]: a player without a sweep)
    -> {axis: [per cell, the cell's value or the keyword's]} for the four sensor axes."""
    default = {axis: sensor_level(axis, v) for axis, v in zip(SENSOR_AXES, (obs_noise, obs_drop, action_noise, action_drop))}
    return {axis: [float(cell.get(axis, default[axis])) for cell in cells] for axis in SENSOR_AXES}


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


def _axis(axis):
    """'name' or 'name[row]' -> (table name, row or None), or (serve axis, None), or (latency axis, None), or (sensor axis, None); a name
    that is none of these raises ValueError."""
    if isinstance(axis, str) and (axis in SERVE_AXES or axis in DELAY_AXES or axis in SENSOR_AXES):
        return axis, None
    m = _AXIS.match(axis) if isinstance(axis, str) else None
    if m is None or m.group(1) not in TABLE_NAMES:
        raise ValueError(f"sweep axis {axis!r}: an axis is one of {', '.join(TABLE_NAMES)}, or one row of a table as name[row], or a sensor axis: "
                         f"{', '.join(SENSOR_AXES)}, or a serve axis: {', '.join(SERVE_AXES)}, or a latency axis in whole control steps: {', '.join(DELAY_AXES)}")
    return m.group(1), None if m.group(2) is None else int(m.group(2))


def _split(cell):
    """One cell {axis: value} -> (the cell with its values normalised, its table entries [(axis as written, table name, row or None,
    scale)], its serve entries {axis: value}, its latency entries {axis: steps}, its sensor entries {axis: level}); an axis or a value
    that is none of these raises ValueError."""
    norm, tables, serves, latency, sensors = {}, [], {}, {}, {}
    for axis, v in cell.items():
        name, row = _axis(axis)
        if name in SERVE_AXES:
            lo, hi = serve.value_range(axis, v)
            norm[axis] = serves[axis] = lo if lo == hi else (lo, hi)
        elif name in DELAY_AXES:
            norm[axis] = latency[axis] = delay_steps(axis, v)
        elif name in SENSOR_AXES:
            norm[axis] = sensors[axis] = sensor_level(axis, v)
        else:
            norm[axis] = scale = float(v)
            if not math.isfinite(scale) or scale < 0.0:
                raise ValueError(f"sweep axis {axis!r}: the scale {v!r} is not a finite number >= 0")
            tables.append((axis, name, row, scale))
    return norm, tables, serves, latency, sensors


class Sweep:
    """G cells of physical parameters, one per group of envs.  A cell maps an axis to one scalar scale; an axis is a table of
    dr.Randomizable.set_randomization (`friction_scale`: every row of it) or one row of one (`dof_stiffness_scale[5]`, which wins over
    the plain axis of the same table in that row).  What a cell does not name stays 1.0.
    A SERVE axis (SERVE_AXES: serve_speed, serve_tilt, serve_tilt_z in degrees; ball_y, ball_z on the 27-dof task) maps to a number — the
    quantity is pinned, and may be negative — or a (lo, hi) range it is drawn from; what a cell does not name is the task's configured range.
    A LATENCY axis (DELAY_AXES: action_delay, obs_delay) maps to a whole number of control steps 0 .. 15 — how old the command the env
    consumes, or the observation the policy sees, is (Delay; Player) — and is seen by neither tables() nor serve_cells(); what a cell does
    not name is the Player's keyword (default 0).
    A SENSOR axis (SENSOR_AXES: obs_noise, action_noise — a noise amplitude >= 0; obs_drop, action_drop — a dropout probability 0 .. 1)
    is what the player's sensor lines (isaacgym_amd.sensor.SensorLine; include/ppenv_sensor.h) add to the observations the policy sees and
    to the commands the env consumes; seen by neither tables() nor serve_cells(); what a cell does not name is the Player's keyword.
    paired: env i of every group is served the same sequence of balls (a serve plan keyed by the index within the group), with or
    without a serve axis.
    `cells` is the list of plain dicts, values normalised (a scale a float, a pinned serve a float, a ranged one (lo, hi), a delay an int);
    beside it, per cell and by kind: `cell_tables` [(axis as written, table name, row or None, scale)], `cell_serves` {axis: value} and
    `cell_latency` {axis: steps} and `cell_sensors` {axis: level} — what tables(), serve_cells(), cell_delays() / delays() and
    cell_sensors() each read, and nothing else."""

    def __init__(self, cells, paired=False):
        cells = [dict(c) for c in cells]
        self.paired = bool(paired)
        if not 1 <= len(cells) <= MAX_GROUPS:
            raise ValueError(f"a sweep has 1..{MAX_GROUPS} cells, not {len(cells)}")
        self.cells, self.cell_tables, self.cell_serves, self.cell_latency, self.cell_sensors = (list(kind) for kind in zip(*(_split(cell) for cell in cells)))
        self.needs_serve_plan = self.paired or any(self.cell_serves)      # serve_cells() is not None: the player sets a serve plan
        self.has_latency = any(self.cell_latency)                         # some cell names a latency axis
        self.has_sensors = any(self.cell_sensors)                         # some cell names a sensor axis

    def __len__(self):
        return len(self.cells)

    @property
    def sets_randomization(self):
        """Whether the player hands tables() to set_randomization(), so that the step runs the table-reading kernel.  A sweep that names a
        table does, of course.  One that is only about the serves (a serve axis, or paired), latency or the sensors leaves the physics alone
        and keeps the plain step kernel.  A sweep that is about nothing at all — unpaired, its cells empty — does too, with no tables: it
        is the sweep whose every scale is 1.0, and plays under the same kernel as any other sweep of scales."""
        return any(self.cell_tables) or not (self.needs_serve_plan or self.has_latency or self.has_sensors)

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
        if not self.needs_serve_plan:
            return None
        return serve.resolve_cells(self.cell_serves, defaults, tuple(defaults))

    def _envs_per_cell(self, num_envs):
        G, N = len(self.cells), int(num_envs)
        if N < G or N % G:
            below = N // G * G
            raise ValueError(f"a sweep of {G} cells needs a multiple of {G} envs, not {N}: the nearest are " +
                             (f"{below} and {below + G}" if below > 0 else f"{G}"))
        return N // G

    def cell_delays(self, action_delay=0, obs_delay=0):
        """-> {axis: [per cell, the cell's value or the keyword's]} for the two latency axes."""
        return cell_delays(self.cell_latency, action_delay, obs_delay)

    def sensor_levels(self, obs_noise=0.0, obs_drop=0.0, action_noise=0.0, action_drop=0.0):
        """-> {axis: [per cell, the cell's value or the keyword's]} for the four sensor axes."""
        return cell_sensors(self.cell_sensors, obs_noise, obs_drop, action_noise, action_drop)

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
            for g, entries in enumerate(self.cell_tables):
                for axis, name, row, v in entries:
                    if (row is None) != plain:
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
