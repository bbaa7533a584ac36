"""Automatic domain randomisation (ADR) of an environment handle (include/ppenv_dr_adr.h): a device-resident curriculum over the RANGES of
reset-time domain randomisation.  Every randomised table has a current [lo, hi]; a share of the envs (`boundary_frac`) play a whole game
pinned to one boundary of one table; finished games are credited to that boundary; once per epoch every boundary whose games score at or
above `t_high` moves outward by its `step`, every one whose games score at or below `t_low` moves back in.  After OpenAI's ADR and
DeXtreme; the rule is this project's own specification (the header states it).

`AutoRandomizer` is a curriculum.HorizonStage, as curriculum.ServeCurriculum is: the tables (handed to env.set_randomization), the per-env
and per-slot state and the launches of its own — one per control step (`step`), one per epoch (`update`) — over the base's staging rows of
one horizon and its `fold`.  torch owns the memory; nothing here reads the device on the host."""
import ctypes as C
import math

import torch

from . import _lib, dr, scene
from .curriculum import HorizonStage


def check_parameters(boundary_frac, min_games, t_low, t_high):
    """-> (boundary_frac, min_games, t_low, t_high) as the library takes them; ValueError, naming the argument, outside boundary_frac
    [0, 1], min_games >= 1 (an integer), t_low <= t_high both finite."""
    try:
        boundary_frac = float(boundary_frac)
    except (TypeError, ValueError):
        boundary_frac = math.nan
    if not (math.isfinite(boundary_frac) and 0.0 <= boundary_frac <= 1.0):
        raise ValueError(f"adr boundary_frac {boundary_frac!r}: a number in [0, 1]")
    if isinstance(min_games, bool) or not isinstance(min_games, int) or not 1 <= min_games < 2 ** 31:
        raise ValueError(f"adr min_games {min_games!r}: an integer >= 1")
    try:
        t_low, t_high = float(t_low), float(t_high)
    except (TypeError, ValueError):
        t_low = t_high = math.nan
    f32max = 3.4028234663852886e38
    if not (math.isfinite(t_low) and abs(t_low) <= f32max):
        raise ValueError(f"adr t_low {t_low!r}: a finite fp32 number")
    if not (math.isfinite(t_high) and abs(t_high) <= f32max):
        raise ValueError(f"adr t_high {t_high!r}: a finite fp32 number")
    if t_low > t_high:
        raise ValueError(f"adr t_low {t_low!r} above t_high {t_high!r}")
    return boundary_frac, min_games, t_low, t_high


def check_dims(dims, table_rows=None):
    """{table name: dict(start=(lo, hi), limit=(lo, hi), step=x)} -> the same with floats, in dr.TABLE_NAMES' order (the order enters the
    RNG key, as a reset-time plan's does).  ValueError, naming the table and the field: an unknown table (or one `table_rows` — an env's
    DR_TABLE_ROWS — does not have), a missing or non-finite field, step <= 0, limit lo <= 0, or not limit lo <= start lo <= start hi <=
    limit hi."""
    dims = dict(dims or {})
    if not dims:
        raise ValueError("adr dims: at least one table")
    known = dr.TABLE_NAMES if table_rows is None else tuple(table_rows)
    unknown = [k for k in dims if k not in known]
    if unknown:
        raise ValueError(f"adr dims: no table {unknown[0]!r} (one of {', '.join(known)})")
    out = {}
    for name in (n for n in dr.TABLE_NAMES if n in dims):
        spec = dims[name]
        try:
            if set(spec) != {"start", "limit", "step"}:
                raise KeyError
            (s0, s1), (l0, l1), step = (float(v) for v in spec["start"]), (float(v) for v in spec["limit"]), float(spec["step"])
        except (TypeError, ValueError, KeyError):
            raise ValueError(f"adr dim {name!r}: expected dict(start=(lo, hi), limit=(lo, hi), step=x), not {spec!r}") from None
        for field, v in (("start lo", s0), ("start hi", s1), ("limit lo", l0), ("limit hi", l1), ("step", step)):
            if not math.isfinite(v):
                raise ValueError(f"adr dim {name!r}: {field} {v!r} is not finite")
        if not step > 0.0:
            raise ValueError(f"adr dim {name!r}: step {step!r} must be above 0")
        if not l0 > 0.0:
            raise ValueError(f"adr dim {name!r}: limit lo {l0!r} must be above 0 (a scaling)")
        if not l0 <= s0 <= s1 <= l1:
            raise ValueError(f"adr dim {name!r}: not limit lo <= start lo <= start hi <= limit hi ({l0!r}, {s0!r}, {s1!r}, {l1!r})")
        out[name] = dict(start=(s0, s1), limit=(l0, l1), step=step)
    return out


def parse(flags):
    """The CLI form: ["link_mass_scale=1:1:0.6:1.4:0.05", ...] -> {table: dict(start, limit, step)} (a table given twice: the last one)."""
    out = {}
    for flag in flags or ():
        name, sep, v = str(flag).partition("=")
        parts = v.split(":")
        try:
            if not sep or len(parts) != 5:
                raise ValueError
            x = [float(p) for p in parts]
        except ValueError:
            raise ValueError(f"--adr {flag!r}: expected TABLE=START_LO:START_HI:LIMIT_LO:LIMIT_HI:STEP") from None
        out[name.strip()] = dict(start=(x[0], x[1]), limit=(x[2], x[3]), step=x[4])
    return out


class AutoRandomizer(HorizonStage):
    def __init__(self, env, dims, boundary_frac=0.25, min_games=256, t_low=0.0, t_high=0.0, seed=None, horizon=32):
        """env: a PPEnv or TAEnv with no randomisation set.  dims: {table name: dict(start=(lo, hi), limit=(lo, hi), step=x)}, the names
        dr.TABLE_NAMES, the row counts env.DR_TABLE_ROWS.  t_low, t_high: mean returns (agent 0's, unscaled) at or below / above which a
        boundary narrows / widens.  seed: a STREAM seed, default scene.stream_seed(the handle's seed, scene.STREAM_TABLES).  horizon: the
        rows of the staging buffers, the H of step(t).  Allocates the tables filled with 1, hands them over with env.set_randomization,
        uploads the struct, zeroes the state and fills every env's columns from the starts."""
        if env.dr_tables is not None or getattr(env, "reset_randomization", None) is not None:
            raise ValueError("the env already has randomisation tables or a reset-time plan set: call env.clear_randomization() first")
        self.boundary_frac, self.min_games, self.t_low, self.t_high = check_parameters(boundary_frac, min_games, t_low, t_high)
        self.dims = check_dims(dims, env.DR_TABLE_ROWS)
        tgt = env.serve_target()                                   # the handle's reset_rows and env_id_offset
        self.L, self.device, self.num_envs, self.num_agents = env.L, torch.device(env.device), int(env.num_envs), int(env.num_agents)
        self.reset_rows, self.env_id_offset, self.horizon = int(tgt["reset_rows"]), int(tgt["env_id_offset"]), int(horizon)
        if seed is None:
            seed = scene.stream_seed(env.config.seed if hasattr(env, "config") else env.params.seed, scene.STREAM_TABLES)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.names = list(self.dims)
        n, D, dev = self.num_envs, len(self.names), self.device
        self.D, self.slots = D, 2 * D + 1
        self.thr = int(math.floor(self.boundary_frac * 16777216.0))
        self.tables = {}
        for name in self.names:
            rows = env.DR_TABLE_ROWS[name]
            self.tables[name] = torch.ones((rows, n) if rows else (n,), dtype=torch.float32, device=dev)
        self.rows = [max(int(env.DR_TABLE_ROWS[name]), 1) for name in self.names]
        z = lambda *shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        S = self.slots
        self.range = z(D, 2, dt=torch.float32)
        self.draws, self.slot, self.ret = z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.float32)
        self.acc_n, self.acc_q, self.games, self.dropped = (z(S, dt=torch.int64) for _ in range(4))
        self.mean, self.widened, self.narrowed = z(S, dt=torch.float32), z(S, dt=torch.int32), z(S, dt=torch.int32)
        self.fin_slot = self._staging(S)
        self._state = _lib.AdrState(*(t.data_ptr() for t in (self.range, self.draws, self.slot, self.ret, self.acc_n, self.acc_q, self.games, self.dropped,
                                                             self.mean, self.widened, self.narrowed)))
        host = _lib.Adr(num_envs=n, env_id_offset=self.env_id_offset, seed=self.seed, reset_rows=self.reset_rows, num_agents=self.num_agents, dims=D, thr=0,
                        min_games=self.min_games, t_low=self.t_low, t_high=self.t_high)
        for m, name, rows in zip(host.dim, self.names, self.rows):
            spec = self.dims[name]
            m.table, m.rows = self.tables[name].data_ptr(), rows
            (m.start_lo, m.start_hi), (m.limit_lo, m.limit_hi), m.step = spec["start"], spec["limit"], spec["step"]
        self.adr_dev = z(C.sizeof(_lib.Adr), dt=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(self.L.pp_dr_adr_upload(C.byref(host), self.boundary_frac, self.adr_dev.data_ptr(), _lib.stream(dev)), self.L)
        env.set_randomization(**self.tables)
        self.fill()

    def fill(self):
        """range = the starts; every env's columns drawn from them, slot = -1, ret = 0 (pp_dr_adr_fill)."""
        _lib.check(self.L.pp_dr_adr_fill(self.adr_dev.data_ptr(), self.num_envs, self.D, C.byref(self._state), _lib.stream(self.device)), self.L)

    def step(self, t, rew_t, reset_t):
        """The per-step launch (pp_dr_adr_step) after the env step that wrote rew_t [A*N] f32 (unscaled) and reset_t [reset_rows*N] int64;
        stages row t of the horizon.  One launch, no synchronisation; it can be captured."""
        self._check_step(t, rew_t, reset_t)
        _lib.check(self.L.pp_dr_adr_step(self.adr_dev.data_ptr(), self.num_envs, rew_t.data_ptr(), reset_t.data_ptr(), C.byref(self._state),
                                         self.fin_slot[t].data_ptr(), self.fin_q[t].data_ptr(), _lib.stream(self.device)), self.L)

    def update(self, tot=None):
        """The totals (default: this rank's `tot`; data-parallel: their sum over the ranks) into the per-slot state, and the boundaries moved
        (pp_dr_adr_update)."""
        tot = self._totals(tot)
        _lib.check(self.L.pp_dr_adr_update(self.adr_dev.data_ptr(), self.D, tot.data_ptr(), C.byref(self._state), _lib.stream(self.device)), self.L)

    def table(self):
        """dict of device tensors: lo, hi [D] (views of `range`), and games, mean, dropped, widened, narrowed [S]."""
        return dict(lo=self.range[:, 0], hi=self.range[:, 1], games=self.games, mean=self.mean, dropped=self.dropped, widened=self.widened,
                    narrowed=self.narrowed)

    def outputs(self):
        t = self.table()
        return dict(adr_lo=t["lo"].clone(), adr_hi=t["hi"].clone(), adr_games=t["games"].clone(), adr_mean=t["mean"].clone())

    _SLOT_STATE = ("range", "acc_n", "acc_q", "games", "dropped", "mean", "widened", "narrowed")

    def state_dict(self):
        """The dims, the parameters, `range` and the per-slot state.  The per-env state is not part of it: the envs restart on resume."""
        sd = {"dims": {k: {"start": list(v["start"]), "limit": list(v["limit"]), "step": v["step"]} for k, v in self.dims.items()},
              "boundary_frac": self.boundary_frac, "min_games": self.min_games, "t_low": self.t_low, "t_high": self.t_high}
        sd.update({k: getattr(self, k).clone() for k in self._SLOT_STATE})
        return sd

    def load_state_dict(self, sd):
        """Restores the ranges and the per-slot state; ValueError if the checkpoint's dims are not this randomizer's."""
        mine = self.state_dict()["dims"]
        theirs = {k: {"start": [float(x) for x in v["start"]], "limit": [float(x) for x in v["limit"]], "step": float(v["step"])} for k, v in sd["dims"].items()}
        if theirs != mine or list(theirs) != list(mine):
            raise ValueError(f"the checkpoint's adr has other dims ({', '.join(theirs)}) than this trainer's ({', '.join(mine)})")
        with torch.no_grad():
            for k in self._SLOT_STATE:
                getattr(self, k).copy_(sd[k])


def table_json(adr, epoch=None):
    """A host copy of the randomizer's table (one read of its small tensors): dict(epoch, parameters, dims: a list of dict(table, start,
    limit, step, lo, hi, and per side games, mean_return, dropped, widened, narrowed), interior: the interior slot's games, mean, dropped)."""
    t = adr.table()
    lo, hi, games, mean, dropped, widened, narrowed = (t[k].tolist() for k in ("lo", "hi", "games", "mean", "dropped", "widened", "narrowed"))
    side = lambda s: dict(games=int(games[s]), mean_return=float(mean[s]), dropped=int(dropped[s]), widened=int(widened[s]), narrowed=int(narrowed[s]))
    dims = [dict(table=name, start=list(adr.dims[name]["start"]), limit=list(adr.dims[name]["limit"]), step=adr.dims[name]["step"], lo=float(lo[d]),
                 hi=float(hi[d]), lo_side=side(2 * d), hi_side=side(2 * d + 1)) for d, name in enumerate(adr.names)]
    s = 2 * adr.D
    return dict(epoch=epoch, boundary_frac=adr.boundary_frac, min_games=adr.min_games, t_low=adr.t_low, t_high=adr.t_high, dims=dims,
                interior=dict(games=int(games[s]), mean_return=float(mean[s]), dropped=int(dropped[s])))


def table_lines(table):
    """table_json's dict -> the CLI's lines: one per dim with its range and, per side, the games, the last judged mean and the moves."""
    head = f"adr{'' if table['epoch'] is None else ' at epoch ' + str(table['epoch'])}: {len(table['dims'])} dims, boundary share " \
           f"{table['boundary_frac']:g}, widen at {table['t_high']:g}, narrow at {table['t_low']:g}, judged every {table['min_games']} games"
    side = lambda r: f"games {r['games']} mean {r['mean_return']:.4g} +{r['widened']} -{r['narrowed']}" + (f" dropped {r['dropped']}" if r["dropped"] else "")
    lines = [f"  {r['table']}: [{r['lo']:.6g}, {r['hi']:.6g}]  (start {r['start'][0]:g}..{r['start'][1]:g}, limit {r['limit'][0]:g}..{r['limit'][1]:g})  "
             f"lo: {side(r['lo_side'])}  hi: {side(r['hi_side'])}" for r in table["dims"]]
    i = table["interior"]
    return [head] + lines + [f"  interior: games {i['games']} mean {i['mean_return']:.4g}" + (f" dropped {i['dropped']}" if i["dropped"] else "")]
