"""The adaptive serve curriculum of an environment handle (include/ppenv_serve_curric.h): the serve space cut into bins, every finished
game's return credited to the bin its ball was drawn from, every env's next serve drawn from a per-bin table that favours the bins the
policy currently scores worst on.  The reference has no serve curriculum: the rule is this project's own specification.

`ServeCurriculum` is what PPEnv.set_serve_curriculum and TAEnv.set_serve_curriculum return, built like serve.ServePlan: the override buffer
(`out`), the per-env and per-bin state, the staging rows of one horizon and the launches — one per control step (`step`), two per epoch
(`fold`, `update`).  The staging, the fold and the epoch's sequence are `HorizonStage`'s, which adr.AutoRandomizer shares.  torch owns
the memory; nothing here reads the device on the host."""
import ctypes as C
import math

import torch

from . import _lib, serve


def check_parameters(power, mix, alpha):
    """-> (power, mix, alpha) as the library takes them; ValueError outside power 0..4 (an integer), mix [0, 1], alpha (0, 1]."""
    if isinstance(power, bool) or not isinstance(power, int) or not 0 <= power <= _lib.CURRIC_MAX_POWER:
        raise ValueError(f"curriculum power {power!r}: an integer 0 .. {_lib.CURRIC_MAX_POWER}")
    try:
        mix, alpha = float(mix), float(alpha)
    except (TypeError, ValueError):
        mix = alpha = math.nan
    if not (math.isfinite(mix) and 0.0 <= mix <= 1.0):
        raise ValueError(f"curriculum mix {mix!r}: a number in [0, 1]")
    if not (math.isfinite(alpha) and 0.0 < alpha <= 1.0):
        raise ValueError(f"curriculum alpha {alpha!r}: a number in (0, 1]")
    return power, mix, alpha


def grid(axes):
    """{axis: (lo, hi, n)} -> the bin cells: every axis cut into n equal sub-intervals, the product of the axes, the LAST axis fastest.
    A cell names only the grid's axes; what it leaves out is the handle's serve_defaults().  More than 256 bins: ValueError."""
    specs = {}
    for axis, spec in dict(axes).items():
        try:
            lo, hi, n = float(spec[0]), float(spec[1]), int(spec[2])
            ok = len(spec) == 3 and n == spec[2] and n >= 1
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise ValueError(f"curriculum axis {axis!r}: {spec!r} is not (lo, hi, bins) with bins >= 1")
        serve.value_range(axis, (lo, hi))
        specs[axis] = (lo, hi, n)
    total = math.prod(n for _, _, n in specs.values())
    if total > _lib.CURRIC_MAX_BINS:
        raise ValueError(f"a serve curriculum of {total} bins: at most {_lib.CURRIC_MAX_BINS}")
    cells = [{}]
    for axis, (lo, hi, n) in specs.items():
        edges = [lo + (hi - lo) * k / n for k in range(n)] + [hi]
        cells = [dict(c, **{axis: (edges[k], edges[k + 1])}) for c in cells for k in range(n)]
    return cells


def grid_parse(flags):
    """The CLI form: ["serve_speed=6:9:4", ...] -> {axis: (lo, hi, bins)} (an axis given twice: the last one)."""
    out = {}
    for flag in flags or ():
        axis, sep, v = str(flag).partition("=")
        parts = v.split(":")
        try:
            if not sep or len(parts) != 3:
                raise ValueError
            out[axis.strip()] = (float(parts[0]), float(parts[1]), int(parts[2]))
        except ValueError:
            raise ValueError(f"--curriculum {flag!r}: expected AXIS=LO:HI:BINS") from None
    return out


class HorizonStage:
    """What ServeCurriculum and adr.AutoRandomizer share: the staging of one horizon — per control step and env the slot (a bin; an ADR
    boundary) a finished game is credited to, -1 for none, and its quantised return —, the fold of a staged horizon into per-slot totals,
    and the epoch's sequence fold -> (the ranks' sum) -> update.  A subclass sets L, device, num_envs, num_agents, reset_rows and horizon,
    calls _staging(K), and has its own step(), update(tot) and outputs()."""

    def _staging(self, K):
        """Allocates `fin` [H, N] int32 (all -1), `fin_q` [H, N] int64, `tot` [3, K] int64 and the fold's scratch.  -> fin."""
        n, z = self.num_envs, lambda *shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.fin, self.fin_q = torch.full((self.horizon, n), -1, dtype=torch.int32, device=self.device), z(self.horizon, n, dt=torch.int64)
        self.tot = z(3, K, dt=torch.int64)
        self._partial = z(int(self.L.pp_serve_curric_fold_bytes(self.horizon * n)), dt=torch.uint8)
        return self.fin

    def _check_step(self, t, rew_t, reset_t):
        assert 0 <= t < self.horizon
        assert rew_t.dtype == torch.float32 and rew_t.is_contiguous() and rew_t.numel() == self.num_agents * self.num_envs
        assert reset_t.dtype == torch.int64 and reset_t.is_contiguous() and reset_t.numel() == self.reset_rows * self.num_envs

    def _totals(self, tot):
        """update()'s argument: this rank's `tot` by default, checked."""
        tot = self.tot if tot is None else tot
        assert tot.dtype == torch.int64 and tot.is_contiguous() and tot.shape == self.tot.shape and tot.device == self.tot.device
        return tot

    def fold(self):
        """The staged horizon -> `tot` [3, K] int64: games, sum of q, dropped games per slot (pp_serve_curric_fold, generic over K)."""
        _lib.check(self.L.pp_serve_curric_fold(self.fin.data_ptr(), self.fin_q.data_ptr(), self.horizon * self.num_envs, self.tot.shape[1], self.tot.data_ptr(),
                                               self._partial.data_ptr() if self._partial.numel() else None, _lib.stream(self.device)), self.L)
        return self.tot

    @torch.no_grad()
    def epoch(self, reduce=None):
        """The collected horizon into the stage: fold, reduce(tot) in place where given (data-parallel: the ranks' sum), update.  -> the
        epoch's named outputs for train_epoch()."""
        tot = self.fold()
        if reduce is not None:
            reduce(tot)
        self.update(tot)
        return self.outputs()


class ServeCurriculum(HorizonStage):
    grid = staticmethod(grid)

    def __init__(self, env, bins, power=1, mix=0.25, alpha=0.3, seed=None, horizon=32):
        """env: a PPEnv or TAEnv (its serve_target() names the override buffer, the form, the layout and the keys).  bins: B cell dicts
        (grid(...), or any dicts a serve plan takes), resolved against env.serve_defaults().  seed: a STREAM seed, default
        scene.stream_seed(the handle's seed, scene.STREAM_SERVES).  horizon: the rows of the staging buffers, the H of step(t).
        Uploads the curriculum, zeroes the state and fills `out` with every env's serve 0 drawn from the uniform table."""
        self.power, self.mix, self.alpha = check_parameters(power, mix, alpha)
        bins = list(bins)
        if not 1 <= len(bins) <= _lib.CURRIC_MAX_BINS:
            raise ValueError(f"a serve curriculum of {len(bins)} bins: 1 .. {_lib.CURRIC_MAX_BINS}")
        tgt = env.serve_target()
        self.L, self.device, self.num_envs, self.num_agents = env.L, torch.device(env.device), int(env.num_envs), int(env.num_agents)
        self.cells = serve.resolve_cells(bins, env.serve_defaults(), tgt["axes"])
        self.bins, self.horizon, self.layout, self.reset_rows = len(bins), int(horizon), int(tgt["layout"]), int(tgt["reset_rows"])
        self.seed = int(tgt["seed"] if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        n, B, dev = self.num_envs, self.bins, self.device
        out = tgt["out"] if tgt["out"] is not None else torch.zeros((n, 5), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
        assert tuple(out.shape) == ((3, n) if self.layout == _lib.SERVE_LAYOUT_SOA3 else (n, 5)), tuple(out.shape)
        self.out = out
        z = lambda *shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.count, self.next_bin, self.cur_bin, self.ret = z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.int32), z(n, dt=torch.float32)
        self.games, self.mean, self.dropped, self.cdf = z(B, dt=torch.int64), z(B, dt=torch.float32), z(B, dt=torch.int64), z(B, dt=torch.int32)
        self.fin_bin = self._staging(B)
        self._state = _lib.ServeCurricState(*(t.data_ptr() for t in (self.count, self.next_bin, self.cur_bin, self.ret, self.games, self.mean,
                                                                     self.dropped, self.cdf)))
        host = _lib.ServeCurric(num_envs=n, env_id_offset=int(tgt["env_id_offset"]), seed=self.seed, form=int(tgt["form"]), layout=self.layout,
                                reset_rows=self.reset_rows, num_agents=self.num_agents, bins=B, power=self.power, mix=self.mix, alpha=self.alpha, cells=None)
        self.curric_dev = z(C.sizeof(_lib.ServeCurric), dt=torch.uint8)
        self.cells_dev = z(B * C.sizeof(_lib.ServeCell), dt=torch.uint8)
        with torch.cuda.device(dev):
            _lib.check(self.L.pp_serve_curric_upload(C.byref(host), serve.cell_structs(self.cells), self.curric_dev.data_ptr(), self.cells_dev.data_ptr(),
                                                     _lib.stream(dev)), self.L)
        self.fill()

    def fill(self):
        """The uniform table, every env's serve(e, count[e]) from it, cur_bin = -1, ret = 0 (pp_serve_curric_fill)."""
        _lib.check(self.L.pp_serve_curric_fill(self.curric_dev.data_ptr(), self.num_envs, self.bins, C.byref(self._state), self.out.data_ptr(),
                                               _lib.stream(self.device)), self.L)

    def step(self, t, rew_t, reset_t):
        """The per-step launch (pp_serve_curric_step) after the env step that wrote rew_t [A*N] f32 (unscaled) and reset_t [reset_rows*N]
        int64; stages row t of the horizon.  One launch, no synchronisation; it can be captured."""
        self._check_step(t, rew_t, reset_t)
        _lib.check(self.L.pp_serve_curric_step(self.curric_dev.data_ptr(), self.num_envs, rew_t.data_ptr(), reset_t.data_ptr(), C.byref(self._state),
                                               self.out.data_ptr(), self.fin_bin[t].data_ptr(), self.fin_q[t].data_ptr(), _lib.stream(self.device)), self.L)

    def update(self, tot=None):
        """The totals (default: this rank's `tot`; data-parallel: their sum over the ranks) into mean / games / dropped, and the new table
        (pp_serve_curric_update)."""
        tot = self._totals(tot)
        _lib.check(self.L.pp_serve_curric_update(self.curric_dev.data_ptr(), self.bins, tot.data_ptr(), C.byref(self._state), _lib.stream(self.device)), self.L)

    def table(self):
        """dict of [B] device tensors: games, mean, dropped, and prob — each bin's share of the table, (cdf[b] - cdf[b-1]) / 2^24 (fp64)."""
        cdf = self.cdf.to(torch.int64)
        prob = torch.diff(cdf, prepend=cdf.new_zeros(1)).double() / float(1 << 24)
        return dict(games=self.games, mean=self.mean, dropped=self.dropped, prob=prob)

    def outputs(self):
        t = self.table()
        return dict(curriculum_games=t["games"].clone(), curriculum_mean=t["mean"].clone(), curriculum_prob=t["prob"])

    def state_dict(self):
        """The resolved bins, the parameters and the per-bin table.  The per-env state is not part of it: the envs restart on resume."""
        return {"bins": [{k: [float(v[0]), float(v[1])] for k, v in c.items()} for c in self.cells], "power": self.power, "mix": self.mix, "alpha": self.alpha,
                "games": self.games.clone(), "mean": self.mean.clone(), "dropped": self.dropped.clone(), "cdf": self.cdf.clone()}

    def load_state_dict(self, sd):
        """Restores the table; ValueError if the checkpoint's bins are not this curriculum's."""
        mine = self.state_dict()["bins"]
        if [{k: list(v) for k, v in c.items()} for c in sd["bins"]] != mine:
            raise ValueError(f"the checkpoint's serve curriculum has other bins ({len(sd['bins'])}) than this trainer's ({len(mine)})")
        with torch.no_grad():
            for k in ("games", "mean", "dropped", "cdf"):
                getattr(self, k).copy_(sd[k])


def table_json(cur, epoch=None):
    """A host copy of the curriculum's table (one read of four [B] tensors): a list of dict(bin, cell, games, mean_return, dropped, prob)."""
    t = cur.table()
    games, mean, dropped, prob = (t[k].tolist() for k in ("games", "mean", "dropped", "prob"))
    return dict(epoch=epoch, power=cur.power, mix=cur.mix, alpha=cur.alpha,
                bins=[dict(bin=b, cell={k: [float(v[0]), float(v[1])] for k, v in cur.cells[b].items()}, games=int(games[b]), mean_return=float(mean[b]),
                           dropped=int(dropped[b]), prob=float(prob[b])) for b in range(cur.bins)])


def table_lines(table):
    """table_json's dict -> the CLI's lines: one per bin with its cell, games, mean return and probability."""
    head = f"serve curriculum{'' if table['epoch'] is None else ' at epoch ' + str(table['epoch'])}: {len(table['bins'])} bins"
    return [head] + ["  bin {bin}: cell {cell}  games {games}  mean return {mean}  prob {prob:.4f}".format(
        bin=r["bin"], cell=" ".join(f"{k}={v[0]:g}..{v[1]:g}" for k, v in r["cell"].items()), games=r["games"],
        mean=f"{r['mean_return']:.4g}" if r["games"] else "-", prob=r["prob"]) + (f"  dropped {r['dropped']}" if r["dropped"] else "") for r in table["bins"]]
