"""The serve plan of an environment handle (include/ppenv_serve.h): each env's NEXT serve, kept on the device in the override buffer the
handle's step kernel reads at a reset instead of its RNG.  `ServePlan` is what PPEnv.set_serve_plan and TAEnv.set_serve_plan return: the
buffer (`out`), the per-env count of consumed serves (`count`), the cells as resolved against the handle's configured ranges (`cells`), and
the launches.  torch owns the memory; the library rewrites the rows of the envs that reset, one launch per control step, no host read."""
import ctypes as C
import math

import torch

from . import _lib

# a cell's keys -> the (lo, hi) fields of pp_serve_cell; ball_y / ball_z exist for the [N,5] layout (the 27-dof task) only
CELL_FIELDS = {"serve_speed": ("speed_lo", "speed_hi"), "serve_tilt": ("tilt_lo_deg", "tilt_hi_deg"), "serve_tilt_z": ("tilt_z_lo_deg", "tilt_z_hi_deg"),
               "ball_y": ("ball_y_lo", "ball_y_hi"), "ball_z": ("ball_z_lo", "ball_z_hi")}
AXES_7DOF = ("serve_speed", "serve_tilt", "serve_tilt_z")
AXES_27DOF = AXES_7DOF + ("ball_y", "ball_z")


def value_range(axis, v):
    """A cell's value — a number (pinned) or (lo, hi) — as a (lo, hi) pair of finite floats with lo <= hi; tilts within the kernels' series."""
    try:
        lo, hi = (float(v), float(v)) if not isinstance(v, (tuple, list)) else (float(v[0]), float(v[1])) if len(v) == 2 else (math.nan, math.nan)
    except (TypeError, ValueError):
        lo = hi = math.nan
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"serve axis {axis!r}: {v!r} is not a finite number or a (lo, hi) pair with lo <= hi")
    if axis in ("serve_tilt", "serve_tilt_z") and max(abs(lo), abs(hi)) > _lib.SERVE_MAX_TILT_DEG:
        raise ValueError(f"serve axis {axis!r}: {v!r} lies beyond +-{_lib.SERVE_MAX_TILT_DEG:g} degrees (the kernels' sine / cosine of a serve angle is a short series)")
    return lo, hi


def resolve_cells(cells, defaults, axes):
    """cells: dicts of any of `axes`, each a number or (lo, hi); defaults: {axis: (lo, hi)}, what a cell does not name.
    -> one {axis: (lo, hi)} per cell.  A key outside `axes` raises ValueError naming them."""
    out = []
    for cell in cells:
        full = {a: (float(defaults[a][0]), float(defaults[a][1])) for a in axes}
        for axis, v in dict(cell).items():
            if axis not in axes:
                raise ValueError(f"serve axis {axis!r}: this environment's serve axes are {', '.join(axes)}")
            full[axis] = value_range(axis, v)
        out.append(full)
    return out


def cell_structs(resolved):
    arr = (_lib.ServeCell * len(resolved))()
    for c, full in zip(arr, resolved):
        for axis, (lo, hi) in full.items():
            setattr(c, CELL_FIELDS[axis][0], lo)
            setattr(c, CELL_FIELDS[axis][1], hi)
    return arr


class ServePlan:
    def __init__(self, L, device, num_envs, cells, defaults, axes, out, form, layout, reset_rows, seed, env_id_offset=0, paired=False):
        """cells: G dicts (G divides num_envs; group g is envs [g * S, (g + 1) * S)).  out: the override buffer, float32 on `device`:
        [3, N] (layout 0) or [N, 5] (layout 1).  seed: a STREAM seed (scene.stream_seed(user seed, scene.STREAM_SERVES)).  paired: key the
        draws by the env's index WITHIN its group, so that env i of every group is served the same sequence of balls.
        Uploads the plan, zeroes `count` and fills `out` with every env's serve 0."""
        self.L, self.device, self.num_envs = L, torch.device(device), int(num_envs)
        cells = list(cells)
        G, n = len(cells), self.num_envs
        if G < 1 or n % G:
            raise ValueError(f"a serve plan of {G} cells needs a multiple of {G} envs, not {n}")
        self.cells = resolve_cells(cells, defaults, axes)
        self.paired, self.reset_rows, self.layout = bool(paired), int(reset_rows), int(layout)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device
        assert tuple(out.shape) == ((3, n) if layout == _lib.SERVE_LAYOUT_SOA3 else (n, 5)), tuple(out.shape)
        self.out = out
        self.count = torch.zeros(n, dtype=torch.int32, device=self.device)            # uint32 on the device: serves consumed
        host = _lib.ServePlan(num_envs=n, env_id_offset=int(env_id_offset), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, form=int(form), layout=int(layout),
                              reset_rows=int(reset_rows), groups=G, envs_per_group=n // G, paired=int(self.paired), cells=None)
        self.plan_dev = torch.zeros(C.sizeof(_lib.ServePlan), dtype=torch.uint8, device=self.device)
        self.cells_dev = torch.zeros(G * C.sizeof(_lib.ServeCell), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pp_serve_plan_upload(C.byref(host), cell_structs(self.cells), self.plan_dev.data_ptr(), self.cells_dev.data_ptr(),
                                              _lib.stream(self.device)), L)
        self.fill()

    def fill(self):
        """out[e] = serve(e, count[e]) for every env (pp_serve_fill); nothing advances."""
        _lib.check(self.L.pp_serve_fill(self.plan_dev.data_ptr(), self.num_envs, self.out.data_ptr(), self.count.data_ptr(), _lib.stream(self.device)), self.L)

    def apply(self, reset_buf):
        """The per-step launch (pp_serve_apply), after the step that wrote reset_buf [reset_rows * N] int64: the envs that reset have consumed
        their serve and get their next one.  One launch, no synchronisation; it can be captured."""
        assert reset_buf.dtype == torch.int64 and reset_buf.is_contiguous() and reset_buf.numel() == self.reset_rows * self.num_envs
        _lib.check(self.L.pp_serve_apply(self.plan_dev.data_ptr(), self.num_envs, reset_buf.data_ptr(), self.out.data_ptr(), self.count.data_ptr(),
                                         _lib.stream(self.device)), self.L)

    def step(self, t, rew_t, reset_t):
        """What RolloutCollector calls after the env step of row t of a horizon (its `serve` object): apply(reset_t)."""
        self.apply(reset_t)

    def apply_ids(self, env_ids):
        """The same for the envs reset_idx(env_ids) lists (pp_serve_apply_ids); duplicates are dropped here (the kernel wants distinct ids)."""
        ids = torch.unique(torch.as_tensor(env_ids, dtype=torch.int64).reshape(-1).to(self.device))
        if ids.numel() == 0:
            return
        _lib.check(self.L.pp_serve_apply_ids(self.plan_dev.data_ptr(), self.num_envs, ids.data_ptr(), ids.numel(), self.out.data_ptr(),
                                             self.count.data_ptr(), _lib.stream(self.device)), self.L)
        ids.record_stream(torch.cuda.current_stream(self.device))
