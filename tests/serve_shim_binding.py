"""ctypes binding of tests/csrc/libppenv_serveshim.so — the serve-plan arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_serve_device.h) compiled for the host, built the way play_shim_binding.lib() builds the accounting's.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import _lib, serve

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "serve_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_serve_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_serve.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_serveshim.so")
_shim = None

# every axis named: what the tests' cells leave out
DEFAULTS = {"serve_speed": (8.0, 8.6), "serve_tilt": (-5.0, 5.0), "serve_tilt_z": (2.0, 10.0), "ball_y": (-0.5, 0.1), "ball_z": (0.96, 1.05)}


def lib():
    global _shim
    if _shim is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, vp, f32 = C.c_int32, C.c_void_p, C.c_float
        L.serve_shim_sizeof_plan.restype = L.serve_shim_sizeof_cell.restype = C.c_size_t
        L.serve_shim_invalid.argtypes = [C.POINTER(_lib.ServePlan), C.POINTER(_lib.ServeCell)]
        L.serve_shim_fill.restype = L.serve_shim_apply.restype = L.serve_shim_apply_ids.restype = L.serve_shim_velocity.restype = None
        L.serve_shim_fill.argtypes = [C.POINTER(_lib.ServePlan), vp, vp]
        L.serve_shim_apply.argtypes = [C.POINTER(_lib.ServePlan), vp, vp, vp]
        L.serve_shim_apply_ids.argtypes = [C.POINTER(_lib.ServePlan), vp, i32, vp, vp]
        L.serve_shim_velocity.argtypes = [i32, f32, f32, f32, vp]
        assert L.serve_shim_sizeof_plan() == C.sizeof(_lib.ServePlan) == 48 and L.serve_shim_sizeof_cell() == C.sizeof(_lib.ServeCell) == 40
        _shim = L
    return _shim


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_plan(num_envs, cells, form, layout, reset_rows=1, seed=0, env_id_offset=0, paired=False, groups=None, envs_per_group=None):
    """(pp_serve_plan pointing at host cells, the cells array) as serve.ServePlan builds them; groups / envs_per_group: overrides, for the refusals."""
    resolved = serve.resolve_cells(cells, DEFAULTS, serve.AXES_27DOF)
    arr = serve.cell_structs(resolved)
    G = len(resolved) if groups is None else groups
    plan = _lib.ServePlan(num_envs=num_envs, env_id_offset=env_id_offset, seed=seed & 0xFFFFFFFFFFFFFFFF, form=form, layout=layout, reset_rows=reset_rows,
                          groups=G, envs_per_group=(num_envs // max(G, 1)) if envs_per_group is None else envs_per_group, paired=int(paired),
                          cells=C.cast(arr, C.c_void_p))
    return plan, arr


class HostServe:
    """isaacgym_amd.serve.ServePlan in numpy, stepped by the kernel body on the CPU."""

    def __init__(self, num_envs, cells, form, layout, reset_rows=1, seed=0, env_id_offset=0, paired=False):
        self.L = lib()
        n = self.num_envs = int(num_envs)
        self.plan, self._cells = host_plan(n, cells, form, layout, reset_rows, seed, env_id_offset, paired)
        assert self.L.serve_shim_invalid(C.byref(self.plan), self._cells) == 0
        self.reset_rows = reset_rows
        self.out = np.zeros((3, n) if layout == _lib.SERVE_LAYOUT_SOA3 else (n, 5), np.float32)
        self.count = np.zeros(n, np.uint32)
        self.fill()

    def fill(self):
        self.L.serve_shim_fill(C.byref(self.plan), _p(self.out), _p(self.count))

    def apply(self, reset_buf):
        r = np.ascontiguousarray(reset_buf, np.int64)
        assert r.size == self.reset_rows * self.num_envs
        self.L.serve_shim_apply(C.byref(self.plan), _p(r), _p(self.out), _p(self.count))

    def apply_ids(self, env_ids):
        ids = np.unique(np.asarray(env_ids, np.int64))
        self.L.serve_shim_apply_ids(C.byref(self.plan), _p(ids), ids.size, _p(self.out), _p(self.count))


def velocity(form, speed, tilt, tilt_z):
    v = np.zeros(3, np.float32)
    lib().serve_shim_velocity(form, speed, tilt, tilt_z, _p(v))
    return v


# ---- the cases the host and the GPU tests share
def scripted_resets(steps, num_envs, reset_rows, p=0.1, seed=7):
    """[steps, reset_rows * num_envs] int64 reset words: each env resets with probability p per step, with a burst of consecutive resets on a
    quarter of the envs; both rows of an env carry its word; some non-zero words are 2**32 (the low half alone would read as zero)."""
    rng = np.random.default_rng(seed)
    fire = rng.random((steps, num_envs)) < p
    fire[10:14, : num_envs // 4] = True
    fire[5, 0] = True
    word = np.where((np.arange(steps)[:, None] + np.arange(num_envs)[None, :]) % 3 == 0, 2 ** 32, 1).astype(np.int64)
    return np.repeat(np.where(fire, word, 0), reset_rows, axis=1).astype(np.int64)


def two_cells():
    return [{"serve_speed": (6.0, 6.5), "serve_tilt": -3.0}, {"serve_speed": (9.0, 9.5), "serve_tilt_z": (4.0, 12.0), "ball_y": (-0.2, 0.0)}]
