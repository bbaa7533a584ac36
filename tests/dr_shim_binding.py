"""ctypes binding of tests/csrc/libppenv_drshim.so — the reset-time domain-randomisation arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_dr_device.h) compiled for the host, built the way shim_binding.lib() builds the step's.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import json
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import scene

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "dr_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_dr_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_dr.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_drshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off", "-fno-signed-zeros", "-ffinite-math-only"])
        u32, u64, i32, i64, vp = C.c_uint32, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p
        L.dr_shim_uniform.restype = L.dr_shim_base.restype = L.dr_shim_weight.restype = L.dr_shim_value.restype = C.c_float
        L.dr_shim_uniform.argtypes = [u64, u32, u32, u32]
        L.dr_shim_base.argtypes = [u64, u32, u32, u32, i32]
        L.dr_shim_weight.argtypes = [i32, i32, i64]
        L.dr_shim_value.argtypes = [C.POINTER(scene.DREntry), u64, u32, u32, u32, i64]
        L.dr_shim_apply.restype = L.dr_shim_apply_ids.restype = None
        L.dr_shim_apply.argtypes = [C.POINTER(scene.DRPlan), vp, vp, vp, vp]
        L.dr_shim_apply_ids.argtypes = [C.POINTER(scene.DRPlan), vp, i32, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostDR:
    """The state a device handle keeps for a plan (isaacgym_amd.dr.ResetRandomizer), in numpy, stepped by the kernel body on the CPU."""

    def __init__(self, plan, num_envs, seed=0, env_id_offset=0, reset_rows=1):
        self.L = lib()
        n = self.num_envs = int(num_envs)
        self.tables = {}
        for name, t in plan["tables"].items():
            fill = 1.0 if t["operation"] == "scaling" else 0.0
            self.tables[name] = np.full((t["rows"], n), fill, np.float32)
        self.plan = scene.build_dr_plan(plan, {k: v.ctypes.data for k, v in self.tables.items()}, n, env_id_offset=env_id_offset, seed=seed,
                                        reset_rows=reset_rows)
        self.randomize_buf = np.zeros(n, np.int64)
        self.draws = np.zeros(n, np.int32)
        self.count = np.zeros(1, np.int64)

    def apply(self, reset_buf):
        r = np.ascontiguousarray(reset_buf, np.int64)
        assert r.size == self.plan.reset_rows * self.num_envs
        self.L.dr_shim_apply(C.byref(self.plan), _p(r), _p(self.randomize_buf), _p(self.count), _p(self.draws))

    def apply_ids(self, env_ids):
        ids = np.unique(np.asarray(env_ids, np.int64))
        self.L.dr_shim_apply_ids(C.byref(self.plan), _p(ids), ids.size, _p(self.randomize_buf), _p(self.count), _p(self.draws))


def entry(distribution, operation, a, b, schedule=None, schedule_steps=0):
    en = scene.DREntry()
    en.rows, en.distribution, en.operation, en.schedule = 1, scene.DR_DISTRIBUTIONS[distribution], scene.DR_OPERATIONS[operation], scene.DR_SCHEDULES[schedule]
    en.a, en.b, en.schedule_steps = a, b, schedule_steps
    return en


# ---- the cases the host and the GPU tests share
def task_block(name):
    return json.load(open(os.path.join(_HERE, "golden", "task_cfgs.json")))[name]["task"]["task"]["randomization_params"]


def scripted_resets(steps, rows, p=0.08, seed=5):
    """The reset_buf sequence the rule tests and the GPU tests drive: each row resets with probability p per step, bursts included
    (consecutive resets of one env exercise `randomize_buf >= frequency` from both sides)."""
    rng = np.random.default_rng(seed)
    r = (rng.random((steps, rows)) < p).astype(np.int64)
    r[10:14, : rows // 4] = 1
    return r


def mixed_plan(**over):
    """A plan with every table shape of the 7-dof tasks and every distribution / operation / schedule once."""
    t = {"dof_stiffness_scale": dict(rows=7, distribution="uniform", operation="scaling", range=(0.5, 1.5), schedule="linear", schedule_steps=150),
         "dof_damping_scale": dict(rows=7, distribution="gaussian", operation="scaling", range=(1.0, 0.1), schedule=None, schedule_steps=0),
         "link_mass_scale": dict(rows=7, distribution="uniform", operation="additive", range=(-0.2, 0.3), schedule="constant", schedule_steps=40),
         "restitution_scale": dict(rows=1, distribution="gaussian", operation="additive", range=(0.0, 0.01), schedule="linear", schedule_steps=3000),
         "friction_scale": dict(rows=1, distribution="uniform", operation="scaling", range=(0.7, 1.3), schedule=None, schedule_steps=0)}
    return dict({"frequency": 5, "tables": t}, **over)
