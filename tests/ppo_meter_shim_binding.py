"""ctypes binding of tests/csrc/libppenv_ppometershim.so — the score meter's arithmetic (isaacgym_amd/csrc/ppenv_ppo_meter_device.h)
compiled for the host in the kernels' summation order, built the way play_shim_binding.lib() builds the play accounting's.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd._lib import PPOMeter

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "ppo_meter_shim.cpp")
_HDRS = [os.path.join(_HERE, "csrc", "butterfly_host.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_ppo_meter_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_ppo_meter.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_ppometershim.so")
_lib = None

FIELDS = ("mean_reward", "mean_length", "current_size", "games_total", "updates")


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.ppo_meter_shim_sizeof_meter.restype = L.ppo_meter_shim_sizeof_partial.restype = C.c_size_t
        L.ppo_meter_shim_update.restype = L.ppo_meter_shim_apply.restype = None
        L.ppo_meter_shim_update.argtypes = [vp, i64, vp, i64, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp]
        L.ppo_meter_shim_apply.argtypes = [vp, C.c_double, i64, i32, i64]
        assert L.ppo_meter_shim_sizeof_meter() == C.sizeof(PPOMeter) == 40 and L.ppo_meter_shim_sizeof_partial() == 24
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def meter_dict(raw):
    """The 40 bytes of a ppenv_ppo_meter -> a Python dict."""
    m = PPOMeter.from_buffer_copy(bytes(raw))
    return {k: getattr(m, k) for k in FIELDS}


class HostMeter:
    """isaacgym_amd.ppo.GameMeter in numpy, stepped by the kernels' arithmetic on the CPU."""

    def __init__(self, num_envs, num_agents, games_to_track):
        self.L = lib()
        self.num_envs, self.num_agents, self.games_to_track = int(num_envs), int(num_agents), int(games_to_track)
        self.rows = self.num_envs * self.num_agents
        self.cur_reward = np.zeros(self.num_envs, np.float32)
        self.cur_len = np.zeros(self.num_envs, np.int32)
        self.meter = np.zeros(C.sizeof(PPOMeter), np.uint8)
        self.steps = None                                          # (S_t, L_t, c_t) of the last update

    def update(self, rew, done):
        """rew [H, rows] float32, done [H, rows] int64 (any row stride)."""
        assert rew.dtype == np.float32 and done.dtype == np.int64 and rew.shape == done.shape and rew.shape[1] == self.rows
        assert rew.strides[1] == 4 and done.strides[1] == 8
        h = rew.shape[0]
        s, l, c = np.zeros(h, np.float64), np.zeros(h, np.int64), np.zeros(h, np.int64)
        self.L.ppo_meter_shim_update(_p(rew), rew.strides[0] // 4 if h > 1 else self.rows, _p(done), done.strides[0] // 8 if h > 1 else self.rows, h,
                                     self.num_envs, self.num_agents, self.games_to_track, _p(self.cur_reward), _p(self.cur_len), _p(self.meter),
                                     _p(s), _p(l), _p(c))
        self.steps = (s, l, c)

    def apply(self, s, l, c):
        self.L.ppo_meter_shim_apply(_p(self.meter), float(s), int(l), int(c), self.games_to_track)

    def read(self):
        return meter_dict(self.meter.tobytes())

    def state_bytes(self):
        return self.cur_reward.tobytes(), self.cur_len.tobytes(), self.meter.tobytes()
