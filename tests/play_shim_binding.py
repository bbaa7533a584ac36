"""ctypes binding of tests/csrc/libppenv_playshim.so — the episode-accounting arithmetic of the HIP kernels
(isaacgym_amd/csrc/ppenv_play_device.h) compiled for the host, built the way dr_shim_binding.lib() builds the randomisation's.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd.play import PlayTotals, totals_dict

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "play_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_play_device.h"), os.path.join(_HERE, "..", "isaacgym_amd", "csrc", "ppenv_device.h"),
         os.path.join(_HERE, "..", "include", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_playshim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, ["-ffp-contract=off"])
        i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
        L.play_shim_sizeof_totals.restype = L.play_shim_sizeof_partial.restype = C.c_size_t
        L.play_shim_reset.restype = L.play_shim_accumulate.restype = None
        L.play_shim_reset.argtypes = [i32, i32, vp, vp, vp]
        L.play_shim_accumulate.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp]
        assert L.play_shim_sizeof_totals() == C.sizeof(PlayTotals) == 72 and L.play_shim_sizeof_partial() == 64
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostStats:
    """isaacgym_amd.play.EpisodeStats in numpy, stepped by the kernel body on the CPU."""

    def __init__(self, num_envs, num_agents, games_num):
        self.L = lib()
        self.num_envs, self.num_agents, self.games_num = int(num_envs), int(num_agents), int(games_num)
        self.rows = self.num_envs * self.num_agents
        self.cur_reward = np.full(self.rows, 7.0, np.float32)          # garbage: reset() must clear it
        self.cur_steps = np.full(self.num_envs, 7, np.int32)
        self.totals = np.full(C.sizeof(PlayTotals), 0x55, np.uint8)
        self.reset()

    def reset(self):
        self.L.play_shim_reset(self.num_envs, self.num_agents, _p(self.cur_reward), _p(self.cur_steps), _p(self.totals))

    def accumulate(self, rew, done):
        r, d = np.ascontiguousarray(rew, np.float32), np.ascontiguousarray(done, np.int64)
        assert r.size == self.rows and d.size == self.rows
        self.L.play_shim_accumulate(_p(r), _p(d), self.num_envs, self.num_agents, self.games_num, _p(self.cur_reward), _p(self.cur_steps),
                                    _p(self.totals))

    def read(self):
        return totals_dict(PlayTotals.from_buffer_copy(self.totals.tobytes()), self.num_agents)

    def state_bytes(self):
        return self.cur_reward.tobytes(), self.cur_steps.tobytes(), self.totals.tobytes()


# ---- the cases the host and the GPU tests share
def scripted_dones(steps, num_envs, num_agents, words=(1,), p=0.08, seed=5):
    """[steps, rows] int64 done words in the shape of dr_shim_binding.scripted_resets: each env finishes with probability p per step,
    plus a burst of consecutive finishes on a quarter of the envs.  Both agent rows of an env carry the env's word (the 4-actor task
    resets them together); the non-zero words cycle through `words`."""
    rng = np.random.default_rng(seed)
    fin = rng.random((steps, num_envs)) < p
    fin[10:14, : num_envs // 4] = True
    fin[5, 0] = True                                                # (num_envs // 4 is 0 for one env)
    w = np.asarray(words, np.int64)
    word = w[(np.arange(steps)[:, None] + np.arange(num_envs)[None, :]) % w.size]
    return np.repeat(np.where(fin, word, 0), num_agents, axis=1).astype(np.int64)


def rewards(steps, rows, seed=6, integer=False):
    """[steps, rows] float32: per-step rewards of the tasks' magnitude (a few units, now and then a penalty in the hundreds), or integers in
    [-3000, 3000] — with those every fp32 return and every fp64 sum is exact, whatever the order."""
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-3000, 3001, (steps, rows)).astype(np.float32)
    r = rng.standard_normal((steps, rows)) * 2.0
    r[rng.random((steps, rows)) < 0.02] -= 300.0
    return r.astype(np.float32)
