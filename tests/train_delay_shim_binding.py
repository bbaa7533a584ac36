"""ctypes binding of tests/csrc/libppenv_traindelayshim.so — the training delay line of the HIP kernel
(isaacgym_amd/csrc/ppenv_train_delay_device.h) compiled for the host and walked in the kernel's order, built the way
play_delay_shim_binding.lib() builds play's — and a numpy restatement of include/ppenv_train_delay.h's rule, written from the header's words:
every pushed array is kept, and a row's delay is redrawn with isaacgym_amd.scene.latency_draws where an episode starts.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

from helpers import build_shim
from isaacgym_amd import scene

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "csrc", "train_delay_shim.cpp")
_HDRS = [os.path.join(_HERE, "..", "isaacgym_amd", "csrc", name) for name in ("ppenv_train_delay_device.h", "ppenv_play_delay_device.h", "ppenv_device.h")] + \
        [os.path.join(_HERE, "..", "include", name) for name in ("ppenv_train_delay.h", "ppenv_play_delay.h", "ppenv_play_group.h", "ppenv_play.h")]
_LIB = os.path.join(_HERE, "csrc", "libppenv_traindelayshim.so")
_lib = None
DELAY_MAX = 15                              # PP_PLAY_DELAY_MAX
RANGES = ((0, 0), (3, 3), (0, 3), (0, 15))  # the (lo, hi) of the rule tests: no delay, fixed, drawn, drawn over the whole range
COMMAND, SENSING = 0, 1


class Consts(C.Structure):
    """pp_train_delay_consts, declared here on its own (the tests of isaacgym_amd._lib.TrainDelayConsts compare the two layouts)."""
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("seed", C.c_uint64), ("env_id_offset", C.c_int32), ("channel", C.c_int32)]


def lib():
    global _lib
    if _lib is None:
        L = build_shim(_SRC, _LIB, _HDRS, [])
        i32, i64, u64, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_void_p
        L.train_delay_shim_draws.restype = L.train_delay_shim_reset.restype = L.train_delay_shim_push.restype = None
        L.train_delay_shim_draws.argtypes = [u64, vp, vp, i64, i32, i32, i32, vp]
        L.train_delay_shim_consts_ok.restype = i32
        L.train_delay_shim_consts_ok.argtypes = [C.POINTER(Consts)]
        L.train_delay_shim_reset.argtypes = [i32, vp, vp]
        L.train_delay_shim_push.argtypes = [vp, i64, vp, i32, i32, i32, C.POINTER(Consts), vp, vp, vp, vp, vp, i64]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def shim_draws(seed, gids, episodes, channel, lo, hi):
    """pp::train_delay_draw over the broadcast of gids x episodes -> int32, lo added."""
    g, n = np.broadcast_arrays(np.asarray(gids, np.uint32), np.asarray(episodes, np.uint32))
    g, n = np.ascontiguousarray(g), np.ascontiguousarray(n)
    out = np.empty(g.shape, np.int32)
    lib().train_delay_shim_draws(int(seed), _p(g), _p(n), g.size, channel, lo, hi, _p(out))
    return out


class HostLine:
    """isaacgym_amd.latency.DelayLine in numpy, stepped by the kernel body on the CPU.  Everything starts ZEROED (the rule tests compare the
    whole ring); `out` is [rows, ld_out] and its padding stays zero."""

    def __init__(self, rows, width, lo, hi, num_agents=1, seed=0, env_id_offset=0, channel=COMMAND, ld_out=None):
        self.L = lib()
        self.rows, self.width, self.A = int(rows), int(width), int(num_agents)
        self.consts = Consts(lo, hi, int(seed), env_id_offset, channel)
        assert self.L.train_delay_shim_consts_ok(C.byref(self.consts)) == 1
        self.ld_out = self.width if ld_out is None else int(ld_out)
        self.age, self.episode, self.delay = (np.zeros(self.rows, np.int32) for _ in range(3))
        self.ring = np.zeros((hi + 1, self.rows, self.width), np.uint32)
        self.out = np.zeros((self.rows, self.ld_out), np.uint32)

    def reset(self):
        self.L.train_delay_shim_reset(self.rows, _p(self.age), _p(self.episode))

    def push(self, x, done=None):
        """x: uint32 [rows, ld_in >= width], C-contiguous; done: int64 [rows] or None.  -> the [rows, width] view of out."""
        assert x.dtype == np.uint32 and x.flags.c_contiguous and x.shape[0] == self.rows and x.shape[1] >= self.width
        d = None if done is None else np.ascontiguousarray(done, np.int64)
        assert d is None or d.shape == (self.rows,)
        self.L.train_delay_shim_push(_p(x), x.shape[1], None if d is None else _p(d), self.rows, self.A, self.width, C.byref(self.consts), _p(self.delay),
                                     _p(self.age), _p(self.episode), _p(self.ring), _p(self.out), self.ld_out)
        return self.out[:, :self.width]


class NumpyLine:
    """The header's rule in numpy.  Every pushed sample is kept; per row the index of the push that began its running episode, the number of
    episodes begun and the running episode's delay, redrawn with scene.latency_draws at each episode start.  The output of push t for row r is
    the sample of push start[r] + max(t - start[r] - d[r], 0); the ring is restated beside it (slot = samples into the episode mod K)."""

    def __init__(self, rows, width, lo, hi, num_agents=1, seed=0, env_id_offset=0, channel=COMMAND):
        self.rows, self.width, self.A, self.lo, self.hi = int(rows), int(width), int(num_agents), int(lo), int(hi)
        self.seed, self.offset, self.channel = int(seed), int(env_id_offset), int(channel)
        self.kept, self.start = [], np.zeros(self.rows, np.int64)
        self.fresh = np.ones(self.rows, bool)                                              # no sample of the running episode yet
        self.episode, self.delay = np.zeros(self.rows, np.int32), np.zeros(self.rows, np.int32)
        self.ring = np.zeros((self.hi + 1, self.rows, self.width), np.uint32)

    @property
    def age(self):
        return np.where(self.fresh, 0, len(self.kept) - self.start).astype(np.int32)

    def push(self, x, done=None):
        t, rows = len(self.kept), np.arange(self.rows)
        self.kept.append(np.array(x[:, :self.width], copy=True))
        first = self.fresh.copy()
        if done is not None:
            first |= np.repeat(np.asarray(done).reshape(-1, self.A)[:, 0] != 0, self.A)    # agent 0's word, for every row of the env
        self.start[first] = t
        self.delay[first] = scene.latency_draws(self.seed, self.offset + rows[first] // self.A, self.episode[first], self.channel, self.lo, self.hi)
        self.episode[first] += 1
        self.fresh[:] = False
        a = t - self.start
        self.ring[a % (self.hi + 1), rows] = self.kept[t]
        src = self.start + np.maximum(a - self.delay, 0)
        out = np.empty((self.rows, self.width), x.dtype)
        for r in range(self.rows):
            out[r] = self.kept[src[r]][r]
        return out


def case_stream(rows, A, W, pushes, pad, seed=23, p_done=0.1):
    """-> xs uint32 [T, rows, W + pad] of random words and dones int64 [T, rows]: agent 0's word set (1, 2 or 2^32) on about p_done of the
    env-steps and copied to the env's other row; where it is not set, agent 1's own word is sometimes set, which the rule ignores."""
    rng = np.random.default_rng(seed + 7 * rows + 1000 * W + pad)
    xs = rng.integers(0, 2 ** 32, (pushes, rows, W + pad), dtype=np.uint64).astype(np.uint32)
    N = rows // A
    words = np.array([1, 2, 1 << 32], np.int64)
    env = np.where(rng.random((pushes, N)) < p_done, words[rng.integers(0, 3, (pushes, N))], 0)
    dones = np.repeat(env, A, axis=1)
    if A == 2:
        stray = (rng.random((pushes, N)) < 0.3) & (env == 0)
        dones[:, 1::2][stray] = 1
    return xs, dones
